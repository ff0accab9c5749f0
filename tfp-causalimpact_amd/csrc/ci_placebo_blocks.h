// ci_placebo_blocks.h -- the placebo forecasts of ci_placebo.h for ANY block list with a state of at
// most 64 components (ci_session_summarize_placebo_blocks; DESIGN.md "Block-model filters").
//
// The model, the layout (a group of G lanes per filter, lane i owns a_i and row i of P in registers)
// and every step of the filter are those at the top of ci_predict_blocks.h.  When t reaches the
// series' next origin -- uniform over the wavefront -- the lane copies its share of the predicted
// moments (a_i, row i of P) and the group forecasts from the copy: the branch of ci_placebo.h, lines
// 10-27, with Z r and Z pz summed in the order of Z a (0, o_0, o_1, ..) and r, one component per
// lane, transformed like the mean.  The OUT selectors SUM, SPREAD, PIT and VAR and the zero slots
// are unchanged.  The group's lane 0 stores: the result is the [B * O, N] matrix, draws contiguous.
// The host checks o + H_b <= T for every origin before the launch: no step beyond the series is read.
//
// With an ENTRY TABLE (q.series_of; ci_session_pool_placebo_blocks) the grid's rows are entries as in
// ci_placebo.h: entry e filters series series_of[e] with the origins' row e and horizon[e] and writes
// rows e * O .. of its outputs.  That build has the selector SUM_VAR: from ONE forecast branch lane 0
// stores SUM into `out` and VAR into `var`, the expressions of the two selectors, both 0 where
// cnt == 0 and in the unused slots -- the filter runs once for both terms of a pooled sum.  The entry
// is uniform over the workgroup: every barrier is met by all 64 lanes as before.
#pragma once
#include <type_traits>

#include "ci_placebo.h"
#include "ci_predict_blocks.h"

namespace ci {

constexpr int PLACEBO_SUM_VAR = 4;  // (entry-table build only) SUM into `out` and VAR into `var`
constexpr int PLACEBO_SUM_VAR_HORIZONS = 5;  // (entry-table build only) SUM_VAR at every checkpoint of the entry's horizon row

struct PlaceboBlocksArgs {
  PlaceboArgs q;                   // q.p as PredBlocksArgs::p; q.series_of read by the entry-table build only
  BlockModel m;
};

struct PlaceboBlocksPoolArgs : PlaceboBlocksArgs {   // q.series_of [E], q.origins [E, O], q.horizon [E], q.p.out [E, O, N]: SUM
  double* var;                     // [E, O, N]: VAR
};

// The entry-table build at SEVERAL HORIZONS (ci_session_pool_placebo_horizons_blocks; the block-model
// twin of placebo_pool_horizons_kernel): the forecast branch runs to the last used horizon of
// horizons[e, .] and at every checkpoint h == horizons[e, k] lane 0 stores SUM into `out` and VAR into
// `var`, rows (e * O + slot) * K + k, with the expressions of SUM_VAR; 0 in the unused origin and
// horizon slots.  q.horizon is not read.  The checkpoint test is uniform over the workgroup -- the
// horizons belong to the entry -- and no barrier sits inside it.
struct PlaceboBlocksPoolHorizonsArgs : PlaceboBlocksPoolArgs {   // q.p.out, var: [E, O, K, N]
  int K;                           // horizon slots per entry
  const int* horizons;             // [E, K] strictly ascending, -1: unused (at the end)
};

// The launches (ci_placebo_blocks.hip): placebo_blocks_kernel<G, out> over B series; its entry-table
// builds <G, PLACEBO_SUM_VAR, PlaceboBlocksPoolArgs> and <G, PLACEBO_SUM_VAR_HORIZONS,
// PlaceboBlocksPoolHorizonsArgs> over E entries.
hipError_t placebo_blocks_launch(hipStream_t stream, int B, int out, const PlaceboBlocksArgs& args);
hipError_t placebo_blocks_pool_launch(hipStream_t stream, int E, const PlaceboBlocksPoolArgs& args);
hipError_t placebo_blocks_launch_f64(hipStream_t stream, int B, int out, const PlaceboBlocksArgs& args);
hipError_t placebo_blocks_pool_launch_f64(hipStream_t stream, int E, const PlaceboBlocksPoolArgs& args);
hipError_t placebo_blocks_pool_horizons_launch(hipStream_t stream, int E, const PlaceboBlocksPoolHorizonsArgs& args);
hipError_t placebo_blocks_pool_horizons_launch_f64(hipStream_t stream, int E, const PlaceboBlocksPoolHorizonsArgs& args);

// The series of grid row e: with an entry table that of entry e, else e itself.
template <bool ENTRIES>
__device__ __forceinline__ size_t pb_series_of(const PlaceboArgs& q, size_t e) {
  if constexpr (ENTRIES) return (size_t)q.series_of[e];
  else return e;
}

// grid (ceil(N / (64 / G)), B), block 64; as placebo_blocks_kernel<G, PLACEBO_SUM_VAR, PlaceboBlocksPoolArgs>
// (the entry-table build) (ceil(N / (64 / G)), E).
template <int G, int OUT, class ARGS = PlaceboBlocksArgs, class IN = float>
__global__ __launch_bounds__(64) void placebo_blocks_kernel(ARGS k) {
  constexpr bool HORIZONS = OUT == PLACEBO_SUM_VAR_HORIZONS;
  constexpr bool ENTRIES = OUT == PLACEBO_SUM_VAR || HORIZONS;
  static_assert((OUT == PLACEBO_SUM_VAR) == std::is_same<ARGS, PlaceboBlocksPoolArgs>::value, "SUM_VAR is the entry-table build's selector");
  static_assert(HORIZONS == std::is_same<ARGS, PlaceboBlocksPoolHorizonsArgs>::value, "SUM_VAR_HORIZONS is the several-horizons build's selector");
  constexpr int FPW = 64 / G;
  __shared__ PbShared sh;
  const PredArgs& p = k.q.p;
  const int N = p.N, T = p.T, NO = k.q.O;
  const int n_own = blockIdx.x * FPW + (int)threadIdx.x / G;
  const bool active = n_own < N;
  const int n = active ? n_own : N - 1;
  const size_t e = blockIdx.y;                   // the grid's row, uniform over the workgroup
  const size_t b = pb_series_of<ENTRIES>(k.q, e), bn = b * N + n;
  PbCtx c;
  double H, a, P[G];
  pb_begin<G, IN>(p, k.m, sh, b, bn, c, H, a, P);
  const bool writer = active && c.i == 0;
  const double scale = p.scales[b], shift = p.shifts[b];
  const IN* y = (const IN*)p.y + b * T;
  const uint8_t* mask = p.mask + b * T;
  const double* reg = p.reg ? p.reg + b * T * N + n : nullptr;
  double* out = p.out + e * NO * N + n;
  double* var = nullptr;
  if constexpr (ENTRIES) var = k.var + e * NO * N + n;
  const int* org = k.q.origins + e * NO;
  int Hb = 0, K = 1;                             // (HORIZONS) Hb: the row's last used horizon
  const int* hz = nullptr;
  if constexpr (HORIZONS) {
    K = k.K;
    hz = k.horizons + e * K;
    for (int i = 0; i < K; ++i) Hb = hz[i] > 0 ? hz[i] : Hb;
    out = p.out + e * NO * K * N + n;            // row (slot * K + kc) of the entry
    var = k.var + e * NO * K * N + n;
  } else {
    Hb = k.q.horizon[e];
  }

  int slot = 0;
  int next = org[0];                             // uniform over the wavefront, as everything of the origins
  double unused = 0.0;
  for (int t = 0; t < T && next >= 0; ++t) {
    if (t == next) {
      // the forecast branch, from a copy of the predicted moments
      double fa = a, r = 0.0, fP[G];
#pragma unroll
      for (int j = 0; j < G; ++j) fP[j] = P[j];
      double V = 0.0, C = 0.0, A = 0.0;
      int cnt = 0;
      int kc = 0, check = -1;                    // (HORIZONS) the next checkpoint: uniform, as the horizons
      if constexpr (HORIZONS) check = hz[0];
      for (int h = 0; h < Hb; ++h) {
        const int u = t + h;
        double pz, m, zpz;
        pb_moments<G>(c, fa, fP, pz, m, zpz);
        if (mask[u] == 0) {
          c.xc[c.lane] = r;                      // (its last readers passed the barriers of pb_moments)
          __syncthreads();
          const double zr = pb_zsum(c, c.xc);
          C += m + (reg ? reg[(size_t)u * N] : 0.0);
          if constexpr (!HORIZONS) A += (double)y[u];   // (the pooled terms hold no A)
          cnt += 1;
          V += (2.0 * zr + zpz) + H;
          r += pz;
        }
        if constexpr (HORIZONS) {
          if (h + 1 == check) {                  // no barrier in here
            double sum = 0.0, vr = 0.0;
            if (cnt > 0) {
              sum = __dadd_rn(__dmul_rn(C, scale), __dmul_rn((double)cnt, shift));
              vr = __dmul_rn(__dmul_rn(V, scale), scale);
            }
            if (writer) {
              const size_t at = ((size_t)slot * K + kc) * N;
              out[at] = sum;
              var[at] = vr;
            }
            ++kc;
            check = kc < K ? hz[kc] : -1;
          }
        }
        if (h + 1 >= Hb) break;
        pb_transition<G, true>(c, u, fa, r, fP);
      }
      if constexpr (HORIZONS) {
        if (writer)
          for (; kc < K; ++kc) {                 // the unused horizon slots
            const size_t at = ((size_t)slot * K + kc) * N;
            out[at] = 0.0;
            var[at] = 0.0;
          }
      } else {
        double res = 0.0;
        if (cnt > 0) {
          const double err = A - C;
          if (OUT == PLACEBO_SUM || OUT == PLACEBO_SUM_VAR) res = __dadd_rn(__dmul_rn(C, scale), __dmul_rn((double)cnt, shift));
          else if (OUT == PLACEBO_SPREAD) res = __dmul_rn(__dmul_rn(__dadd_rn(V, __dmul_rn(err, err)), scale), scale);
          else if (OUT == PLACEBO_VAR) res = __dmul_rn(__dmul_rn(V, scale), scale);
          else res = 0.5 * erfc(-err / sqrt(2.0 * V));
        }
        if (writer) out[(size_t)slot * N] = res;
        if constexpr (ENTRIES) {
          if (writer) var[(size_t)slot * N] = cnt > 0 ? __dmul_rn(__dmul_rn(V, scale), scale) : 0.0;
        }
      }
      ++slot;
      next = slot < NO ? org[slot] : -1;
      if (next < 0) break;
    }
    // the filter's step t (predict_blocks_kernel)
    double pz, m, zpz;
    pb_moments<G>(c, a, P, pz, m, zpz);
    if (mask[t] == 0) {
      const double F = zpz + H;
      const double f = m + (reg ? reg[(size_t)t * N] : 0.0);
      const double v = (double)y[t] - f;
      pb_update<G>(c, a, P, pz, F, v);
    }
    if (t + 1 >= T) break;
    pb_transition<G, false>(c, t, a, unused, P);
  }
  if constexpr (HORIZONS) {
    if (writer)
      for (size_t i = (size_t)slot * K; i < (size_t)NO * K; ++i) {   // the unused origin slots
        out[i * N] = 0.0;
        var[i * N] = 0.0;
      }
  } else {
    if constexpr (ENTRIES) {
      if (writer)
        for (int i = slot; i < NO; ++i) var[(size_t)i * N] = 0.0;
    }
    if (writer)
      for (; slot < NO; ++slot) out[(size_t)slot * N] = 0.0;
  }
}

// The SIMULATED placebo forecasts of ci_placebo.h (placebo_sim_kernel: its definition, line by line)
// for the block models: the branch is the filter's own step -- pb_moments, pb_update,
// pb_transition<G, false> -- on the copy, fed with v = sqrt(F) z.  Every lane of a group forms the
// same normal from the group's (chain, draw): nothing crosses lanes for it.  Lane 0 stores.
struct PlaceboBlocksSimArgs {
  PlaceboSimArgs s;                // s.q.p as PredBlocksArgs::p
  BlockModel m;
};

// The launches (ci_placebo_blocks.hip): placebo_blocks_sim_kernel<G, link> over nb series from
// args.s.b0, its ENTRIES build over E entries.
hipError_t placebo_blocks_sim_launch(hipStream_t stream, int nb, int link, const PlaceboBlocksSimArgs& args);
hipError_t placebo_blocks_sim_entries_launch(hipStream_t stream, int E, int link, const PlaceboBlocksSimArgs& args);
hipError_t placebo_blocks_sim_launch_f64(hipStream_t stream, int nb, int link, const PlaceboBlocksSimArgs& args);
hipError_t placebo_blocks_sim_entries_launch_f64(hipStream_t stream, int E, int link, const PlaceboBlocksSimArgs& args);

// grid (ceil(N / (64 / G)), series of the launch), block 64.  The entry-table build (ENTRIES;
// ci_session_pool_simulated_placebo_blocks) has the grid (ceil(N / (64 / G)), entries of the launch)
// and rows as placebo_sim_kernel's; the entry is uniform over the workgroup, so every barrier is met
// by all 64 lanes as before.
template <int G, int LINK, bool ENTRIES = false, class IN = float>
__global__ __launch_bounds__(64) void placebo_blocks_sim_kernel(PlaceboBlocksSimArgs k) {
  constexpr int FPW = 64 / G;
  __shared__ PbShared sh;
  const PredArgs& p = k.s.q.p;
  const int N = p.N, T = p.T, NO = k.s.q.O;
  const int n_own = blockIdx.x * FPW + (int)threadIdx.x / G;
  const bool active = n_own < N;
  const int n = active ? n_own : N - 1;
  const size_t e = blockIdx.y, b = ENTRIES ? (size_t)k.s.q.series_of[e] : (size_t)k.s.b0 + e, bn = b * N + n;
  const size_t plan = ENTRIES ? e : b;           // the row of the plan: origins [., O], horizon [.]
  PbCtx c;
  double H, a, P[G];
  pb_begin<G, IN>(p, k.m, sh, b, bn, c, H, a, P);
  const bool writer = active && c.i == 0;
  const double scale = p.scales[b], shift = p.shifts[b];
  const IN* y = (const IN*)p.y + b * T;
  const uint8_t* mask = p.mask + b * T;
  const double* reg = p.reg ? p.reg + b * T * N + n : nullptr;
  double* out = p.out + e * NO * N + n;
  int* counted = writer && n == 0 ? k.s.counted + e * NO : nullptr;
  const int* org = k.s.q.origins + plan * NO;
  const int Hb = k.s.q.horizon[plan];
  Rng rng;
  rng.k0 = k.s.keys[2 * b];
  rng.k1 = k.s.keys[2 * b + 1];
  rng.chain = k.s.chain_offset + (uint32_t)(n / k.s.kept);
  const uint32_t iter = (uint32_t)(n % k.s.kept);

  int slot = 0;
  int next = org[0];                             // uniform over the wavefront, as everything of the origins
  double unused = 0.0;
  for (int t = 0; t < T && next >= 0; ++t) {
    if (t == next) {
      // the simulated branch, from a copy of the predicted moments
      double fa = a, fP[G];
#pragma unroll
      for (int j = 0; j < G; ++j) fP[j] = P[j];
      double S = 0.0, z0 = 0.0, z1 = 0.0;
      U4 r4 = {0u, 0u, 0u, 0u};
      int cnt = 0;
      for (int h = 0; h < Hb; ++h) {
        const int u = t + h;
        const double z = placebo_sim_normal(rng, iter, (uint32_t)slot, h, r4, z0, z1);
        double pz, m, zpz;
        pb_moments<G>(c, fa, fP, pz, m, zpz);
        if (mask[u] == 0) {
          const double F = zpz + H;
          const double f = m + (reg ? reg[(size_t)u * N] : 0.0);
          const double v = __dmul_rn(sqrt(F), z);
          const double ysim = __dadd_rn(f, v);
          S += link_value<LINK>(__dadd_rn(__dmul_rn(ysim, scale), shift));
          cnt += 1;
          pb_update<G>(c, fa, fP, pz, F, v);
        }
        if (h + 1 >= Hb) break;
        pb_transition<G, false>(c, u, fa, unused, fP);
      }
      if (writer) out[(size_t)slot * N] = cnt > 0 ? S : 0.0;
      if (counted) counted[slot] = cnt;
      ++slot;
      next = slot < NO ? org[slot] : -1;
      if (next < 0) break;
    }
    // the filter's step t (predict_blocks_kernel)
    double pz, m, zpz;
    pb_moments<G>(c, a, P, pz, m, zpz);
    if (mask[t] == 0) {
      const double F = zpz + H;
      const double f = m + (reg ? reg[(size_t)t * N] : 0.0);
      const double v = (double)y[t] - f;
      pb_update<G>(c, a, P, pz, F, v);
    }
    if (t + 1 >= T) break;
    pb_transition<G, false>(c, t, a, unused, P);
  }
  for (; slot < NO; ++slot) {
    if (writer) out[(size_t)slot * N] = 0.0;
    if (counted) counted[slot] = 0;
  }
}

}  // namespace ci
