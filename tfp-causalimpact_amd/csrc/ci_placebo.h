// ci_placebo.h -- placebo forecasts of every fit of a finished session: for every series b, pooled
// draw n and ORIGIN o inside the observed series the H_b-step forecast of the window's sum without
// any update, in float64 (ci_session_summarize_placebo; DESIGN.md "Placebo forecasts").
//
// The model, the state space, Z, T_t, Q_t, reg[n, t] and the initial moments are those at the top of
// ci_predict.h, and so is the layout: one lane per (series, draw), a wavefront holds 64 consecutive
// draws of one series, templated on <HAS_SLOPE, NS, OUT> so that every array is a fully unrolled
// register array.  The lane runs the filter of ci_predict.h over t = 0, 1, ..; when t reaches the
// series' next origin -- uniform over the wavefront: the origins belong to the series -- it copies
// the predicted moments (a, P) of x_o given y[0 .. o - 1] and forecasts from the copy:
//   r = 0 (D components: Cov(S, x) of the running sum S), V = C = A = 0, cnt = 0
//   for h = 0 .. H_b - 1, t = o + h:
//     pz = P Z';  m = Z a
//     mask[t] == 0:  C += m + reg[n, t];  A += double(y[t]);  cnt += 1
//                    V += (2 (Z r) + Z pz) + sigma_obs^2;  r += pz
//     h + 1 < H_b:   a <- T_t a;  r <- T_t r;  P <- T_t P T_t' + Q_t
// C is the conditional mean of the sum of the counted observations, V its exact predictive variance
// for that draw (observation noise included).  Per (b, origin i, n), selected by OUT:
//   SUM    = C * scale[b] + cnt * shift[b]          (separate roundings)
//   SPREAD = ((V + (A - C)^2) * scale[b]) * scale[b]
//   PIT    = 0.5 erfc(-(A - C) / sqrt(2 V))
//   VAR    = (V * scale[b]) * scale[b]             (the variance alone: what a pooled sum adds up)
// An origin whose window counts no step, and a slot without origin (-1, at the end of the row),
// read 0 in all four.  The filter then goes on from the untouched (a, P) and stops after the
// series' last origin.  The result is the [B * O, N] matrix `out`, draws contiguous: what the
// row-statistics kernel reads.  The host checks o + H_b <= T_b for every origin before the launch:
// no step beyond the series is read.
//
// With an ENTRY TABLE (series_of; ci_session_pool_placebo) the grid's rows are entries of a group
// table instead of series: entry e filters series series_of[e] with the origins' row e and horizon[e],
// and writes rows e * O .. of `out`.  A series may be the member of several groups, each with origins
// and a horizon of its own.  placebo_pool_kernel then adds the entries' rows to the groups'
// accumulators and placebo_finish_kernel turns the accumulators into the three matrices of the
// pooled sum, N(S, U) given the members' draws:
//   e = seen - S;  SUM = S;  SPREAD = U + e^2;  PIT = 0.5 erfc(-e / sqrt(2 U));  all 0 where U == 0.
// The SIMULATED totals (below) pool over the same table (ci_session_pool_simulated_placebo): the
// ENTRIES build of placebo_sim_kernel simulates the entries' rows, placebo_pool_kernel<0, 1> adds them
// to one-plane accumulators, and the row statistics of the simulated placebo are taken over those.
#pragma once
#include "ci_link.h"
#include "ci_predict.h"
#include "ci_rng.h"

namespace ci {

enum PlaceboOut { PLACEBO_SUM = 0, PLACEBO_SPREAD = 1, PLACEBO_PIT = 2, PLACEBO_VAR = 3 };

struct PlaceboArgs {
  PredArgs p;                      // the filter's inputs; p.out [B, O, N], p.ll unused
  int O;                           // origin slots per series
  const int* origins;              // [B, O] strictly ascending, -1: unused (at the end)
  const int* horizon;              // [B]
  const int* series_of = nullptr;  // the entry table: [E] the series of every entry, origins [E, O],
                                   // horizon [E], p.out [E, O, N]; nullptr: entry b is series b
};

// The launches (ci_placebo.hip): placebo_kernel<has_slope, num_seasons, out> over B series or
// entries; placebo_pool_kernel<which> adding the rows of the entries c0 .. c1 - 1 in M to the groups'
// accumulators; placebo_finish_kernel<out> over the accumulators' rows r0 .. r0 + rows - 1 into M.
hipError_t placebo_launch(hipStream_t stream, int B, int has_slope, int num_seasons, int out,
                          const PlaceboArgs& args);
hipError_t placebo_launch_f64(hipStream_t stream, int B, int has_slope, int num_seasons, int out,
                              const PlaceboArgs& args);
hipError_t placebo_pool_launch(hipStream_t stream, int N, int O, int G, int which, int c0, int c1,
                               const int* offsets, const double* weights, const double* M, double* acc);
hipError_t placebo_finish_launch(hipStream_t stream, int N, size_t r0, size_t rows, int out,
                                 const double* acc, const double* seen, double* M);

// a <- T a, P <- T P T' + Q of step t -> t + 1 (the lines of predict_kernel): the trend's part, then
// the block's where `change` is set.
template <int HAS_SLOPE, int NS, int D>
__device__ __forceinline__ void placebo_propagate(double (&a)[D], double (&P)[D * (D + 1) / 2], bool change,
                                                  double q_level, double q_slope, double q_drift) {
#define PM(i, j) P[pred_sym<D>(i, j)]
  constexpr int N1 = NS ? NS - 1 : 0, O = 1 + HAS_SLOPE;
  if (HAS_SLOPE) {
    a[0] += a[1];
    const double p01 = PM(0, 1) + PM(1, 1);
    PM(0, 0) = (PM(0, 0) + PM(0, 1)) + p01;
    PM(0, 1) = p01;
#pragma unroll
    for (int j = 2; j < D; ++j) PM(0, j) += PM(1, j);
  }
  if constexpr (NS > 0) {
    if (change) pred_season_step<O, N1, D>(a, P, q_drift);
  }
  PM(0, 0) += q_level;
  if (HAS_SLOPE) PM(1, 1) += q_slope;
#undef PM
}

// grid (ceil(N / 64), B), block 64; with an entry table (ceil(N / 64), E).
template <int HAS_SLOPE, int NS, int OUT, class IN = float>
__global__ __launch_bounds__(64) void placebo_kernel(PlaceboArgs k) {
  constexpr int N1 = NS ? NS - 1 : 0, O = 1 + HAS_SLOPE, D = O + N1, NP = D * (D + 1) / 2;
  constexpr int ZS = O < D ? O : 0;              // the block's first effect (NS > 0)
  const int n = blockIdx.x * 64 + threadIdx.x, N = k.p.N, T = k.p.T, NO = k.O;
  const size_t e = blockIdx.y;
  const size_t b = k.series_of ? (size_t)k.series_of[e] : e;
  if (n >= N) return;
  const int Tb = k.p.series_T ? k.p.series_T[b] : T;
  const size_t bn = b * N + n;
  const double so = (double)((const IN*)k.p.obs)[bn], H = so * so;
  const double sl = (double)((const IN*)k.p.lscale)[bn], q_level = sl * sl;
  double q_slope = 0.0, q_drift = 0.0;
  if (HAS_SLOPE) {
    const double ss = (double)((const IN*)k.p.sscale)[bn];
    q_slope = ss * ss;
  }
  if (NS) {
    const double q = (double)((const IN*)k.p.drift)[bn] / (double)NS;
    q_drift = q * q;
  }
  const double scale = k.p.scales[b], shift = k.p.shifts[b];
  const double* init = k.p.init + 4 * b;
  const IN* y = (const IN*)k.p.y + b * T;
  const uint8_t* mask = k.p.mask + b * T;
  const double* reg = k.p.reg ? k.p.reg + b * T * N + n : nullptr;
  double* out = k.p.out + e * NO * N + n;
  const int* org = k.origins + e * NO;
  const int Hb = k.horizon[e];

  double a[D], P[NP];
#define PM(i, j) P[pred_sym<D>(i, j)]
#define FM(i, j) fP[pred_sym<D>(i, j)]
#pragma unroll
  for (int i = 0; i < D; ++i) a[i] = 0.0;
#pragma unroll
  for (int i = 0; i < NP; ++i) P[i] = 0.0;
  a[0] = init[0];
  PM(0, 0) = init[1];
  if (HAS_SLOPE) PM(1, 1) = init[2];
  if (NS) {
    const double v = init[3];
#pragma unroll
    for (int i = 0; i < N1; ++i)
#pragma unroll
      for (int j = i; j < N1; ++j) PM(O + i, O + j) = v * ((i == j ? 1.0 : 0.0) - 1.0 / (double)NS);
  }

  int slot = 0;
  int next = org[0];                             // uniform over the wavefront, as everything of the origins
  for (int t = 0; t < Tb && next >= 0; ++t) {
    if (t == next) {
      // the forecast branch, from a copy of the predicted moments
      double fa[D], fP[NP], r[D];
#pragma unroll
      for (int i = 0; i < D; ++i) fa[i] = a[i], r[i] = 0.0;
#pragma unroll
      for (int i = 0; i < NP; ++i) fP[i] = P[i];
      double V = 0.0, C = 0.0, A = 0.0;
      int cnt = 0;
      for (int h = 0; h < Hb; ++h) {
        const int u = t + h;
        double pz[D];
#pragma unroll
        for (int i = 0; i < D; ++i) pz[i] = NS ? FM(i, 0) + FM(i, ZS) : FM(i, 0);
        if (mask[u] == 0) {
          const double m = NS ? fa[0] + fa[ZS] : fa[0];
          const double zr = NS ? r[0] + r[ZS] : r[0];
          const double zpz = NS ? pz[0] + pz[ZS] : pz[0];
          C += m + (reg ? reg[(size_t)u * N] : 0.0);
          A += (double)y[u];
          cnt += 1;
          V += (2.0 * zr + zpz) + H;
#pragma unroll
          for (int i = 0; i < D; ++i) r[i] += pz[i];
        }
        if (h + 1 >= Hb) break;
        if (HAS_SLOPE) r[0] += r[1];
        bool change = false;
        if constexpr (NS > 0) {
          change = k.p.season_change[u] != 0;
          if (change) pred_season_rotate<O, N1, D>(r);
        }
        placebo_propagate<HAS_SLOPE, NS, D>(fa, fP, change, q_level, q_slope, q_drift);
      }
      double res = 0.0;
      if (cnt > 0) {
        const double err = A - C;
        if (OUT == PLACEBO_SUM) res = __dadd_rn(__dmul_rn(C, scale), __dmul_rn((double)cnt, shift));
        else if (OUT == PLACEBO_SPREAD) res = __dmul_rn(__dmul_rn(__dadd_rn(V, __dmul_rn(err, err)), scale), scale);
        else if (OUT == PLACEBO_VAR) res = __dmul_rn(__dmul_rn(V, scale), scale);
        else res = 0.5 * erfc(-err / sqrt(2.0 * V));
      }
      out[(size_t)slot * N] = res;
      ++slot;
      next = slot < NO ? org[slot] : -1;
      if (next < 0) break;
    }
    // the filter's step t (predict_kernel)
    double pz[D];
#pragma unroll
    for (int i = 0; i < D; ++i) pz[i] = NS ? PM(i, 0) + PM(i, ZS) : PM(i, 0);
    if (mask[t] == 0) {
      const double m = NS ? a[0] + a[ZS] : a[0];
      const double F = (NS ? pz[0] + pz[ZS] : pz[0]) + H;
      const double f = m + (reg ? reg[(size_t)t * N] : 0.0);
      const double v = (double)y[t] - f;
#pragma unroll
      for (int i = 0; i < D; ++i) a[i] += (pz[i] / F) * v;
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = i; j < D; ++j) PM(i, j) -= pz[i] * pz[j] / F;
    }
    if (t + 1 >= Tb) break;
    bool change = false;
    if constexpr (NS > 0) change = k.p.season_change[t] != 0;
    placebo_propagate<HAS_SLOPE, NS, D>(a, P, change, q_level, q_slope, q_drift);
  }
#undef PM
#undef FM
  for (; slot < NO; ++slot) out[(size_t)slot * N] = 0.0;
}

// ---- SIMULATED placebo forecasts (ci_session_simulate_placebo; DESIGN.md "Simulated placebo
// forecasts").  Under an outcome link the window's total is a sum of exp's of jointly Gaussian values
// and has no closed form, so one path of the window is drawn per posterior draw instead: by the chain
// rule y_{o+h} given the simulated y_o .. y_{o+h-1} is N(f_h, F_h) of a filter that is updated with
// the simulated values, so the forecast branch is the filter's own step fed with a draw from its own
// forecast -- no r, V, C, A, and no factor of P.  From the copy (a, P) of the predicted moments:
//   S = 0.0, cnt = 0
//   for h = 0 .. H_b - 1, u = o + h:
//     pz = P Z';  m = Z a;  F = Z pz + sigma_obs^2;  f = m + reg[n, u]
//     mask[u] == 0:  z = normal_d(key_b, chain_offset + n / S_kept, n % S_kept, SITE_PLACEBO_SIM, slot, h)
//                    v = sqrt(F) * z;  ysim = f + v                    (separate roundings)
//                    S += link(ysim * scale[b] + shift[b]);  cnt += 1  (two roundings, as ci_link.h)
//                    a += (pz / F) v;  P -= pz pz' / F                 (the filter's update)
//     h + 1 < H_b:   a <- T_u a;  P <- T_u P T_u' + Q_u
// TOTAL[b, slot, n] = S, 0.0 where cnt == 0 and in the unused slots.  idx of the normal is h whether
// or not the step is counted: one Philox call serves four consecutive h, its two Box-Muller pairs
// are formed when h reaches them.  Lane 0 of the grid's first column also stores cnt per (b, slot):
// the rows the statistics below leave at 0.
struct PlaceboSimArgs {
  PlaceboArgs q;                   // q.p.out [rows of this launch, N]; q.series_of read by the entry-table build only
  int b0;                          // the first series of this launch: grid row r is series b0 + r (no entry table)
  int kept;                        // S: kept draws per chain, n = c * S + s
  uint32_t chain_offset;           // the global id of the session's chain 0
  const uint32_t* keys;            // [B, 2]: the Philox key every series' fit ran on
  int* counted;                    // [rows of this launch]: cnt of (series, slot)
};

// The launches (ci_placebo.hip): placebo_sim_kernel<has_slope, num_seasons, link> over nb series from
// args.b0, its ENTRIES build over E entries; placebo_pool_kernel<0, 1> adding the entries' totals to
// one-plane accumulators; placebo_sim_seen_kernel<rewrite> over the rows of M.
hipError_t placebo_sim_launch(hipStream_t stream, int nb, int has_slope, int num_seasons, int link,
                              const PlaceboSimArgs& args);
hipError_t placebo_sim_entries_launch(hipStream_t stream, int E, int has_slope, int num_seasons, int link,
                                      const PlaceboSimArgs& args);
hipError_t placebo_sim_launch_f64(hipStream_t stream, int nb, int has_slope, int num_seasons, int link,
                                  const PlaceboSimArgs& args);
hipError_t placebo_sim_entries_launch_f64(hipStream_t stream, int E, int has_slope, int num_seasons, int link,
                                          const PlaceboSimArgs& args);
hipError_t placebo_pool_totals_launch(hipStream_t stream, int N, int O, int G, int c0, int c1,
                                      const int* offsets, const double* weights, const double* M, double* acc);
hipError_t placebo_sim_seen_launch(hipStream_t stream, size_t rows, int N, double* M, const double* seen,
                                   const int* counted, double* below, int rewrite);

// The normal of step h of a window: the Philox call of h >> 2 and the Box-Muller pair of h >> 1 are
// formed when h enters them and carried in (r, z0, z1) -- normal_d(g, iter, SITE_PLACEBO_SIM, sub, h).
__device__ __forceinline__ double placebo_sim_normal(const Rng& g, uint32_t iter, uint32_t sub, int h, U4& r,
                                                     double& z0, double& z1) {
  if ((h & 3) == 0) r = site_call(g, iter, SITE_PLACEBO_SIM, sub, (uint32_t)h >> 2);
  if ((h & 1) == 0) {
    const bool hi = (h & 2) != 0;
    box_muller_d(hi ? r.z : r.x, hi ? r.w : r.y, z0, z1);
  }
  return (h & 1) ? z1 : z0;
}

// grid (ceil(N / 64), series of the launch), block 64.  The entry-table build (ENTRIES) has the grid
// (ceil(N / 64), entries of the launch): row e simulates series q.series_of[e] from the origins' row e
// with q.horizon[e] and writes rows e * O .. of `out` and `counted` -- the tables of
// ci_session_pool_placebo, whose pointers the host sets to the launch's first entry; b0 is not
// read.  Everything else of the row, the Philox key included, is the series'.
template <int HAS_SLOPE, int NS, int LINK, bool ENTRIES = false, class IN = float>
__global__ __launch_bounds__(64) void placebo_sim_kernel(PlaceboSimArgs k) {
  constexpr int N1 = NS ? NS - 1 : 0, O = 1 + HAS_SLOPE, D = O + N1, NP = D * (D + 1) / 2;
  constexpr int ZS = O < D ? O : 0;              // the block's first effect (NS > 0)
  const PredArgs& p = k.q.p;
  const int n = blockIdx.x * 64 + threadIdx.x, N = p.N, T = p.T, NO = k.q.O;
  const size_t e = blockIdx.y, b = ENTRIES ? (size_t)k.q.series_of[e] : (size_t)k.b0 + e;
  const size_t plan = ENTRIES ? e : b;           // the row of the plan: origins [., O], horizon [.]
  if (n >= N) return;
  const int Tb = p.series_T ? p.series_T[b] : T;
  const size_t bn = b * N + n;
  const double so = (double)((const IN*)p.obs)[bn], H = so * so;
  const double sl = (double)((const IN*)p.lscale)[bn], q_level = sl * sl;
  double q_slope = 0.0, q_drift = 0.0;
  if (HAS_SLOPE) {
    const double ss = (double)((const IN*)p.sscale)[bn];
    q_slope = ss * ss;
  }
  if (NS) {
    const double q = (double)((const IN*)p.drift)[bn] / (double)NS;
    q_drift = q * q;
  }
  const double scale = p.scales[b], shift = p.shifts[b];
  const double* init = p.init + 4 * b;
  const IN* y = (const IN*)p.y + b * T;
  const uint8_t* mask = p.mask + b * T;
  const double* reg = p.reg ? p.reg + b * T * N + n : nullptr;
  double* out = p.out + e * NO * N + n;
  int* counted = n == 0 ? k.counted + e * NO : nullptr;
  const int* org = k.q.origins + plan * NO;
  const int Hb = k.q.horizon[plan];
  Rng rng;
  rng.k0 = k.keys[2 * b];
  rng.k1 = k.keys[2 * b + 1];
  rng.chain = k.chain_offset + (uint32_t)(n / k.kept);
  const uint32_t iter = (uint32_t)(n % k.kept);

  double a[D], P[NP];
#define PM(i, j) P[pred_sym<D>(i, j)]
#define FM(i, j) fP[pred_sym<D>(i, j)]
#pragma unroll
  for (int i = 0; i < D; ++i) a[i] = 0.0;
#pragma unroll
  for (int i = 0; i < NP; ++i) P[i] = 0.0;
  a[0] = init[0];
  PM(0, 0) = init[1];
  if (HAS_SLOPE) PM(1, 1) = init[2];
  if (NS) {
    const double v = init[3];
#pragma unroll
    for (int i = 0; i < N1; ++i)
#pragma unroll
      for (int j = i; j < N1; ++j) PM(O + i, O + j) = v * ((i == j ? 1.0 : 0.0) - 1.0 / (double)NS);
  }

  int slot = 0;
  int next = org[0];                             // uniform over the wavefront, as everything of the origins
  for (int t = 0; t < Tb && next >= 0; ++t) {
    if (t == next) {
      // the simulated branch, from a copy of the predicted moments
      double fa[D], fP[NP];
#pragma unroll
      for (int i = 0; i < D; ++i) fa[i] = a[i];
#pragma unroll
      for (int i = 0; i < NP; ++i) fP[i] = P[i];
      double S = 0.0, z0 = 0.0, z1 = 0.0;
      U4 r4 = {0u, 0u, 0u, 0u};
      int cnt = 0;
      for (int h = 0; h < Hb; ++h) {
        const int u = t + h;
        const double z = placebo_sim_normal(rng, iter, (uint32_t)slot, h, r4, z0, z1);
        double pz[D];
#pragma unroll
        for (int i = 0; i < D; ++i) pz[i] = NS ? FM(i, 0) + FM(i, ZS) : FM(i, 0);
        if (mask[u] == 0) {
          const double m = NS ? fa[0] + fa[ZS] : fa[0];
          const double F = (NS ? pz[0] + pz[ZS] : pz[0]) + H;
          const double f = m + (reg ? reg[(size_t)u * N] : 0.0);
          const double v = __dmul_rn(sqrt(F), z);
          const double ysim = __dadd_rn(f, v);
          S += link_value<LINK>(__dadd_rn(__dmul_rn(ysim, scale), shift));
          cnt += 1;
#pragma unroll
          for (int i = 0; i < D; ++i) fa[i] += (pz[i] / F) * v;
#pragma unroll
          for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = i; j < D; ++j) FM(i, j) -= pz[i] * pz[j] / F;
        }
        if (h + 1 >= Hb) break;
        bool change = false;
        if constexpr (NS > 0) change = p.season_change[u] != 0;
        placebo_propagate<HAS_SLOPE, NS, D>(fa, fP, change, q_level, q_slope, q_drift);
      }
      out[(size_t)slot * N] = cnt > 0 ? S : 0.0;
      if (counted) counted[slot] = cnt;
      ++slot;
      next = slot < NO ? org[slot] : -1;
      if (next < 0) break;
    }
    // the filter's step t (predict_kernel)
    double pz[D];
#pragma unroll
    for (int i = 0; i < D; ++i) pz[i] = NS ? PM(i, 0) + PM(i, ZS) : PM(i, 0);
    if (mask[t] == 0) {
      const double m = NS ? a[0] + a[ZS] : a[0];
      const double F = (NS ? pz[0] + pz[ZS] : pz[0]) + H;
      const double f = m + (reg ? reg[(size_t)t * N] : 0.0);
      const double v = (double)y[t] - f;
#pragma unroll
      for (int i = 0; i < D; ++i) a[i] += (pz[i] / F) * v;
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = i; j < D; ++j) PM(i, j) -= pz[i] * pz[j] / F;
    }
    if (t + 1 >= Tb) break;
    bool change = false;
    if constexpr (NS > 0) change = p.season_change[t] != 0;
    placebo_propagate<HAS_SLOPE, NS, D>(a, P, change, q_level, q_slope, q_drift);
  }
#undef PM
#undef FM
  for (; slot < NO; ++slot) {
    out[(size_t)slot * N] = 0.0;
    if (counted) counted[slot] = 0;
  }
}

// The statistics of the rows of TOTAL [rows, N] that need `seen` [rows]: one wavefront per row, four
// rows per workgroup (comp_row_stats_kernel's layout).
//   below[row] = #{n : TOTAL <= seen}, an integer count (exact in any order), stored as a double;
//   with REWRITE the row becomes (TOTAL - seen)^2 in place, one rounding per operation -- its row
//   mean is spread_mean.
// A row with counted == 0 (no step counted, or an unused slot) reads 0 in both and is left at 0.
template <int REWRITE>
__global__ __launch_bounds__(256) void placebo_sim_seen_kernel(size_t rows, int N, double* __restrict__ M,
                                                               const double* __restrict__ seen,
                                                               const int* __restrict__ counted,
                                                               double* __restrict__ below) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  double* x = M + row * N;
  int c = 0;
  if (counted[row] > 0) {                        // uniform over the wavefront
    const double s = seen[row];
    for (int i = lane; i < N; i += 64) {
      const double v = x[i];
      c += v <= s ? 1 : 0;
      if (REWRITE) {
        const double d = __dsub_rn(v, s);
        x[i] = __dmul_rn(d, d);
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
  if (lane == 0 && below) below[row] = (double)c;
}

// The entries c0 .. c1 - 1 of the group table, whose rows [(c1 - c0) * O, N] of one pass lie in M,
// added to the accumulators acc [G, O, 2, N] (S, then U): one lane per (group, slot, draw), the
// group's entries of this chunk in ascending order, one rounding per operation --
//   WHICH == 0 (M holds SUM):  S = S + w_k * s_k;    WHICH == 1 (M holds VAR):  U = U + (w_k * w_k) * v_k
// so the result depends neither on the launch geometry nor on where the entries are cut.
// grid (ceil(N / 64), min(G * O, 65535)), block 64.
// PLANES: the planes of a row of acc.  placebo_pool_kernel<0, 1> is the ONE-PLANE accumulate of
// ci_session_pool_simulated_placebo: M holds the entries' simulated totals, acc is [G, O, N] and
// POOL = POOL + w_k * TOTAL_k -- the arithmetic of WHICH == 0 on accumulators of stride N.
template <int WHICH, int PLANES = 2>
__global__ __launch_bounds__(64) void placebo_pool_kernel(int N, int O, size_t rows, int c0, int c1,
                                                          const int* __restrict__ offsets,
                                                          const double* __restrict__ weights,
                                                          const double* __restrict__ M,
                                                          double* __restrict__ acc) {
  static_assert(WHICH < PLANES, "the plane of this pass");
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  for (size_t row = blockIdx.y; row < rows; row += gridDim.y) {
    const size_t g = row / O, i = row - g * O;
    const int k0 = offsets[g] > c0 ? offsets[g] : c0;
    const int k1 = offsets[g + 1] < c1 ? offsets[g + 1] : c1;
    if (k0 >= k1) continue;
    double* at = acc + (row * PLANES + WHICH) * N + n;
    double a = *at;
    for (int k = k0; k < k1; ++k) {
      const double w = WHICH ? __dmul_rn(weights[k], weights[k]) : weights[k];
      a = __dadd_rn(a, __dmul_rn(w, M[((size_t)(k - c0) * O + i) * N + n]));
    }
    *at = a;
  }
}

// The rows r0 .. r0 + rows - 1 of the accumulators acc [G * O, 2, N] against seen [G * O]: the
// matrix OUT (PLACEBO_SUM, PLACEBO_SPREAD or PLACEBO_PIT of the pooled sum) [rows, N] in `out`.
// grid (ceil(N / 64), min(rows, 65535)), block 64.
template <int OUT>
__global__ __launch_bounds__(64) void placebo_finish_kernel(int N, size_t r0, size_t rows,
                                                            const double* __restrict__ acc,
                                                            const double* __restrict__ seen,
                                                            double* __restrict__ out) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  for (size_t r = blockIdx.y; r < rows; r += gridDim.y) {
    const size_t row = r0 + r;
    const double S = acc[row * 2 * N + n], U = acc[(row * 2 + 1) * N + n];
    double res = 0.0;
    if (U != 0.0) {
      const double err = seen[row] - S;
      if (OUT == PLACEBO_SUM) res = S;
      else if (OUT == PLACEBO_SPREAD) res = __dadd_rn(U, __dmul_rn(err, err));
      else res = 0.5 * erfc(-err / sqrt(2.0 * U));
    }
    out[r * N + n] = res;
  }
}

// ---- Placebo forecasts at SEVERAL HORIZONS in one filter pass (ci_session_summarize_placebo_horizons;
// DESIGN.md "Placebo forecasts at several horizons").  The running C, V, A and cnt of placebo_kernel's
// forecast loop after h steps are what a window of horizon h returns: the loop of H_b = h and the first
// h iterations of a longer one perform the same operations in the same order (the loop leaves before
// the propagation that would follow).  So the forecast of an origin runs to the row's LAST horizon and
// at every CHECKPOINT h == horizons[b, k] -- after the accumulation of step h - 1 -- the lane forms SUM,
// SPREAD and PIT with placebo_kernel's own expressions and stores all three:
//   out[(plane * rows + ((b - b0) * O + slot) * K + k) * N + n],  plane = PLACEBO_SUM, _SPREAD, _PIT
// -- three matrices [rows, N], draws contiguous, of rows = nb * O * K rows each for the nb series of
// the launch.  horizons [B, K]: strictly ascending, >= 1, -1 = unused, at the end of the row; the host
// checks o + (the row's last horizon) <= T_b for every origin.  The checkpoint test is uniform over
// the wavefront: horizons and origins belong to the series.  Unused origin slots and unused horizon
// slots read 0 in every plane.
struct PlaceboHorizonsArgs {
  PredArgs p;                      // the filter's inputs; p.out [3, rows, N], p.ll unused
  int O;                           // origin slots per series
  const int* origins;              // [B, O] strictly ascending, -1: unused (at the end)
  int K;                           // horizon slots per series
  const int* horizons;             // [B, K] strictly ascending, -1: unused (at the end)
  int b0;                          // the first series of this launch: grid row e is series b0 + e
  size_t rows;                     // nb * O * K: the rows of one plane
};

// The launch (ci_placebo.hip): placebo_horizons_kernel<has_slope, num_seasons> over nb series from
// args.b0; num_seasons 0 (no block) or 2..7.
hipError_t placebo_horizons_launch(hipStream_t stream, int nb, int has_slope, int num_seasons,
                                   const PlaceboHorizonsArgs& args);
hipError_t placebo_horizons_launch_f64(hipStream_t stream, int nb, int has_slope, int num_seasons,
                                       const PlaceboHorizonsArgs& args);

// grid (ceil(N / 64), series of the launch), block 64.
template <int HAS_SLOPE, int NS, class IN = float>
__global__ __launch_bounds__(64) void placebo_horizons_kernel(PlaceboHorizonsArgs k) {
  constexpr int N1 = NS ? NS - 1 : 0, O = 1 + HAS_SLOPE, D = O + N1, NP = D * (D + 1) / 2;
  constexpr int ZS = O < D ? O : 0;              // the block's first effect (NS > 0)
  const int n = blockIdx.x * 64 + threadIdx.x, N = k.p.N, T = k.p.T, NO = k.O, K = k.K;
  const size_t e = blockIdx.y, b = (size_t)k.b0 + e;
  if (n >= N) return;
  const int Tb = k.p.series_T ? k.p.series_T[b] : T;
  const size_t bn = b * N + n;
  const double so = (double)((const IN*)k.p.obs)[bn], H = so * so;
  const double sl = (double)((const IN*)k.p.lscale)[bn], q_level = sl * sl;
  double q_slope = 0.0, q_drift = 0.0;
  if (HAS_SLOPE) {
    const double ss = (double)((const IN*)k.p.sscale)[bn];
    q_slope = ss * ss;
  }
  if (NS) {
    const double q = (double)((const IN*)k.p.drift)[bn] / (double)NS;
    q_drift = q * q;
  }
  const double scale = k.p.scales[b], shift = k.p.shifts[b];
  const double* init = k.p.init + 4 * b;
  const IN* y = (const IN*)k.p.y + b * T;
  const uint8_t* mask = k.p.mask + b * T;
  const double* reg = k.p.reg ? k.p.reg + b * T * N + n : nullptr;
  const size_t plane = k.rows * N;               // the doubles of one plane
  double* out = k.p.out + e * NO * K * N + n;    // row (slot * K + kc) of the series, plane SUM
  const int* org = k.origins + b * NO;
  const int* hz = k.horizons + b * K;
  int Hb = 0;                                    // the row's last used horizon
  for (int i = 0; i < K; ++i) Hb = hz[i] > 0 ? hz[i] : Hb;

  double a[D], P[NP];
#define PM(i, j) P[pred_sym<D>(i, j)]
#define FM(i, j) fP[pred_sym<D>(i, j)]
#pragma unroll
  for (int i = 0; i < D; ++i) a[i] = 0.0;
#pragma unroll
  for (int i = 0; i < NP; ++i) P[i] = 0.0;
  a[0] = init[0];
  PM(0, 0) = init[1];
  if (HAS_SLOPE) PM(1, 1) = init[2];
  if (NS) {
    const double v = init[3];
#pragma unroll
    for (int i = 0; i < N1; ++i)
#pragma unroll
      for (int j = i; j < N1; ++j) PM(O + i, O + j) = v * ((i == j ? 1.0 : 0.0) - 1.0 / (double)NS);
  }

  int slot = 0;
  int next = org[0];                             // uniform over the wavefront, as everything of the origins
  for (int t = 0; t < Tb && next >= 0; ++t) {
    if (t == next) {
      // the forecast branch, from a copy of the predicted moments (placebo_kernel's, with checkpoints)
      double fa[D], fP[NP], r[D];
#pragma unroll
      for (int i = 0; i < D; ++i) fa[i] = a[i], r[i] = 0.0;
#pragma unroll
      for (int i = 0; i < NP; ++i) fP[i] = P[i];
      double V = 0.0, C = 0.0, A = 0.0;
      int cnt = 0;
      double* row = out + (size_t)slot * K * N;
      int kc = 0;
      int check = hz[0];                         // the next checkpoint: uniform, as the horizons
      for (int h = 0; h < Hb; ++h) {
        const int u = t + h;
        double pz[D];
#pragma unroll
        for (int i = 0; i < D; ++i) pz[i] = NS ? FM(i, 0) + FM(i, ZS) : FM(i, 0);
        if (mask[u] == 0) {
          const double m = NS ? fa[0] + fa[ZS] : fa[0];
          const double zr = NS ? r[0] + r[ZS] : r[0];
          const double zpz = NS ? pz[0] + pz[ZS] : pz[0];
          C += m + (reg ? reg[(size_t)u * N] : 0.0);
          A += (double)y[u];
          cnt += 1;
          V += (2.0 * zr + zpz) + H;
#pragma unroll
          for (int i = 0; i < D; ++i) r[i] += pz[i];
        }
        if (h + 1 == check) {
          double sum = 0.0, spread = 0.0, pit = 0.0;
          if (cnt > 0) {
            const double err = A - C;
            sum = __dadd_rn(__dmul_rn(C, scale), __dmul_rn((double)cnt, shift));
            spread = __dmul_rn(__dmul_rn(__dadd_rn(V, __dmul_rn(err, err)), scale), scale);
            pit = 0.5 * erfc(-err / sqrt(2.0 * V));
          }
          double* at = row + (size_t)kc * N;
          at[0] = sum;
          at[plane] = spread;
          at[2 * plane] = pit;
          ++kc;
          check = kc < K ? hz[kc] : -1;
        }
        if (h + 1 >= Hb) break;
        if (HAS_SLOPE) r[0] += r[1];
        bool change = false;
        if constexpr (NS > 0) {
          change = k.p.season_change[u] != 0;
          if (change) pred_season_rotate<O, N1, D>(r);
        }
        placebo_propagate<HAS_SLOPE, NS, D>(fa, fP, change, q_level, q_slope, q_drift);
      }
      for (; kc < K; ++kc) {                     // the unused horizon slots
        double* at = row + (size_t)kc * N;
        at[0] = 0.0;
        at[plane] = 0.0;
        at[2 * plane] = 0.0;
      }
      ++slot;
      next = slot < NO ? org[slot] : -1;
      if (next < 0) break;
    }
    // the filter's step t (predict_kernel)
    double pz[D];
#pragma unroll
    for (int i = 0; i < D; ++i) pz[i] = NS ? PM(i, 0) + PM(i, ZS) : PM(i, 0);
    if (mask[t] == 0) {
      const double m = NS ? a[0] + a[ZS] : a[0];
      const double F = (NS ? pz[0] + pz[ZS] : pz[0]) + H;
      const double f = m + (reg ? reg[(size_t)t * N] : 0.0);
      const double v = (double)y[t] - f;
#pragma unroll
      for (int i = 0; i < D; ++i) a[i] += (pz[i] / F) * v;
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = i; j < D; ++j) PM(i, j) -= pz[i] * pz[j] / F;
    }
    if (t + 1 >= Tb) break;
    bool change = false;
    if constexpr (NS > 0) change = k.p.season_change[t] != 0;
    placebo_propagate<HAS_SLOPE, NS, D>(a, P, change, q_level, q_slope, q_drift);
  }
#undef PM
#undef FM
  for (size_t i = (size_t)slot * K; i < (size_t)NO * K; ++i) {   // the unused origin slots
    double* at = out + i * N;
    at[0] = 0.0;
    at[plane] = 0.0;
    at[2 * plane] = 0.0;
  }
}

// ---- The POOLED terms at several horizons in one filter pass (ci_session_pool_placebo_horizons;
// DESIGN.md "Pooled placebo forecasts at several horizons").  The entry-table build of the kernel
// above: grid row e filters series series_of[e] from the origins' row e and runs the forecast branch
// to the last used horizon of horizons[e, .] -- the row of the entry's group, handed in per entry as
// PlaceboArgs::horizon is.  At every checkpoint h == horizons[e, k] the lane stores the two terms a
// pooled sum adds up, with placebo_kernel's expressions and roundings:
//   SUM = C * scale[b] + cnt * shift[b] (separate roundings);  VAR = (V * scale[b]) * scale[b]
// both 0 where cnt == 0, in the unused origin slots and in the unused horizon slots.  No A, no erfc:
// the observed sums enter at placebo_finish_kernel.  Two planes of `rows` = E * O * K rows each,
//   out[(plane * rows + (e * O + slot) * K + k) * N + n],  plane 0 SUM, 1 VAR
// so that placebo_pool_kernel and placebo_finish_kernel read them with O * K in the place of O.
struct PlaceboPoolHorizonsArgs {
  PredArgs p;                      // the filter's inputs; p.out [2, rows, N], p.ll unused
  int O;                           // origin slots per entry
  const int* origins;              // [E, O] strictly ascending, -1: unused (at the end)
  int K;                           // horizon slots per entry
  const int* horizons;             // [E, K] strictly ascending, -1: unused (at the end)
  const int* series_of;            // [E] the series of every entry
  size_t rows;                     // E * O * K: the rows of one plane
};

// The launch (ci_placebo.hip): placebo_pool_horizons_kernel<has_slope, num_seasons> over E entries;
// num_seasons 0 (no block) or 2..7.
hipError_t placebo_pool_horizons_launch(hipStream_t stream, int E, int has_slope, int num_seasons,
                                        const PlaceboPoolHorizonsArgs& args);
hipError_t placebo_pool_horizons_launch_f64(hipStream_t stream, int E, int has_slope, int num_seasons,
                                            const PlaceboPoolHorizonsArgs& args);

// grid (ceil(N / 64), entries of the launch), block 64.
template <int HAS_SLOPE, int NS, class IN = float>
__global__ __launch_bounds__(64) void placebo_pool_horizons_kernel(PlaceboPoolHorizonsArgs k) {
  constexpr int N1 = NS ? NS - 1 : 0, O = 1 + HAS_SLOPE, D = O + N1, NP = D * (D + 1) / 2;
  constexpr int ZS = O < D ? O : 0;              // the block's first effect (NS > 0)
  const int n = blockIdx.x * 64 + threadIdx.x, N = k.p.N, T = k.p.T, NO = k.O, K = k.K;
  const size_t e = blockIdx.y, b = (size_t)k.series_of[e];
  if (n >= N) return;
  const int Tb = k.p.series_T ? k.p.series_T[b] : T;
  const size_t bn = b * N + n;
  const double so = (double)((const IN*)k.p.obs)[bn], H = so * so;
  const double sl = (double)((const IN*)k.p.lscale)[bn], q_level = sl * sl;
  double q_slope = 0.0, q_drift = 0.0;
  if (HAS_SLOPE) {
    const double ss = (double)((const IN*)k.p.sscale)[bn];
    q_slope = ss * ss;
  }
  if (NS) {
    const double q = (double)((const IN*)k.p.drift)[bn] / (double)NS;
    q_drift = q * q;
  }
  const double scale = k.p.scales[b], shift = k.p.shifts[b];
  const double* init = k.p.init + 4 * b;
  const IN* y = (const IN*)k.p.y + b * T;
  const uint8_t* mask = k.p.mask + b * T;
  const double* reg = k.p.reg ? k.p.reg + b * T * N + n : nullptr;
  const size_t plane = k.rows * N;               // the doubles of one plane
  double* out = k.p.out + e * NO * K * N + n;    // row (slot * K + kc) of the entry, plane SUM
  const int* org = k.origins + e * NO;
  const int* hz = k.horizons + e * K;
  int Hb = 0;                                    // the row's last used horizon
  for (int i = 0; i < K; ++i) Hb = hz[i] > 0 ? hz[i] : Hb;

  double a[D], P[NP];
#define PM(i, j) P[pred_sym<D>(i, j)]
#define FM(i, j) fP[pred_sym<D>(i, j)]
#pragma unroll
  for (int i = 0; i < D; ++i) a[i] = 0.0;
#pragma unroll
  for (int i = 0; i < NP; ++i) P[i] = 0.0;
  a[0] = init[0];
  PM(0, 0) = init[1];
  if (HAS_SLOPE) PM(1, 1) = init[2];
  if (NS) {
    const double v = init[3];
#pragma unroll
    for (int i = 0; i < N1; ++i)
#pragma unroll
      for (int j = i; j < N1; ++j) PM(O + i, O + j) = v * ((i == j ? 1.0 : 0.0) - 1.0 / (double)NS);
  }

  int slot = 0;
  int next = org[0];                             // uniform over the wavefront, as everything of the entry
  for (int t = 0; t < Tb && next >= 0; ++t) {
    if (t == next) {
      // the forecast branch, from a copy of the predicted moments (placebo_kernel's, with checkpoints)
      double fa[D], fP[NP], r[D];
#pragma unroll
      for (int i = 0; i < D; ++i) fa[i] = a[i], r[i] = 0.0;
#pragma unroll
      for (int i = 0; i < NP; ++i) fP[i] = P[i];
      double V = 0.0, C = 0.0;
      int cnt = 0;
      double* row = out + (size_t)slot * K * N;
      int kc = 0;
      int check = hz[0];                         // the next checkpoint: uniform, as the horizons
      for (int h = 0; h < Hb; ++h) {
        const int u = t + h;
        double pz[D];
#pragma unroll
        for (int i = 0; i < D; ++i) pz[i] = NS ? FM(i, 0) + FM(i, ZS) : FM(i, 0);
        if (mask[u] == 0) {
          const double m = NS ? fa[0] + fa[ZS] : fa[0];
          const double zr = NS ? r[0] + r[ZS] : r[0];
          const double zpz = NS ? pz[0] + pz[ZS] : pz[0];
          C += m + (reg ? reg[(size_t)u * N] : 0.0);
          cnt += 1;
          V += (2.0 * zr + zpz) + H;
#pragma unroll
          for (int i = 0; i < D; ++i) r[i] += pz[i];
        }
        if (h + 1 == check) {
          double sum = 0.0, var = 0.0;
          if (cnt > 0) {
            sum = __dadd_rn(__dmul_rn(C, scale), __dmul_rn((double)cnt, shift));
            var = __dmul_rn(__dmul_rn(V, scale), scale);
          }
          double* at = row + (size_t)kc * N;
          at[0] = sum;
          at[plane] = var;
          ++kc;
          check = kc < K ? hz[kc] : -1;
        }
        if (h + 1 >= Hb) break;
        if (HAS_SLOPE) r[0] += r[1];
        bool change = false;
        if constexpr (NS > 0) {
          change = k.p.season_change[u] != 0;
          if (change) pred_season_rotate<O, N1, D>(r);
        }
        placebo_propagate<HAS_SLOPE, NS, D>(fa, fP, change, q_level, q_slope, q_drift);
      }
      for (; kc < K; ++kc) {                     // the unused horizon slots
        double* at = row + (size_t)kc * N;
        at[0] = 0.0;
        at[plane] = 0.0;
      }
      ++slot;
      next = slot < NO ? org[slot] : -1;
      if (next < 0) break;
    }
    // the filter's step t (predict_kernel)
    double pz[D];
#pragma unroll
    for (int i = 0; i < D; ++i) pz[i] = NS ? PM(i, 0) + PM(i, ZS) : PM(i, 0);
    if (mask[t] == 0) {
      const double m = NS ? a[0] + a[ZS] : a[0];
      const double F = (NS ? pz[0] + pz[ZS] : pz[0]) + H;
      const double f = m + (reg ? reg[(size_t)t * N] : 0.0);
      const double v = (double)y[t] - f;
#pragma unroll
      for (int i = 0; i < D; ++i) a[i] += (pz[i] / F) * v;
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = i; j < D; ++j) PM(i, j) -= pz[i] * pz[j] / F;
    }
    if (t + 1 >= Tb) break;
    bool change = false;
    if constexpr (NS > 0) change = k.p.season_change[t] != 0;
    placebo_propagate<HAS_SLOPE, NS, D>(a, P, change, q_level, q_slope, q_drift);
  }
#undef PM
#undef FM
  for (size_t i = (size_t)slot * K; i < (size_t)NO * K; ++i) {   // the unused origin slots
    double* at = out + i * N;
    at[0] = 0.0;
    at[plane] = 0.0;
  }
}

}  // namespace ci
