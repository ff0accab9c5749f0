// ci_gibbs.hip -- the Gibbs session of the C-ABI (include/causalimpact_amd.h) over the HIP kernels:
// ci_session_create* (plan the route, allocate, upload), run, streamed run, fetch, profile, and
// ci_fit_gibbs on top of them; the component test entry points.  Plain HIP runtime: no torch, no
// TensorFlow.  One ci_session == one device-resident fit.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ci_session.h"
#include "ci_kernels8.h"
#include "ci_wide.h"
#include "ci_seasonal_tp.h"
#include "ci_setup.h"

namespace ci {
// ------------------------------------------------------------------------------------
// component test kernels
// ------------------------------------------------------------------------------------
static __global__ void test_rng_kernel(uint32_t k0, uint32_t k1, uint32_t chain, uint32_t iter,
                                uint32_t site, uint32_t sub, int n, float* uni, float* nor,
                                double alpha, double* gam) {
  Rng g{k0, k1, chain};
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += blockDim.x) {
    uni[i] = (float)uniform_d(g, iter, site, sub, (uint32_t)i);
    float z[1];
    fill_normals<1>(g, iter, site, sub, (uint32_t)i, z);
    nor[i] = z[0];
  }
  if (tid < 64) {
    const double v = gamma_wave(alpha, g, iter, site, sub, tid);
    if (tid == 0) gam[0] = v;
    // also exercise the 4-wide path: normals via fill_normals<4> must agree with <1>
    float z4[4];
    fill_normals<4>(g, iter, site, sub, (uint32_t)(tid * 4), z4);
    for (int q = 0; q < 4; ++q)
      if (tid * 4 + q < n) nor[n + tid * 4 + q] = z4[q];
  }
}

// ------------------------------------------------------------------------------------
// the tail of a streamed fit (ci_session_run_streamed): what is left when the sampler ends
// ------------------------------------------------------------------------------------
// One result array's share of the tail: nseg runs of seg_len floats, seg_stride floats apart, at
// the same offsets in source (HBM) and destination (the device address of pinned host memory).
struct TailSeg {
  float* dst;
  const float* src;
  unsigned long long seg_len, seg_stride;
  unsigned int nseg;
};
constexpr int TAIL_MAX = 10;        // the members of ci_outputs
constexpr int TAIL_PART = 1024;     // floats per work item: one float4 per thread
constexpr int TAIL_BLOCKS = 64;     // workgroups per array
struct TailArgs { TailSeg e[TAIL_MAX]; };

// Launched with grid (TAIL_BLOCKS, arrays) behind the sampler on its stream: writes the rows of the
// last chunk and the arrays without a time axis straight into the caller's pinned buffers, with
// 16-byte stores wherever source and destination are aligned alike.
static __global__ __launch_bounds__(256) void tail_gather_kernel(TailArgs a) {
  const TailSeg e = a.e[blockIdx.y];
  const size_t parts = (e.seg_len + TAIL_PART - 1) / TAIL_PART;
  const size_t items = parts * e.nseg;
  const size_t tid = threadIdx.x;
  for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
    const size_t seg = it / parts, lo = (it % parts) * TAIL_PART;
    const size_t n = e.seg_len - lo < (size_t)TAIL_PART ? e.seg_len - lo : (size_t)TAIL_PART;
    float* d = e.dst + seg * e.seg_stride + lo;
    const float* s = e.src + seg * e.seg_stride + lo;
    size_t head = (4 - (((uintptr_t)d >> 2) & 3)) & 3;      // floats up to d's 16-byte boundary
    if (head > n || (((uintptr_t)(s + head)) & 15) != 0) head = n;   // (s not aligned like d: all scalar)
    for (size_t i = tid; i < head; i += blockDim.x) d[i] = s[i];
    const size_t nv = (n - head) / 4;
    const float4* s4 = reinterpret_cast<const float4*>(s + head);
    float4* d4 = reinterpret_cast<float4*>(d + head);
    for (size_t i = tid; i < nv; i += blockDim.x) d4[i] = s4[i];
    for (size_t i = head + nv * 4 + tid; i < n; i += blockDim.x) d[i] = s[i];
  }
}

}  // namespace ci

extern "C" {

int ci_abi_version(void) { return CI_ABI_VERSION; }

void ci_series_stream_key(const uint32_t seed[2], int32_t series_id, uint32_t key[2]) {
  key[0] = ci::stream_key0(seed[0], 0, series_id);
  key[1] = ci::stream_key1(seed[1], 0, series_id);
}

// Releases a half-built session when ci_session_create leaves through an error path.
struct SessionGuard {
  ci_session* s;
  ~SessionGuard() { if (s) ci_session_destroy(s); }
};

// The lengths (3 to the stride T) and the ids (>= 0, when given) of a ragged session's series.
static int check_lengths(const ci_problem* pb, const int32_t* series_lengths, const int32_t* series_ids,
                         int* longest) {
  for (int b = 0; b < pb->num_series; ++b) {
    const int tb = series_lengths[b];
    if (tb < 3) return fail("series_lengths[%d] must be >= 3, got %d", b, tb);
    if (tb > pb->T) return fail("series_lengths[%d] = %d exceeds the stride T=%d", b, tb, pb->T);
    if (tb > *longest) *longest = tb;
    if (series_ids && series_ids[b] < 0) return fail("series_ids[%d] must be >= 0, got %d", b, series_ids[b]);
  }
  return 0;
}

// Everything ci_session_create_ragged checks, before any device call.
static int validate_ragged(const ci_problem* pb, const int32_t* series_lengths, const int32_t* series_ids) {
  if (validate(pb)) return 1;
  if (!series_lengths) return fail("series_lengths is NULL");
  if (pb->num_blocks > 0)
    return fail("ragged sessions hold trend models only: num_blocks must be 0, got %d", pb->num_blocks);
  if (pb->P > ci::MAXP)
    return fail("ragged sessions take at most %d design columns, got P=%d", ci::MAXP, pb->P);
  const int L = steps_per_thread(pb->T);
  if (L == 0)
    return fail("ragged sessions take series of at most %d steps, got T=%d", ci::NT * 16, pb->T);
  int longest = 0;
  if (check_lengths(pb, series_lengths, series_ids, &longest)) return 1;
  if (longest != pb->T)
    return fail("T must be the longest series of the session: max(series_lengths) = %d, T = %d",
                longest, pb->T);
  for (int b = 0; b < pb->num_series; ++b)
    if (steps_per_thread(series_lengths[b]) != L)
      return fail("series_lengths[%d] = %d runs %d steps per thread, the longest series (%d) runs %d: "
                  "all series of a ragged session must share that class",
                  b, series_lengths[b], steps_per_thread(series_lengths[b]), pb->T, L);
  return 0;
}

// Everything ci_session_create_ragged_seasonal checks, before any device call.
static int validate_ragged_seasonal(const ci_problem* pb, const int32_t* series_lengths,
                                    const int32_t* series_ids, const uint8_t* season_change) {
  if (validate(pb)) return 1;
  if (!series_lengths) return fail("series_lengths is NULL");
  if (!season_change) return fail("season_change is NULL");
  if (pb->num_blocks != 1)
    return fail("ragged seasonal sessions hold trend plus one seasonal block: num_blocks must be 1, got %d",
                pb->num_blocks);
  if (pb->num_seasons[0] < 2 || pb->num_seasons[0] > 7)
    return fail("ragged seasonal sessions take a block of 2 to 7 seasons, got num_seasons[0]=%d",
                pb->num_seasons[0]);
  if (pb->P > ci::MAXP)
    return fail("ragged seasonal sessions take at most %d design columns, got P=%d", ci::MAXP, pb->P);
  if ((pb->T & 3) != 0)
    return fail("the stride T of a ragged seasonal session must be a multiple of 4, got T=%d", pb->T);
  // (T <= 65536: validate() has refused a longer series of this model already)
  int longest = 0;
  if (check_lengths(pb, series_lengths, series_ids, &longest)) return 1;
  if (longest <= pb->T - 4)
    return fail("T must be the longest series of the session rounded up to a multiple of 4: "
                "max(series_lengths) = %d, T = %d", longest, pb->T);
  const int Lc = ci::wide_quad_steps(longest);
  for (int b = 0; b < pb->num_series; ++b)
    if (ci::wide_quad_steps(series_lengths[b]) != Lc)
      return fail("series_lengths[%d] = %d runs chunks of %d steps, the longest series (%d) chunks of %d: "
                  "all series of a ragged seasonal session must share that class",
                  b, series_lengths[b], ci::wide_quad_steps(series_lengths[b]), longest, Lc);
  // (a single fit of the model would not run the time-parallel kernel under any of these)
  if (pb->flags & CI_FLAG_SEQUENTIAL_SEASONAL)
    return fail("ragged seasonal sessions do not take CI_FLAG_SEQUENTIAL_SEASONAL");
  if (pb->flags & CI_FLAG_CLUSTER_SEASONAL)
    return fail("ragged seasonal sessions do not take CI_FLAG_CLUSTER_SEASONAL");
  if (pb->flags & CI_FLAG_MULTIWAVE_SEASONAL)
    return fail("ragged seasonal sessions do not take CI_FLAG_MULTIWAVE_SEASONAL");
  if (pb->flags & CI_FLAG_SEASONAL_WORKSPACE)
    return fail("ragged seasonal sessions do not take CI_FLAG_SEASONAL_WORKSPACE");
  return 0;
}

}  // extern "C"

// ---- 1. plan: the route, a function of the problem, `ragged` and the device's CU count ----------
// Fills every route field of the session (kpb / inert_block, L, x_in_lds, pm, eight_waves, wide, mw,
// tp, seasonal_gws, Lc, cluster, dk_lds, lds_bytes, lds_prof, the workspace sizes, fn, fn_prof,
// fn_prof8, kernel_name; sched_word from $CI_SCHED_WORD).  No device call, no allocation.
static int plan_route(ci_session* s, int num_cus) {
  const bool ragged = s->ragged;
  // Trend-only series longer than the register-resident kernel holds (T > 4096) run on the
  // time-parallel kernel (ci_wide.h) with one INERT seasonal block: 2 seasons, zero initial
  // variance, no season changes => its effect is identically 0, the model and every random
  // number of the trend / regression draws are unchanged (the block's own drift-scale draw uses
  // its own Philox site).
  s->kpb = s->pb;
  // More than MAXP design columns: every model runs on the sequential one-wavefront kernel, whose
  // regression block then keeps its O(P^2) arrays in a per-chain HBM workspace (any T as well).
  const bool bigp = s->pb.P > ci::MAXP;
  // (53+ columns, trend only: the BIGP build of that kernel, at any length -- wide_bigp_ok)
  s->inert_block = s->pb.num_blocks == 0 &&
                   ((steps_per_thread(s->pb.T) == 0 && !bigp) || wide_bigp_ok(&s->pb));
  if (s->inert_block) {
    s->kpb.num_blocks = 1;
    s->kpb.num_seasons[0] = 2;
    s->kpb.flags &= ~CI_FLAG_SEQUENTIAL_SEASONAL;
  }
  const ci_problem* pb = &s->kpb;
  const int T = pb->T, P = pb->P, B = pb->num_series, C = pb->num_chains;
  const int D = pb->has_slope ? 2 : 1;
  const int K = pb->num_blocks;
  char nm[96];
  if (K == 0 && !bigp) {
    s->L = steps_per_thread(T);
    // X lives in LDS when the whole layout fits in 160 KiB (leave room for a second block).
    const ci::LdsLayout with_x = ci::make_layout(P, D, ci::NT * s->L, 1);
    s->x_in_lds = (P > 0 && with_x.total <= 150 * 1024) ? 1 : 0;
    s->lds_bytes = ci::make_layout(P, D, ci::NT * s->L, s->x_in_lds).total;
    // P <= 16: the register-resident regression block, with the design in LDS or -- long series --
    // streamed from L2; beyond 16 columns the LDS block drawn by the whole workgroup
    const int pm = (P == 0) ? 0 : (P <= 16 ? (s->x_in_lds ? 1 : 3) : 2);
    s->pm = pm;
    // (x_in_lds and pm are functions of P and the steps-per-thread class alone: a ragged session
    //  makes the choices of a single fit of any of its series)
    const CiInst* inst = ci_inst(D, s->L);
    const CiRaggedInst* rinst = ci_ragged_inst(D, s->L);
    if (!inst || !rinst) return fail("no kernel for L=%d", s->L);
    s->fn = (KernelFn)(ragged ? rinst->gibbs(pm) : inst->gibbs(pm));
    s->fn_prof = ragged ? nullptr : (KernelFn)inst->gibbs(pm + 8);   // instrumented variant (ci_session_profile)
    if (!s->fn || (!ragged && !s->fn_prof)) return fail("no kernel for L=%d", s->L);
    // the instrumented variant is always the four-wave kernel: its own LDS layout
    s->lds_prof = s->lds_bytes;
    snprintf(nm, sizeof(nm), ragged ? "ci::gibbs_kernel<%d,%d,%d,false,ragged>" : "ci::gibbs_kernel<%d,%d,%d,false>",
             D, s->L, pm);
    s->kernel_name = nm;
    // latency build (ci_kernels8.h): eight wavefronts per chain -- four time waves, a regression
    // wave that owns the serial section and sweeps the next iteration's matrix during the draw,
    // three randomness waves.  Same draws, bit for bit (shared functions for everything that
    // rounds, -ffp-contract=on; tested across the CU-count boundary), so choosing by launch size
    // never changes a result.
    // ... when every chain has a compute unit to itself: eight 256-register wavefronts fill a CU,
    // the four-wave kernel leaves room for two workgroups, so launches with more workgroups than
    // CUs (batches of series: throughput, not latency) keep the four-wave kernel
    const bool latency_regime = (long long)B * C <= (long long)num_cus;
    // (ragged sessions always take the four-wave kernel: same bits, only the timing differs)
    if ((pm == 1 || pm == 3) && latency_regime && !(pb->flags & CI_FLAG_FOUR_WAVES) && !ragged) {
      // the design in LDS when it fits beside the randomness buffers, else read from L2 (the
      // same sums in the same order: the same bits)
      size_t base8 = 0;
      KernelFn f8 = (KernelFn)inst->gibbs8(0, 0, &base8);
      size_t lds8 = base8 + (size_t)P * ci::NT * s->L * sizeof(float);
      int xg = 0;
      if (!f8 || lds8 > 160 * 1024) {
        f8 = (KernelFn)inst->gibbs8(0, 1, &base8);
        lds8 = base8;
        xg = 1;
      }
      if (f8 && lds8 <= 160 * 1024) {
        s->fn = f8;
        s->fn_prof8 = xg ? nullptr : (KernelFn)inst->gibbs8(1, 0, nullptr);
        s->eight_waves = true;
        // Experiment / test knob (tools/exp_sched.py, the schedule-independence test): a
        // replacement for the helper waves' schedule word.  Read ONCE here, never on the launch
        // path, and only a well-formed word is accepted -- a stray variable cannot silently change
        // the production schedule.
        if (const char* e_ = getenv("CI_SCHED_WORD")) {
          char* end_ = nullptr;
          const long v_ = strtol(e_, &end_, 0);
          if (end_ == e_ || *end_ != 0 || v_ < 0 || v_ > 0xFFFF)
            return fail("CI_SCHED_WORD must be an integer in [0, 65535], got '%s'", e_);
          s->sched_word = (int)v_;
        }
        s->lds_bytes = lds8;
        snprintf(nm, sizeof(nm), xg ? "ci::gibbs_kernel8<%d,%d,L2>" : "ci::gibbs_kernel8<%d,%d>", D, s->L);
        s->kernel_name = nm;
      }
    }
    return 0;
  }
  s->D_full = D;
  s->dred = D;
  for (int k = 0; k < K; ++k) { s->D_full += pb->num_seasons[k]; s->dred += pb->num_seasons[k] - 1; }
  const long long groups = ((long long)B * C + 7) / 8 * 8;
  s->wide = use_wide(pb);
  if (s->wide) {
    s->Lc = ci::wide_quad_steps(T);
    s->lds_bytes = ci::make_wlayout(P, s->dred).total;
    const CiWideInst* wi = ci_wide_inst(D, pb->num_seasons[0]);
    const CiKernelInst* ki = bigp ? ci_wide_bigp_inst(D, pb->num_seasons[0])
                                  : ragged ? ci_wide_ragged_inst(D, pb->num_seasons[0]) : nullptr;
    s->fn = (KernelFn)(bigp || ragged ? (ki ? ki->gibbs : nullptr) : (wi ? wi->gibbs : nullptr));
  } else {
    // arrays over time in LDS when the whole layout fits (fastest), else in a per-chain HBM
    // workspace: no bound on the series length, and room in LDS for the P > 16 regression block.
    // States of more than 64 components (or CI_FLAG_MULTIWAVE_SEASONAL): the multi-wavefront
    // build, a function of the model alone like every route
    s->mw = s->D_full > 64 || (pb->flags & CI_FLAG_MULTIWAVE_SEASONAL) != 0;
    const int nwv = s->mw ? ci::MW_NWV : 1;
    const ci::SLayout in_lds = ci::make_slayout(T, P, K, s->D_full, s->dred, pb->has_slope, 0, nwv);
    s->seasonal_gws = in_lds.total > 150 * 1024 || (pb->flags & CI_FLAG_SEASONAL_WORKSPACE) != 0;
    const ci::SLayout lay = ci::make_slayout(T, P, K, s->D_full, s->dred, pb->has_slope,
                                             s->seasonal_gws ? 1 : 0, nwv);
    s->lds_bytes = lay.total;
    s->seasonal_ws_bytes = ((lay.t_total + 255) & ~(size_t)255) + (bigp ? ci::bigp_workspace_bytes(P) : 0);
  }
  // Any other block list -- and trend models with more than MAXP design columns -- with a state
  // of at most 32 components: the TIME-PARALLEL kernel of ci_seasonal_tp.h, a cluster of up to 32
  // workgroups of 4 wavefronts per chain (one chunk of the series per wavefront).  The ROUTE is a
  // function of the model and the series alone (T, D, P) -- never of the launch size or the device's
  // CU count: the two seasonal kernels agree only up to float summation order, and a series of a
  // batch must reproduce fit_causalimpact on that series alone bit for bit, on any device.  The
  // launch size only decides how many real workgroups share a chain's chunks (same bits).
  // (measured, round 5: below ~110 steps the one-wavefront kernel is as fast or faster -- 158 us
  // against 171 us at T = 96 on the 4+7+6 model, 202 us against 174 us at T = 128)
  const int tp_min_t = P > ci::MAXP ? 64 : 112;
  if (ragged && !(s->wide && !bigp && s->fn))
    return fail("ragged seasonal sessions run the time-parallel kernel only (one block of 2 to 7 seasons, P <= %d)", ci::MAXP);
  if (!s->wide && !s->mw && s->D_full <= ci::TP_MAXD && T >= tp_min_t && !(pb->flags & CI_FLAG_SEQUENTIAL_SEASONAL) &&
      !(pb->flags & CI_FLAG_SEASONAL_WORKSPACE)) {
    const ci::TpLds tl = ci::make_tplds(P, s->D_full);
    if (tl.total <= 160 * 1024) {
      // the chunk grid (G virtual workgroups of TP_NWV chunks) depends on the series alone; the
      // launch size only decides how many real workgroups (Gc) share them: same bits either way
      int G = 1;
      while (G < ci::TP_MAXG && T / (2 * G * ci::TP_NWV) >= 16) G *= 2;
      int Gc = 1;
      if (!(pb->flags & CI_FLAG_NO_CLUSTER))
        while (Gc < G && groups * (2 * Gc) <= num_cus) Gc *= 2;
      s->tp = true;
      s->cluster = Gc;
      s->Lc = G;
      s->lds_bytes = tl.total;
      s->tp_ws_bytes = ci::make_tplayout(T, P, K, s->D_full, pb->has_slope, G).total;
      const CiKernelInst* ti = ci_seasonal_tp_inst(ci::tp_nr(s->D_full) / 4);   // register rows of 4 nq columns
      s->fn = (KernelFn)(ti ? ti->gibbs : nullptr);
    }
  }
  if (s->lds_bytes > 160 * 1024) {
    return fail("seasonal model needs %zu bytes of LDS per chain (max 163840): fewer covariates "
                "or a narrower seasonal state", s->lds_bytes);
  }
  if (s->wide) {
    // clusters: 8, 4 or 2 CUs per chain while every workgroup of the launch is resident at once
    // (the handshakes spin); needs whole 16-byte chunks of 4 steps and a regression block
    // (a ragged session: one workgroup per chain -- clusters need T_b % 4 == 0 of every series, and
    //  every cluster size gives the same bits)
    if (!(pb->flags & CI_FLAG_NO_CLUSTER) && P > 0 && (T & 3) == 0 && !ragged) {
      if (groups * 16 <= num_cus) s->cluster = 16;
      else if (groups * 8 <= num_cus) s->cluster = 8;
      else if (groups * 4 <= num_cus) s->cluster = 4;
      else if (groups * 2 <= num_cus) s->cluster = 2;
    }
    if ((s->cluster == 16 || s->cluster == 8) && getenv("CI_WIDE_DK_GLOBAL") == nullptr) {
      // the draw's workers other than main are helpers whose LDS holds no regression matrices
      const size_t need = ci::make_wlayout(P, s->dred).big0 + ci::wide_dk_lds_bytes(s->Lc);
      if (need <= 160 * 1024 - 256) {
        s->dk_lds = 1;
        if (need > s->lds_bytes) s->lds_bytes = need;
      }
    }
  }
  if (!s->wide && !s->tp) {
    const int which = (s->seasonal_gws ? 1 : 0) | (bigp ? 2 : 0);
    s->fn = (KernelFn)(s->mw ? ci_gibbs_seasonal_mw_fn(which) : ci_gibbs_seasonal_fn(which));
  }
  if (!s->fn) return fail("no kernel for this seasonal model");
  if (s->tp) snprintf(nm, sizeof(nm), "ci::gibbs_seasonal_tp_kernel<%d> %d chunks x%d", ci::tp_nr(s->D_full) / 4,
                      s->Lc * ci::TP_NWV, s->cluster);
  else if (s->wide) snprintf(nm, sizeof(nm), bigp ? "ci::gibbs_wide_kernel<%d,%d,bigp>" : ragged ? "ci::gibbs_wide_kernel<%d,%d,ragged>" : "ci::gibbs_wide_kernel<%d,%d>", D, pb->num_seasons[0]);
  else if (s->mw) snprintf(nm, sizeof(nm), "ci::gibbs_seasonal_kernel<%s,%s,%d> (multi-wave)",
                           s->seasonal_gws ? "true" : "false", bigp ? "true" : "false", ci::MW_NWV);
  else snprintf(nm, sizeof(nm), "ci::gibbs_seasonal_kernel<%s,%s>", s->seasonal_gws ? "true" : "false",
                bigp ? "true" : "false");
  s->kernel_name = nm;
  return 0;
}

// ---- 2. allocate: every device buffer the route needs -------------------------------------------
static int session_allocate(ci_session* s, bool with_series_ids) {
  const ci_problem* pb = &s->kpb;
  const int T = pb->T, P = pb->P, B = pb->num_series, C = pb->num_chains, S = pb->num_results;
  const int K = pb->num_blocks;
  const size_t BT = (size_t)B * T, BCS = (size_t)B * C * S;
  HIP_TRY(s->y.alloc(BT));
  HIP_TRY(s->mask.alloc(BT));
  HIP_TRY(s->Xt.alloc((size_t)B * P * T));
  HIP_TRY(s->xtx.alloc((size_t)B * P * P));
  HIP_TRY(s->omega.alloc((size_t)B * P * P));
  HIP_TRY(s->wps.alloc(B));
  HIP_TRY(s->sp.alloc(B));
  HIP_TRY(s->o_obs.alloc(BCS));
  HIP_TRY(s->o_lscale.alloc(BCS));
  HIP_TRY(s->o_sscale.alloc(BCS));
  HIP_TRY(s->o_w.alloc(BCS * P));
  HIP_TRY(s->o_level.alloc(BCS * T));
  HIP_TRY(s->o_slope.alloc(pb->has_slope ? BCS * T : 0));
  HIP_TRY(s->o_pm.alloc((size_t)B * C * T));
  HIP_TRY(s->o_traj.alloc(BCS * T));
  if (s->ragged) {
    HIP_TRY(s->series_T.alloc(B));
    if (with_series_ids) HIP_TRY(s->series_ids.alloc(B));
  }
  if (K == 0 && P <= ci::MAXP) return 0;
  HIP_TRY(s->season_change.alloc((size_t)K * T));
  HIP_TRY(s->ssp.alloc(B));
  HIP_TRY(s->p1_chol.alloc((size_t)B * s->dred * s->dred));
  if (!s->inert_block) {
    HIP_TRY(s->o_drift.alloc(BCS * K));
    HIP_TRY(s->o_seasonal.alloc(BCS * T * K));
  }
  if (s->wide) {
    HIP_TRY(s->ws.alloc((size_t)B * C * ci::wide_workspace_floats(s->dred, s->Lc)));
    const size_t nseg = ((size_t)(T >> 2) + ci::NT - 1) / ci::NT;
    const size_t RS = (size_t)(P > 16 ? P : 16) + 4;
    HIP_TRY(s->csync.alloc((size_t)B * C * ci::CL_INTS));
    HIP_TRY(s->cpart.alloc((size_t)B * C * (nseg > 0 ? nseg : 1) * ci::NW * RS));
    HIP_TRY(s->cw.alloc((size_t)B * C * ci::wide_cw_floats(P)));
    HIP_TRY(s->cv.alloc((size_t)B * C * ci::wide_cv_doubles(P)));
  } else if (s->tp) {
    HIP_TRY(s->ws.alloc((size_t)B * C * (s->tp_ws_bytes / sizeof(float))));
    HIP_TRY(s->csync.alloc((size_t)B * C * ci::TPC_INTS));
  } else if (s->seasonal_ws_bytes > 0) {
    HIP_TRY(s->ws.alloc((size_t)B * C * (s->seasonal_ws_bytes / sizeof(float))));
  }
  return 0;
}

// ---- 3. upload: the staged inputs and the per-series parameter blocks ---------------------------
// (yh: y with the masked steps zeroed; sph, wps: the per-series blocks -- staged by the caller)
static int session_upload(ci_session* s, const std::vector<float>& yh,
                          const std::vector<ci::DevSeriesParams>& sph, const std::vector<double>& wps,
                          const int32_t* series_lengths,
                          const int32_t* series_ids, const uint8_t* mask, const float* X,
                          const uint8_t* season_change, const ci_series_params* params) {
  const ci_problem* pb = &s->kpb;
  const int T = pb->T, P = pb->P, B = pb->num_series, K = pb->num_blocks;
  const size_t BT = (size_t)B * T;
  if (s->ragged) {
    // Elements [T_b, T) of the per-step outputs are never written by the kernel: cleared here,
    // once, so that they read 0 after every run.
    HIP_TRY(hipMemset(s->o_level.p, 0, s->o_level.n * sizeof(float)));
    if (s->o_slope.n) HIP_TRY(hipMemset(s->o_slope.p, 0, s->o_slope.n * sizeof(float)));
    HIP_TRY(hipMemset(s->o_pm.p, 0, s->o_pm.n * sizeof(float)));
    HIP_TRY(hipMemset(s->o_traj.p, 0, s->o_traj.n * sizeof(float)));
    if (s->o_seasonal.n) HIP_TRY(hipMemset(s->o_seasonal.p, 0, s->o_seasonal.n * sizeof(float)));
    HIP_TRY(hipMemcpy(s->series_T.p, series_lengths, B * sizeof(int), hipMemcpyHostToDevice));
    if (series_ids) HIP_TRY(hipMemcpy(s->series_ids.p, series_ids, B * sizeof(int), hipMemcpyHostToDevice));
  }
  if (K > 0 || P > ci::MAXP) {
    // (the inert block of a long trend-only series never changes season)
    const std::vector<uint8_t> no_changes(s->inert_block ? (size_t)T : 0, 0);
    if (K > 0)
      HIP_TRY(hipMemcpy(s->season_change.p, s->inert_block ? no_changes.data() : season_change, (size_t)K * T,
                        hipMemcpyHostToDevice));
    std::vector<ci::DevSeasonalParams> ssh(B);
    std::vector<float> ch((size_t)B * s->dred * s->dred, 0.f);
    for (int b = 0; b < B; ++b) {
      ssh[b] = dev_seasonal_params(params[b], s->inert_block);
      const std::vector<float> cf = prior_chol_reduced(pb, params[b], s->dred, s->inert_block);
      std::copy(cf.begin(), cf.end(), ch.begin() + (size_t)b * s->dred * s->dred);
    }
    HIP_TRY(hipMemcpy(s->ssp.p, ssh.data(), B * sizeof(ci::DevSeasonalParams), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->p1_chol.p, ch.data(), ch.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(s->y.p, yh.data(), BT * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s->mask.p, mask, BT, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s->sp.p, sph.data(), B * sizeof(ci::DevSeriesParams), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s->wps.p, wps.data(), B * sizeof(double), hipMemcpyHostToDevice));
  if (P > 0) {
    const std::vector<float> xt = transpose_design<float>(B, T, P, X);
    HIP_TRY(hipMemcpy(s->Xt.p, xt.data(), xt.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  return 0;
}

static int session_create_impl(const ci_problem* pb, const int32_t* series_lengths,
                               const int32_t* series_ids, const float* y, const uint8_t* mask,
                               const float* X, const uint8_t* season_change,
                               const ci_series_params* params, ci_session** out) {
  if (!y || !mask || !params || !out) return fail("NULL argument");
  if (pb->num_blocks > 0 && !season_change) return fail("season_change is NULL but num_blocks > 0");
  if (pb->P > 0 && !X) return fail("X is NULL but P=%d", pb->P);
  // host-side staging: zero masked outcomes, count observations (rows [T_b, T) of a ragged series
  // are padding); checked before the first device call
  const int B = pb->num_series;
  std::vector<float> yh;
  std::vector<double> n_obs, wps(B);
  std::vector<ci::DevSeriesParams> sph(B);
  if (stage_outcomes<float>(B, pb->T, series_lengths, y, mask, yh, n_obs)) return 1;
  if (check_weights_prior_scale(params, B)) return 1;
  for (int b = 0; b < B; ++b) {
    sph[b] = dev_series_params(params[b], n_obs[b]);
    wps[b] = params[b].weights_prior_scale;
  }
  HIP_TRY(hipSetDevice(pb->device));
  ci_session* s = new ci_session();
  SessionGuard guard{s};
  s->pb = *pb;
  s->ragged = series_lengths != nullptr;
  if (s->ragged) s->lengths.assign(series_lengths, series_lengths + B);
  if (series_ids) s->ids.assign(series_ids, series_ids + B);
  s->params.assign(params, params + B);
  if (plan_route(s, device_cu_count(pb->device))) return 1;
  // one LDS limit per function, after the route is complete
  HIP_TRY(hipFuncSetAttribute((const void*)s->fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)s->lds_bytes));
  if (s->fn_prof8)
    HIP_TRY(hipFuncSetAttribute((const void*)s->fn_prof8, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)s->lds_bytes));
  if (s->fn_prof)
    HIP_TRY(hipFuncSetAttribute((const void*)s->fn_prof, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)s->lds_prof));
  HIP_TRY(pool_stream_get(&s->stream));
  HIP_TRY(pool_event_get(&s->ev0));
  HIP_TRY(pool_event_get(&s->ev1));
  if (session_allocate(s, series_ids != nullptr)) return 1;
  if (session_upload(s, yh, sph, wps, series_lengths, series_ids, mask, X, season_change, params)) return 1;
  guard.s = nullptr;
  *out = s;
  return 0;
}

extern "C" {

int ci_session_create(const ci_problem* pb, const float* y, const uint8_t* mask, const float* X,
                      const uint8_t* season_change, const ci_series_params* params,
                      ci_session** out) {
  if (validate(pb)) return 1;
  return session_create_impl(pb, nullptr, nullptr, y, mask, X, season_change, params, out);
}

int ci_session_create_ragged(const ci_problem* pb, const int32_t* series_lengths,
                             const int32_t* series_ids, const float* y, const uint8_t* mask,
                             const float* X, const ci_series_params* params, ci_session** out) {
  if (validate_ragged(pb, series_lengths, series_ids)) return 1;
  return session_create_impl(pb, series_lengths, series_ids, y, mask, X, nullptr, params, out);
}

int ci_session_create_ragged_seasonal(const ci_problem* pb, const int32_t* series_lengths,
                                      const int32_t* series_ids, const float* y, const uint8_t* mask,
                                      const float* X, const uint8_t* season_change,
                                      const ci_series_params* params, ci_session** out) {
  if (validate_ragged_seasonal(pb, series_lengths, series_ids, season_change)) return 1;
  return session_create_impl(pb, series_lengths, series_ids, y, mask, X, season_change, params, out);
}

static int session_launch(ci_session* s) {
  const ci_problem& pb = s->pb;
  HIP_TRY(hipSetDevice(pb.device));
  ci::KArgs a;
  fill_kargs(a, pb.T, pb.P, pb.num_warmup, pb.num_results, pb.num_chains, pb.num_series, pb.chain_offset,
             series_stream_base(pb), pb.seed);
  fill_kargs_buffers(a, (const float*)s->y.p, s->mask.p, (const float*)s->Xt.p, s->xtx.p, s->omega.p, s->sp.p,
                     s->outputs());
  a.x_in_lds = s->x_in_lds;
  a.progress = s->progress_every > 0 ? s->progress : nullptr;
  a.progress_every = s->progress_every > 0 ? s->progress_every : 1;
  a.dbg = s->sched_word;
  a.series_T = s->series_T.p;          // (null unless the session is ragged)
  a.series_ids = s->series_ids.p;
  if (s->profile) {
    if (!s->prof.p) HIP_TRY(s->prof.alloc(32));
    HIP_TRY(hipMemsetAsync(s->prof.p, 0, 32 * sizeof(long long), s->stream));
    a.prof = s->prof.p;
  }
  if (pb.P > 0) {
    hipLaunchKernelGGL(ci::setup_regression_kernel<float>, dim3(pb.num_series * pb.P * pb.P), dim3(64), 0,
                       s->stream, pb.T, pb.P, s->Xt.p, s->mask.p, s->wps.p, s->xtx.p, s->omega.p,
                       (const int*)s->series_T.p);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(s->ev0, s->stream));
  const ci_problem& kpb = s->kpb;
  if (kpb.num_blocks > 0 || kpb.P > ci::MAXP) {
    ci::SArgs sa;
    memset(&sa, 0, sizeof(sa));       // (lat_theta = NULL: the Gibbs sampler, not the latents-only mode)
    sa.k = a;
    sa.K = kpb.num_blocks; sa.has_slope = kpb.has_slope; sa.dred = s->dred;
    for (int k = 0; k < ci::SMAXK; ++k) sa.nseas[k] = k < kpb.num_blocks ? kpb.num_seasons[k] : 0;
    sa.season_change = s->season_change.p; sa.ssp = s->ssp.p; sa.p1_chol = s->p1_chol.p;
    sa.out_drift = s->o_drift.p; sa.out_seasonal = s->o_seasonal.p;
    sa.ws = s->ws.p; sa.Lc = s->Lc;
    sa.ws_stride = s->tp ? s->tp_ws_bytes : (s->wide ? 0 : s->seasonal_ws_bytes);
    sa.cluster = (s->wide || s->tp) ? s->cluster : 1;
    sa.cluster_drop = (pb.flags & CI_FLAG_TEST_DROP_HELPER) ? sa.cluster - 1 : 0;
    sa.dk_lds = s->wide ? s->dk_lds : 0;
    sa.csync = s->csync.p; sa.cpart = s->cpart.p; sa.cw = s->cw.p; sa.cv = s->cv.p;
    int grid = pb.num_series * pb.num_chains;
    if ((s->wide || s->tp) && s->cluster > 1) {
      HIP_TRY(hipMemsetAsync(s->csync.p, 0, s->csync.n * sizeof(int), s->stream));
      grid = (grid + 7) / 8 * 8 * s->cluster;       // (chain, role) <- workgroup id: see ci_wide.h
    }
    const int nthr = s->tp ? ci::TP_NT : (s->wide ? ci::NT : (s->mw ? 64 * ci::MW_NWV : 64));
    hipLaunchKernelGGL((void (*)(ci::SArgs))s->fn, dim3(grid), dim3(nthr),
                       s->lds_bytes, s->stream, sa);
  } else {
    if (s->profile && s->eight_waves && s->fn_prof8) {
      hipLaunchKernelGGL(s->fn_prof8, dim3(pb.num_series * pb.num_chains), dim3(ci::NT8), s->lds_bytes,
                         s->stream, a);
    } else if (s->profile && s->fn_prof) {
      // the instrumented variant is the four-wave kernel (its own LDS layout)
      hipLaunchKernelGGL(s->fn_prof, dim3(pb.num_series * pb.num_chains), dim3(ci::NT), s->lds_prof,
                         s->stream, a);
    } else {
      hipLaunchKernelGGL(s->fn, dim3(pb.num_series * pb.num_chains),
                         dim3(s->eight_waves ? ci::NT8 : ci::NT), s->lds_bytes, s->stream, a);
    }
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev1, s->stream));
  return 0;
}


int ci_session_run(ci_session* s, float* kernel_ms) {
  if (!s) return fail("session is NULL");
  if (refuse_draws_session(s, "ci_session_run")) return 1;
  s->progress_every = 0;
  if (session_launch(s)) return 1;
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, s->ev0, s->ev1));
  s->ran = true;
  return 0;
}

// The [B*C, S, T] arrays of a session, paired with the caller's buffers.
struct BigPair { float* dst; const float* src; size_t row; };
// An array without a time axis per draw: complete, like the last chunk, when the sampler ends.
struct SmallPair { float* dst; const float* src; size_t n; };

// Tails of up to this many bytes go through tail_gather_kernel, larger ones to the copy engines
// (with chunk_draws >= S the whole result is "the last chunk").  -DCI_TAIL_GATHER_MAX_BYTES=0
// builds the library without the kernel's use: every tail through copies behind the wait on ev1.
// Measured at cfg2's shape (T = 1000, P = 11, 8 chains, three [S, T] arrays to pinned memory;
// profiles/streamed_tail_parent_vs_branch.jsonl, "kind": "tail_sweep"), step time minus kernel
// time in us, copies -> kernel: 1.25 MB 168 -> 73, 2.0 MB 147 -> 65, 3.1 MB 146 -> 83, 6.3 MB
// 202 -> 140, 12.5 MB 311 -> 257, 25 MB 542 -> 481, 50 MB 982 -> 936, 96 MB (chunk_draws = S)
// 1798 -> 1775.  Both move the bytes at the link's rate (~55 GB/s); what the kernel saves is a
// constant 50-95 us of command latency.  Up to 12.5 MB that is 17 % of the tail or more; beyond
// 16 MiB it is a tenth or less, paid for with up to 640 workgroups held for the length of a PCIe
// transfer on a device other sessions may be sampling on -- there the copy engines keep the work.
#ifndef CI_TAIL_GATHER_MAX_BYTES
#define CI_TAIL_GATHER_MAX_BYTES (16u << 20)
#endif

// The device's address of `p` if `p` is the start of a block of pinned host memory that kernels
// can write; NULL for pageable (or unknown) memory, which only a staged copy reaches.
static float* pinned_device_address(float* p) {
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof(at));
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();        // an unregistered pointer is no error of this fit
    return nullptr;
  }
  if (at.type != hipMemoryTypeHost || at.hostPointer != (void*)p) return nullptr;
  return (float*)at.devicePointer;
}

// Leaves both streams of a streamed run idle when the run is left early.
struct StreamsIdle {
  ci_session* s;
  ~StreamsIdle() {
    if (!s) return;
    (void)hipStreamSynchronize(s->copy_stream);
    (void)hipStreamSynchronize(s->stream);
  }
};

int ci_session_run_streamed(ci_session* s, ci_outputs* o, int32_t chunk_draws, float* kernel_ms) {
  if (!s || !o) return fail("NULL argument");
  if (refuse_draws_session(s, "ci_session_run_streamed")) return 1;
  if (chunk_draws < 1) return fail("chunk_draws must be >= 1, got %d", chunk_draws);
  if (s->ragged) return fail("ci_session_run_streamed does not take ragged sessions: use ci_session_run and ci_session_fetch");
  const ci_problem& pb = s->pb;
  HIP_TRY(hipSetDevice(pb.device));
  const int S = pb.num_results, T = pb.T, K = pb.num_blocks;
  const size_t BC = (size_t)pb.num_series * pb.num_chains;
  if (!s->copy_stream) HIP_TRY(pool_stream_get(&s->copy_stream));
  // the register-resident kernel publishes its progress; the seasonal kernels do not (their
  // results are copied in the same chunks once the kernel has finished)
  const bool live = s->kpb.num_blocks == 0 && s->kpb.P <= ci::MAXP;
  if (live) {
    if (!s->progress)
      HIP_TRY(hipHostMalloc((void**)&s->progress, BC * sizeof(unsigned int), hipHostMallocCoherent));
    for (size_t i = 0; i < BC; ++i) s->progress[i] = 0u;
    s->progress_every = chunk_draws;
  } else {
    s->progress_every = 0;
  }
  if (session_launch(s)) { s->progress_every = 0; return 1; }
  s->progress_every = 0;
  std::vector<BigPair> big;
  if (o->level) big.push_back({o->level, s->o_level.p, (size_t)T});
  if (o->slope && pb.has_slope) big.push_back({o->slope, s->o_slope.p, (size_t)T});
  if (o->posterior_trajectories) big.push_back({o->posterior_trajectories, s->o_traj.p, (size_t)T});
  if (o->seasonal_levels && s->o_seasonal.n) big.push_back({o->seasonal_levels, s->o_seasonal.p, (size_t)T * K});
  const SmallPair small[] = {
      {o->observation_noise_scale, s->o_obs.p, s->o_obs.n}, {o->level_scale, s->o_lscale.p, s->o_lscale.n},
      {o->slope_scale, s->o_sscale.p, s->o_sscale.n},       {o->weights, s->o_w.p, s->o_w.n},
      {o->posterior_means, s->o_pm.p, s->o_pm.n},           {o->seasonal_drift_scales, s->o_drift.p, s->o_drift.n}};
  // From here on copies and kernels that write the caller's buffers are in flight: whatever the
  // way out, both streams are idle before the caller gets its buffers (and the pool its streams) back.
  StreamsIdle idle{s};
  // The tail -- the last chunk's rows and the arrays without a time axis -- is known now, and so is
  // when it is ready: at ev1.  It is queued while the sampler runs, so that nothing is left for the
  // host to submit once the GPU has gone idle.  Arrays the device can write itself (pinned
  // destinations) go through ONE gather kernel behind ev1 on the sampler's stream; the others
  // through copies behind a wait on ev1.
  const int tail_next = (S - 1) / chunk_draws * chunk_draws;      // first draw of the last chunk
  size_t tail_bytes = 0;
  for (const BigPair& b : big) tail_bytes += BC * (size_t)(S - tail_next) * b.row * sizeof(float);
  for (const SmallPair& m : small) tail_bytes += m.dst ? m.n * sizeof(float) : 0;
  bool big_gathered[4] = {false, false, false, false}, small_gathered[6] = {false, false, false, false, false, false};
  ci::TailArgs ta;
  int ng = 0;
  if (tail_bytes <= (size_t)CI_TAIL_GATHER_MAX_BYTES) {
    for (size_t i = 0; i < big.size(); ++i)
      if (float* d = pinned_device_address(big[i].dst)) {
        const size_t off = (size_t)tail_next * big[i].row;
        ta.e[ng++] = {d + off, big[i].src + off, (size_t)(S - tail_next) * big[i].row, (size_t)S * big[i].row,
                      (unsigned int)BC};
        big_gathered[i] = true;
      }
    for (int i = 0; i < 6; ++i)
      if (small[i].dst && small[i].n)
        if (float* d = pinned_device_address(small[i].dst)) {
          ta.e[ng++] = {d, small[i].src, small[i].n, 0, 1u};
          small_gathered[i] = true;
        }
    if (ng) {
      hipLaunchKernelGGL(ci::tail_gather_kernel, dim3(ci::TAIL_BLOCKS, ng), dim3(256), 0, s->stream, ta);
      HIP_TRY(hipGetLastError());
    }
  }
  int next = 0;
  while (next < S) {
    const int target = std::min(S, next + chunk_draws);
    if (live && target == S) {
      // the last chunk: no waiting for its progress value, the copies wait for the kernel's end
      HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev1, 0));
    } else if (live) {
      // wait until every chain has published `target` complete draws
      for (;;) {
        unsigned int lo = 0xFFFFFFFFu;
        volatile unsigned int* pr = s->progress;
        for (size_t i = 0; i < BC; ++i) lo = std::min(lo, (unsigned int)pr[i]);
        if (lo >= (unsigned int)target) break;
        const hipError_t q = hipStreamQuery(s->stream);
        if (q == hipSuccess) break;                 // kernel finished: everything is in HBM
        if (q != hipErrorNotReady) return fail("Gibbs kernel failed: %s", hipGetErrorString(q));
        __builtin_ia32_pause();
      }
    } else if (next == 0) {
      HIP_TRY(hipStreamSynchronize(s->stream));
    }
    for (size_t i = 0; i < big.size(); ++i) {
      if (target == S && big_gathered[i]) continue;
      const BigPair& b = big[i];
      const size_t pitch = (size_t)S * b.row * sizeof(float);
      HIP_TRY(hipMemcpy2DAsync(b.dst + (size_t)next * b.row, pitch, b.src + (size_t)next * b.row, pitch,
                               (size_t)(target - next) * b.row * sizeof(float), BC,
                               hipMemcpyDeviceToHost, s->copy_stream));
    }
    next = target;
  }
  for (int i = 0; i < 6; ++i)
    if (small[i].dst && small[i].n && !small_gathered[i])
      HIP_TRY(hipMemcpyAsync(small[i].dst, small[i].src, small[i].n * sizeof(float), hipMemcpyDeviceToHost,
                             s->copy_stream));
  // ONE wait for the copies (they end after the sampler: gated on ev1, or queued after it had
  // ended); the sampler's stream, with the gather kernel, is then idle or about to be.  A failed
  // kernel is reported from its own stream first.
  const hipError_t copied = hipStreamSynchronize(s->copy_stream);
  const hipError_t sampled = hipStreamSynchronize(s->stream);
  if (sampled != hipSuccess) return fail("Gibbs kernel failed: %s", hipGetErrorString(sampled));
  if (copied != hipSuccess) return fail("copying the results failed: %s", hipGetErrorString(copied));
  idle.s = nullptr;
  if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, s->ev0, s->ev1));
  s->ran = true;
  if (o->slope && !pb.has_slope) memset(o->slope, 0, s->o_level.n * sizeof(float));
  return 0;
}


int ci_session_fetch(ci_session* s, ci_outputs* o) {
  if (!s || !o) return fail("NULL argument");
  if (refuse_draws_session(s, "ci_session_fetch")) return 1;
  HIP_TRY(hipSetDevice(s->pb.device));
  return copy_outputs(o, s->outputs());
}

int ci_session_algorithmic_bytes(const ci_session* s, double* bytes) {
  if (!s || !bytes) return fail("NULL argument");
  if (refuse_draws_session(s, "ci_session_algorithmic_bytes")) return 1;
  const ci_problem& pb = s->pb;
  const double P = pb.P, S = pb.num_results;
  if (s->ragged) {
    // the real steps of every series, not the padding up to the stride
    double steps = 0.0;
    for (int tb : s->lengths) steps += tb;
    const double slope = pb.has_slope ? 1.0 : 0.0, K = pb.num_blocks;
    *bytes = pb.num_chains * (S * (4.0 * steps * (2.0 + slope + K) + pb.num_series * 4.0 * (P + 2.0 + slope + K)) +
                              4.0 * steps * (P + 1.0) + steps);
    return 0;
  }
  const double T = pb.T;
  const double chains = (double)pb.num_series * pb.num_chains;
  // per retained draw 4 T (d_out + 1) + 4 (P + 2 + slope + K), d_out = level
  // + slope + the seasonal latents the fit materialises (one per block: ci_outputs.seasonal_levels);
  // inputs once per chain: 4 T (P + 1) + T.
  const double K = pb.num_blocks;
  const double d_out = 1.0 + (pb.has_slope ? 1.0 : 0.0) + K;
  const double per_draw = 4.0 * T * (d_out + 1.0) + 4.0 * (P + 2.0 + (pb.has_slope ? 1.0 : 0.0) + K);
  const double per_chain = 4.0 * T * (P + 1.0) + T;
  *bytes = chains * (S * per_draw + per_chain);
  return 0;
}

int ci_session_kernel_name(const ci_session* s, char* buf, int32_t buflen) {
  if (!s) return fail("session is NULL");
  if (refuse_draws_session(s, "ci_session_kernel_name")) return 1;
  return copy_name(s->kernel_name, buf, buflen);
}

int ci_session_profile(ci_session* s, int enable, int64_t* cycles16) {
  if (!s) return fail("session is NULL");
  if (refuse_draws_session(s, "ci_session_profile")) return 1;
  if (s->ragged && enable) return fail("ci_session_profile does not take ragged sessions (no instrumented ragged build)");
  s->profile = enable != 0;
  if (cycles16) {
    if (!s->prof.p) { memset(cycles16, 0, 32 * sizeof(int64_t)); return 0; }
    HIP_TRY(hipMemcpy(cycles16, s->prof.p, 32 * sizeof(int64_t), hipMemcpyDeviceToHost));
  }
  return 0;
}

// The buffers free themselves (DevBuf) once the streams they were used on have been parked, that
// is, synchronised.
int ci_session_destroy(ci_session* s) {
  if (!s) return 0;
  (void)hipSetDevice(s->pb.device);
  pool_event_put(s->ev0, s->pb.device);
  pool_event_put(s->ev1, s->pb.device);
  pool_stream_put(s->stream, s->pb.device);
  pool_stream_put(s->copy_stream, s->pb.device);
  if (s->progress) (void)hipHostFree(s->progress);
  delete s;
  return 0;
}

int ci_fit_gibbs(const ci_problem* pb, const float* y, const uint8_t* mask, const float* X,
                 const uint8_t* season_change, const ci_series_params* params, ci_outputs* outputs) {
  if (!outputs) return fail("outputs is NULL");
  ci_session* s = nullptr;
  if (ci_session_create(pb, y, mask, X, season_change, params, &s)) return 1;
  int rc = ci_session_run(s, nullptr);
  if (!rc) rc = ci_session_fetch(s, outputs);
  ci_session_destroy(s);
  return rc;
}

int ci_test_rng(int device, const uint32_t seed[2], uint32_t chain, uint32_t iter, uint32_t site,
                uint32_t sub, int32_t n, float* uniforms, float* normals, double alpha,
                double* gamma_draw) {
  if (n < 1 || n > 256) return fail("n must be in [1, 256]");
  HIP_TRY(hipSetDevice(device));
  DevBuf<float> du, dn;
  DevBuf<double> dg;
  HIP_TRY(du.alloc(n));
  HIP_TRY(dn.alloc(2 * (size_t)n));
  HIP_TRY(dg.alloc(1));
  hipLaunchKernelGGL(ci::test_rng_kernel, dim3(1), dim3(256), 0, 0, seed[0], seed[1], chain, iter,
                     site, sub, n, du.p, dn.p, alpha, dg.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(uniforms, du.p, n * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(normals, dn.p, 2 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(gamma_draw, dg.p, sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}


int ci_test_dk_draw(const ci_problem* pb, const ci_series_params* params, const float* resid,
                    const uint8_t* mask, const uint8_t* season_change, double obs_scale,
                    double level_scale, double slope_scale, const double* drift_scales,
                    uint32_t iter, float* out_latents) {
  (void)season_change; (void)drift_scales;
  if (validate(pb)) return 1;
  const CiInst* inst = ci_inst(pb->has_slope ? 2 : 1, steps_per_thread(pb->T));
  if (!inst) return fail("ci_test_dk_draw: no kernel for T=%d", pb->T);
  HIP_TRY(hipSetDevice(pb->device));
  const int T = pb->T, D = pb->has_slope ? 2 : 1;
  DevBuf<float> dres, dout;
  DevBuf<uint8_t> dmask;
  HIP_TRY(dres.alloc(T));
  HIP_TRY(dmask.alloc(T));
  HIP_TRY(dout.alloc((size_t)T * D));
  HIP_TRY(hipMemcpy(dres.p, resid, T * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dmask.p, mask, T, hipMemcpyHostToDevice));
  const uint32_t chain = (uint32_t)pb->chain_offset;
  const ci_series_params* q = params;
  inst->launch_dk(T, dres.p, dmask.p, (float)(obs_scale * obs_scale), (float)level_scale, (float)slope_scale,
                  (float)q->init_level_loc, (float)(q->init_level_scale * q->init_level_scale),
                  (float)(q->init_slope_scale * q->init_slope_scale), pb->seed[0], pb->seed[1], chain, iter,
                  dout.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out_latents, dout.p, (size_t)T * D * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}


}  // extern "C"
