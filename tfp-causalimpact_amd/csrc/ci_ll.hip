// ci_ll.hip -- the log-likelihood / HMC session of the C-ABI (ci_ll_session_*, ci_kalman_loglik):
// Kalman log-likelihood and score evaluations, latent draws and the on-device HMC fit, on the
// register-resident kernels (ci_inst.hip), the time-parallel scans (ci_wide.hip) or the sequential
// route (ci_seasonal.hip).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ci_session.h"
#include "ci_hmc.h"
#include "ci_score_seq.h"
#include "ci_wide_score.h"

namespace ci {
// Per-chain mean over the S retained draws of the noise-free predictor (causalimpact_lib.py:627)
// from the per-group sums the latents pass leaves: part [B, C, NG, T] -> pm [B, C, T].  One thread
// per (series, chain, t) -- grid (T / 256, C, B) --, coalesced over t; the order of the sums is
// fixed, so chain c's mean does not depend on how chains or series are split over launches.
static __global__ void hmc_mean_kernel(int C, int NG, int S, int T, const float* __restrict__ part,
                                       float* __restrict__ pm) {
  // part [B, C, NG, T]: sums of the predictor over groups of consecutive draws (latents_kernel)
  const int t = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  if (t >= T || c >= C) return;
  const size_t bc = (size_t)blockIdx.z * C + c;
  const float* p = part + bc * NG * T + t;
  float acc = 0.f;
  for (int g = 0; g < NG; ++g) acc += p[(size_t)g * T];
  pm[bc * T + t] = acc / (float)S;
}

// (sigma_obs, sigma_level, sigma_slope, beta) rows in float64 -> the float32 sample container: N
// rows [B, C, S] of a batched fit flattened.
static __global__ void hmc_unpack_kernel(int N, int P, const double* __restrict__ draws,
                                         float* __restrict__ obs, float* __restrict__ lscale,
                                         float* __restrict__ sscale, float* __restrict__ w) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const double* r = draws + (size_t)n * (3 + P);
  obs[n] = (float)r[0];
  lscale[n] = (float)r[1];
  sscale[n] = (float)r[2];
  for (int j = 0; j < P; ++j) w[(size_t)n * P + j] = (float)r[3 + j];
}

}  // namespace ci

// draws per workgroup in the HMC fit's latent pass (their predictor sums stay in registers)
constexpr int HMC_LATENT_GROUP = 8;

namespace {
// Gaussian slab of the weights prior: Omega = 0.01 (X'X/2 + diag(X'X)/2) / T, all rows
// (causalimpact_lib.py:451-453); X [T, P] row-major.
std::vector<double> slab_omega(const float* X, int T, int P, double weights_prior_scale) {
  std::vector<double> om((size_t)P * P, 0.0);
  for (int t = 0; t < T; ++t)
    for (int i = 0; i < P; ++i)
      for (int j = 0; j < P; ++j)
        om[(size_t)i * P + j] += (double)X[(size_t)t * P + i] * (double)X[(size_t)t * P + j];
  for (int i = 0; i < P; ++i)
    for (int j = 0; j < P; ++j)
      om[(size_t)i * P + j] = 0.01 * (i == j ? om[(size_t)i * P + j] : 0.5 * om[(size_t)i * P + j]) / T *
                              weights_prior_scale;
  return om;
}
}  // namespace

struct LlSessionGuard {
  ci_ll_session* s;
  ~LlSessionGuard() { if (s) ci_ll_session_destroy(s); }
};


extern "C" {


int ci_ll_session_create(const ci_problem* pb, const ci_series_params* params, const float* y,
                         const uint8_t* mask, const float* X, int32_t max_evals,
                         ci_ll_session** out) {
  if (pb && pb->num_blocks != 0)
    return fail("ci_ll_session_create: seasonal blocks need ci_ll_session_create2 (season_change)");
  return ci_ll_session_create2(pb, params, y, mask, X, nullptr, max_evals, out);
}

// What both creators share: the geometry and the first series' initial state, the stream and
// events, and the inputs of B series -- y (masked steps zeroed: yh), mask [B, T], the designs
// feature-major [B, P, T] and their slab precisions [B, P, P] -- with room for max_evals rows of K
// + 3 + P parameters.
static int ll_session_inputs(ci_ll_session* s, const ci_problem* pb, const ci_series_params* params,
                             int32_t max_evals, const std::vector<float>& yh, const uint8_t* mask,
                             const float* X) {
  const int T = pb->T, P = pb->P, B = pb->num_series, K = pb->num_blocks;
  s->T = T; s->P = P; s->D = pb->has_slope ? 2 : 1; s->B = B;
  s->device = pb->device; s->max_evals = max_evals;
  s->prm = params[0];
  s->prms.assign(params, params + B);
  s->a1 = (float)params[0].init_level_loc;
  s->p10 = (float)(params[0].init_level_scale * params[0].init_level_scale);
  s->p11 = (float)(params[0].init_slope_scale * params[0].init_slope_scale);
  HIP_TRY(pool_stream_get(&s->stream));
  HIP_TRY(pool_event_get(&s->ev0));
  HIP_TRY(pool_event_get(&s->ev1));
  HIP_TRY(pool_event_get(&s->ev2));
  HIP_TRY(s->y.alloc((size_t)B * T));
  HIP_TRY(s->mask.alloc((size_t)B * T));
  HIP_TRY(s->xt.alloc((size_t)B * P * T));
  HIP_TRY(s->omega.alloc((size_t)B * P * P));
  HIP_TRY(s->theta.alloc((size_t)max_evals * (3 + K + P)));
  HIP_TRY(s->ll.alloc(max_evals));
  HIP_TRY(s->grad.alloc((size_t)max_evals * (3 + K + P)));
  HIP_TRY(hipMemcpy(s->y.p, yh.data(), yh.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s->mask.p, mask, (size_t)B * T, hipMemcpyHostToDevice));
  if (P == 0) return 0;
  const std::vector<float> xt = transpose_design<float>(B, T, P, X);
  HIP_TRY(hipMemcpy(s->xt.p, xt.data(), xt.size() * sizeof(float), hipMemcpyHostToDevice));
  for (int b = 0; b < B; ++b) {
    const std::vector<double> om = slab_omega(X + (size_t)b * T * P, T, P, params[b].weights_prior_scale);
    HIP_TRY(hipMemcpy(s->omega.p + (size_t)b * P * P, om.data(), om.size() * sizeof(double),
                      hipMemcpyHostToDevice));
  }
  return 0;
}

int ci_ll_session_create2(const ci_problem* pb, const ci_series_params* params, const float* y,
                          const uint8_t* mask, const float* X, const uint8_t* season_change,
                          int32_t max_evals, ci_ll_session** out) {
  if (validate(pb)) return 1;
  if (pb->num_blocks > 0 && !season_change) return fail("season_change is NULL but num_blocks > 0");
  if (pb->P > ci::HMC_MAXP) return fail("log-likelihood path: P must be <= %d, got %d", ci::HMC_MAXP, pb->P);
  if (!params || !y || !mask || !out || max_evals < 1) return fail("bad argument");
  if (check_weights_prior_scale(params, 1)) return 1;
  if (pb->P > 0 && !X) return fail("X is NULL but P=%d", pb->P);
  const bool seq = pb->num_blocks > 0 || steps_per_thread(pb->T) == 0;
  if (seq && pb->P > ci::MAXP)
    return fail("log-likelihood path, seasonal blocks or T > 4096: P must be <= %d, got %d", ci::MAXP, pb->P);
  int dfull = pb->has_slope ? 2 : 1;
  for (int k = 0; k < pb->num_blocks; ++k) dfull += pb->num_seasons[k];
  // trend + one block of 2-7 seasons (or a long trend-only series: an inert 2-season block) run on
  // the time-parallel scans of ci_wide_score.h; everything else sequentially (ci_score_seq.h)
  const bool wide_ll = seq && !(pb->flags & CI_FLAG_SEQUENTIAL_SEASONAL) &&
                       wide_steps_per_thread(pb->T) <= ci::WIDE_MAX_LC &&
                       (pb->num_blocks == 0 ||
                        (pb->num_blocks == 1 && pb->num_seasons[0] >= 2 && pb->num_seasons[0] <= 7));
  if (seq && !wide_ll && dfull > 64)
    return fail("seasonal state too wide for one wavefront: %d > 64 (the log-likelihood and "
                "sampler=\"hmc\" paths hold states of at most 64 components; the Gibbs sampler up to %d)",
                dfull, ci::MW_MAXD);
  std::vector<float> yh;
  std::vector<double> n_obs;
  if (stage_outcomes<float>(1, pb->T, nullptr, y, mask, yh, n_obs)) return 1;
  HIP_TRY(hipSetDevice(pb->device));
  ci_ll_session* s = new ci_ll_session();
  LlSessionGuard guard{s};
  ci_problem one = *pb;            // (a single series, whatever pb->num_series says)
  one.num_series = 1;
  if (ll_session_inputs(s, &one, params, max_evals, yh, mask, X)) return 1;
  const int T = s->T, K = pb->num_blocks;
  s->L = seq ? 0 : steps_per_thread(T);
  s->seq = seq; s->K = K; s->D_full = dfull;
  for (int k = 0; k < K; ++k) s->nseas[k] = pb->num_seasons[k];
  s->p1e = (float)(params->init_seasonal_scale * params->init_seasonal_scale);
  s->wide = wide_ll;
  s->wide_ns = pb->num_blocks == 1 ? pb->num_seasons[0] : 2;
  s->Lc = wide_ll ? wide_steps_per_thread(T) : 0;
  s->inst = seq ? nullptr : ci_inst(s->D, s->L);
  s->winst = wide_ll ? ci_wide_inst(s->D, s->wide_ns) : nullptr;
  if (seq ? (wide_ll && !s->winst) : !s->inst) return fail("no kernel for D=%d, L=%d", s->D, s->L);
  if (seq) {
    const size_t per_eval = wide_ll ? ci::wide_score_ws_floats(s->D + s->wide_ns - 1, s->Lc)
                                    : ci::seq_score_ws_floats(T, dfull);
    HIP_TRY(s->seq_ws.alloc((size_t)max_evals * per_eval));
    s->seq_ws_evals = (size_t)max_evals;
    s->spb = *pb;
    s->dred = dfull - K;
    const ci::DevSeriesParams dsp = dev_series_params(*params, n_obs[0]);
    const ci::DevSeasonalParams dss = dev_seasonal_params(*params, false);
    const std::vector<float> cf = prior_chol_reduced(pb, *params, s->dred, false);
    HIP_TRY(s->d_sp.alloc(1));
    HIP_TRY(s->d_ssp.alloc(1));
    HIP_TRY(s->p1_chol.alloc(cf.size()));
    HIP_TRY(hipMemcpy(s->d_sp.p, &dsp, sizeof(dsp), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->d_ssp.p, &dss, sizeof(dss), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->p1_chol.p, cf.data(), cf.size() * sizeof(float), hipMemcpyHostToDevice));
    if (K > 0) {
      HIP_TRY(s->season_change.alloc((size_t)K * T));
      HIP_TRY(hipMemcpy(s->season_change.p, season_change, (size_t)K * T, hipMemcpyHostToDevice));
    }
  }
  guard.s = nullptr;
  *out = s;
  return 0;
}

int ci_ll_session_create_batch(const ci_problem* pb, const ci_series_params* params, const float* y,
                               const uint8_t* mask, const float* X, int32_t max_evals,
                               ci_ll_session** out) {
  // everything is checked before the first device call
  if (!pb || !params || !y || !mask || !out)
    return fail("ci_ll_session_create_batch: problem, params, y, mask and session must not be NULL");
  const int B = pb->num_series, T = pb->T, P = pb->P;
  if (B < 1) return fail("ci_ll_session_create_batch: num_series must be >= 1, got %d", B);
  if (pb->num_blocks != 0)
    return fail("ci_ll_session_create_batch: seasonal blocks are not supported (trend models only; "
                "fit seasonal models one series at a time with ci_ll_session_create2)");
  if (T > ci::NT * 16)
    return fail("ci_ll_session_create_batch: T must be <= %d, got %d (longer series: one at a time "
                "with ci_ll_session_create2)", ci::NT * 16, T);
  if (P > ci::HMC_MAXP)
    return fail("ci_ll_session_create_batch: P must be <= %d, got %d", ci::HMC_MAXP, P);
  if (validate(pb)) return 1;
  if (max_evals < 1) return fail("ci_ll_session_create_batch: max_evals must be >= 1, got %d", max_evals);
  if (P > 0 && !X) return fail("ci_ll_session_create_batch: X is NULL but P=%d", P);
  if (check_weights_prior_scale(params, B)) return 1;
  std::vector<float> yh;
  std::vector<double> n_obs;
  if (stage_outcomes<float>(B, T, nullptr, y, mask, yh, n_obs)) return 1;
  const CiInst* inst = ci_inst(pb->has_slope ? 2 : 1, steps_per_thread(T));
  if (!inst) return fail("ci_ll_session_create_batch: no kernel for T=%d", T);
  HIP_TRY(hipSetDevice(pb->device));
  ci_ll_session* s = new ci_ll_session();
  LlSessionGuard guard{s};
  if (ll_session_inputs(s, pb, params, max_evals, yh, mask, X)) return 1;
  s->L = steps_per_thread(T);
  s->D_full = s->D;
  s->inst = inst;
  s->series_stream_base = series_stream_base(*pb);
  guard.s = nullptr;
  *out = s;
  return 0;
}

// The HMC fit of a session on the sequential route (seasonal blocks and / or T > 4096): the chain
// (hmc_seq_kernel, one workgroup per chain), then ONE launch of the sequential Gibbs kernel in its
// latents-only mode: a workgroup (one wavefront) per retained draw.
static int hmc_run_sequential(ci_ll_session* s, const ci_hmc_options* o, const double* init_theta,
                              float* kernel_ms) {
  const int P = s->P, C = o->num_chains, S = o->num_results, T = s->T, K = s->K;
  const size_t N = (size_t)C * S;
  const int has_slope = s->D == 2 ? 1 : 0;
  const int nsc = 2 + has_slope + K;
  const int dim = (o->prior == CI_HMC_PRIOR_HORSESHOE ? 3 * P + 2 : P) + nsc;
  if ((size_t)C > s->seq_ws_evals) {
    const size_t per_eval = s->wide ? ci::wide_score_ws_floats(s->D + s->wide_ns - 1, s->Lc)
                                    : ci::seq_score_ws_floats(T, s->D_full);
    HIP_TRY(s->seq_ws.alloc((size_t)C * per_eval));
    s->seq_ws_evals = (size_t)C;
  }
  if (init_theta) {
    if (s->h_init.n != (size_t)C * dim) HIP_TRY(s->h_init.alloc((size_t)C * dim));
    HIP_TRY(hipMemcpyAsync(s->h_init.p, init_theta, (size_t)C * dim * sizeof(double),
                           hipMemcpyHostToDevice, s->stream));
  }
  ci::HmcSeqArgs a;
  a.q.T = T; a.q.P = P; a.q.K = K; a.q.has_slope = has_slope; a.q.E = C;
  for (int k = 0; k < ci::SMAXK; ++k) a.q.nseas[k] = k < K ? s->nseas[k] : 0;
  a.q.y = s->y.p; a.q.mask = s->mask.p; a.q.Xt = s->xt.p; a.q.season_change = s->season_change.p;
  a.q.theta = nullptr; a.q.a1 = s->a1; a.q.p10 = s->p10; a.q.p11 = s->p11; a.q.p1e = s->p1e;
  a.q.out_ll = nullptr; a.q.out_grad = nullptr; a.q.ws = s->seq_ws.p;
  a.C = C; a.W = o->num_warmup; a.S = S; a.n_leap = o->num_leapfrog; a.chain_offset = o->chain_offset;
  a.prior_mode = o->prior; a.seed0 = o->seed[0]; a.seed1 = o->seed[1];
  a.omega = s->omega.p;
  const ci_series_params& q = s->prm;
  {
    int n = 0;
    a.ig_a[n] = q.obs_conc; a.ig_b[n] = q.obs_scale; a.init_log[n++] = std::log(q.obs_scale0);
    a.ig_a[n] = q.level_conc; a.ig_b[n] = q.level_scale; a.init_log[n++] = std::log(std::max(q.level_scale0, 1e-4));
    if (has_slope) {
      a.ig_a[n] = q.slope_conc; a.ig_b[n] = q.slope_scale; a.init_log[n++] = std::log(std::max(q.slope_scale0, 1e-4));
    }
    for (int k = 0; k < K; ++k) {
      a.ig_a[n] = q.drift_conc; a.ig_b[n] = q.drift_scale;
      a.init_log[n++] = std::log(std::max(q.drift_scale0[k], 1e-4));
    }
  }
  a.hs_scale0 = o->horseshoe_scale; a.target_accept = o->target_accept; a.eps0 = o->initial_step_size;
  a.init = init_theta ? s->h_init.p : nullptr;
  a.draws = s->h_draws.p; a.accept_rate = s->h_acc.p; a.step_size = s->h_eps.p;
  HIP_TRY(hipEventRecord(s->ev0, s->stream));
  if (s->wide) {
    ci::HmcWideArgs wa;
    wa.h = a; wa.Lc = s->Lc; wa.ws = s->seq_ws.p;
    s->winst->launch_hmc(&wa, s->stream);
  } else {
    ci_launch_hmc_seq(&a, s->D_full, s->stream);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev1, s->stream));
  // ---- latent path + predictive trajectory of every retained draw
  const ci::SLayout in_lds = ci::make_slayout(T, P, K, s->D_full, s->dred, has_slope, 0);
  const bool gws = in_lds.total > 150 * 1024;
  const ci::SLayout lay = ci::make_slayout(T, P, K, s->D_full, s->dred, has_slope, gws ? 1 : 0);
  if (lay.total > 160 * 1024) return fail("latent pass needs %zu bytes of LDS (max 163840)", lay.total);
  const size_t ws_stride = (lay.t_total + 255) & ~(size_t)255;
  if (gws && s->lat_ws.n < N * (ws_stride / sizeof(float)))
    HIP_TRY(s->lat_ws.alloc(N * (ws_stride / sizeof(float))));
  ci::SArgs sa;
  memset(&sa, 0, sizeof(sa));
  ci::KArgs& k = sa.k;
  // one "chain" per retained draw; the predictor of every draw goes to h_loc (its mean: below)
  fill_kargs(k, T, P, 0, 1, (int)N, 1, o->chain_offset, -1, o->seed);
  fill_kargs_buffers(k, (const float*)s->y.p, s->mask.p, (const float*)s->xt.p, nullptr, nullptr, s->d_sp.p,
                     OutBufs<float>{s->h_obs, s->h_lscale, s->h_sscale, s->h_w, s->h_level, s->h_slope,
                                    s->h_loc, s->h_traj, s->h_drift, s->h_seasonal, has_slope != 0});
  k.progress_every = 1;
  sa.K = K; sa.has_slope = has_slope; sa.dred = s->dred;
  for (int kk = 0; kk < ci::SMAXK; ++kk) sa.nseas[kk] = kk < K ? s->nseas[kk] : 0;
  sa.season_change = s->season_change.p; sa.ssp = s->d_ssp.p; sa.p1_chol = s->p1_chol.p;
  sa.out_drift = s->h_drift.p; sa.out_seasonal = s->h_seasonal.p;
  sa.ws = s->lat_ws.p; sa.Lc = 0; sa.cluster = 1; sa.ws_stride = gws ? ws_stride : 0;
  sa.lat_theta = s->h_draws.p; sa.lat_S = S;
  void* fn = ci_gibbs_seasonal_fn(gws ? 1 : 0);
  HIP_TRY(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lay.total));
  hipLaunchKernelGGL((void (*)(ci::SArgs))fn, dim3((unsigned)N), dim3(64), lay.total, s->stream, sa);
  HIP_TRY(hipGetLastError());
  // per-chain mean of the noise-free predictor over the S draws (hmc_mean_kernel: groups of 1)
  hipLaunchKernelGGL(ci::hmc_mean_kernel, dim3((T + 255) / 256, C), dim3(256), 0, s->stream, C, S, S, T,
                     s->h_loc.p, s->h_pm.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev2, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (kernel_ms) {
    HIP_TRY(hipEventElapsedTime(&kernel_ms[0], s->ev0, s->ev1));
    HIP_TRY(hipEventElapsedTime(&kernel_ms[1], s->ev1, s->ev2));
  }
  s->h_ran = true;
  return 0;
}

int ci_ll_session_hmc_run(ci_ll_session* s, const ci_hmc_options* o, const double* init_theta,
                          float* kernel_ms) {
  if (!s || !o) return fail("NULL argument");
  if (o->num_chains < 1 || o->num_results < 1 || o->num_warmup < 0 || o->num_leapfrog < 1)
    return fail("need num_chains >= 1, num_results >= 1, num_warmup >= 0, num_leapfrog >= 1");
  if (!(o->target_accept > 0.0 && o->target_accept < 1.0) || !(o->initial_step_size > 0.0))
    return fail("need 0 < target_accept < 1 and initial_step_size > 0");
  if (o->prior != CI_HMC_PRIOR_SLAB && o->prior != CI_HMC_PRIOR_HORSESHOE)
    return fail("prior must be CI_HMC_PRIOR_SLAB or CI_HMC_PRIOR_HORSESHOE, got %d", o->prior);
  if (o->prior == CI_HMC_PRIOR_HORSESHOE && !(o->horseshoe_scale > 0.0))
    return fail("horseshoe prior needs horseshoe_scale > 0");
  if (o->num_chains > 65535) return fail("num_chains must be <= 65535, got %d", o->num_chains);
  HIP_TRY(hipSetDevice(s->device));
  // num_chains is per series: B x C chains, every per-chain output with a leading series axis
  const int P = s->P, C = o->num_chains, S = o->num_results, T = s->T, B = s->B;
  const size_t BC = (size_t)B * C, N = BC * S;
  s->h_ran = false;
  if (s->h_C != C || s->h_S != S) {
    s->summ = SummScratch();         // sized for the old shape
    s->h_C = 0; s->h_S = 0;          // an allocation failing below must not leave a stale shape
    HIP_TRY(s->h_draws.alloc(N * (3 + s->K + P)));
    if (s->seq) {
      HIP_TRY(s->h_seasonal.alloc(N * T * s->K));
      HIP_TRY(s->h_drift.alloc(N * s->K));
      HIP_TRY(s->h_loc.alloc(N * T));
    }
    HIP_TRY(s->h_acc.alloc(BC));
    HIP_TRY(s->h_eps.alloc(BC));
    HIP_TRY(s->h_level.alloc(N * T));
    HIP_TRY(s->h_slope.alloc(s->D == 2 ? N * T : 0));
    HIP_TRY(s->h_part.alloc(BC * ((S + HMC_LATENT_GROUP - 1) / HMC_LATENT_GROUP) * T));
    HIP_TRY(s->h_traj.alloc(N * T));
    HIP_TRY(s->h_pm.alloc(BC * T));
    HIP_TRY(s->h_obs.alloc(N));
    HIP_TRY(s->h_lscale.alloc(N));
    HIP_TRY(s->h_sscale.alloc(N));
    HIP_TRY(s->h_w.alloc(N * P));
    s->h_C = C; s->h_S = S;
  }
  if (s->seq) return hmc_run_sequential(s, o, init_theta, kernel_ms);
  const int dim = ci::hmc_dim(P, s->D, o->prior);
  if (init_theta) {
    if (s->h_init.n != BC * dim) HIP_TRY(s->h_init.alloc(BC * dim));
    HIP_TRY(hipMemcpyAsync(s->h_init.p, init_theta, BC * dim * sizeof(double),
                           hipMemcpyHostToDevice, s->stream));
  }
  // the per-series constants (hmc_kernel, latents_kernel)
  std::vector<ci::HmcSeries> ser(B);
  for (int b = 0; b < B; ++b) {
    const ci_series_params& q = s->prms[b];
    ci::HmcSeries& e = ser[b];
    e.ig_a[0] = q.obs_conc; e.ig_b[0] = q.obs_scale;
    e.ig_a[1] = q.level_conc; e.ig_b[1] = q.level_scale;
    e.ig_a[2] = q.slope_conc; e.ig_b[2] = q.slope_scale;
    e.init_log[0] = std::log(q.obs_scale0);
    e.init_log[1] = std::log(std::max(q.level_scale0, 1e-4));
    e.init_log[2] = std::log(std::max(q.slope_scale0, 1e-4));
    e.hs_scale0 = o->horseshoe_scale;
    e.a1 = (float)q.init_level_loc;
    e.p10 = (float)(q.init_level_scale * q.init_level_scale);
    e.p11 = (float)(q.init_slope_scale * q.init_slope_scale);
    e.pad = 0.f;
  }
  if (s->h_ser.n != (size_t)B) HIP_TRY(s->h_ser.alloc(B));
  HIP_TRY(hipMemcpy(s->h_ser.p, ser.data(), B * sizeof(ci::HmcSeries), hipMemcpyHostToDevice));
  ci::HmcArgs a;
  a.init = init_theta ? s->h_init.p : nullptr;
  {
    // tests only: the five-barrier driver of rounds 2-4, to compare bits with the fused one
    const char* e_ = getenv("CI_HMC_LEGACY_DRIVER");
    a.legacy_driver = (e_ && e_[0] == '1' && e_[1] == 0) ? 1 : 0;
  }
  // tools/exp_hmc_phases.py: phase cycles of chain 0 (s_memtime on its thread 0), printed to stderr
  DevBuf<long long> hprof;
  a.prof = nullptr;
  if (getenv("CI_HMC_PROF") != nullptr) {
    HIP_TRY(hprof.alloc(32));
    HIP_TRY(hipMemsetAsync(hprof.p, 0, 32 * sizeof(long long), s->stream));
    a.prof = hprof.p;
  }
  a.T = T; a.P = P; a.B = B; a.C = C; a.W = o->num_warmup; a.S = S; a.n_leap = o->num_leapfrog;
  a.chain_offset = o->chain_offset; a.seed0 = o->seed[0]; a.seed1 = o->seed[1];
  a.series_stream_base = s->series_stream_base;
  a.prior_mode = o->prior;
  a.y = s->y.p; a.mask = s->mask.p; a.Xt = s->xt.p; a.omega = s->omega.p; a.ser = s->h_ser.p;
  a.target_accept = o->target_accept; a.eps0 = o->initial_step_size;
  a.draws = s->h_draws.p; a.accept_rate = s->h_acc.p; a.step_size = s->h_eps.p;
  HIP_TRY(hipEventRecord(s->ev0, s->stream));
  s->inst->launch_hmc(&a, s->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev1, s->stream));
  // latent path + posterior-predictive trajectory of every retained draw (one workgroup per
  // draw: C*S workgroups fill the chip), the per-chain predictor means and the float32 container
  s->inst->launch_latents(T, P, (int)N, s->y.p, s->mask.p, s->xt.p, s->h_draws.p, s->a1, s->p10, s->p11,
                          o->seed[0], o->seed[1], (uint32_t)o->chain_offset, 0u, S, HMC_LATENT_GROUP, C,
                          s->series_stream_base, s->h_ser.p, s->h_level.p, s->h_slope.p, nullptr,
                          s->h_traj.p, s->h_part.p, s->stream);
  hipLaunchKernelGGL(ci::hmc_mean_kernel, dim3((T + 255) / 256, C, B), dim3(256), 0, s->stream, C,
                     (S + HMC_LATENT_GROUP - 1) / HMC_LATENT_GROUP, S, T, s->h_part.p, s->h_pm.p);
  hipLaunchKernelGGL(ci::hmc_unpack_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream,
                     (int)N, P, s->h_draws.p, s->h_obs.p, s->h_lscale.p, s->h_sscale.p, s->h_w.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev2, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (kernel_ms) {
    HIP_TRY(hipEventElapsedTime(&kernel_ms[0], s->ev0, s->ev1));
    HIP_TRY(hipEventElapsedTime(&kernel_ms[1], s->ev1, s->ev2));
  }
  if (a.prof) {
    long long h[32];
    HIP_TRY(hipMemcpy(h, hprof.p, sizeof(h), hipMemcpyDeviceToHost));
    std::fprintf(stderr, "ci hmc prof:");
    for (int i = 0; i < 32; ++i) std::fprintf(stderr, " %lld", h[i]);
    std::fprintf(stderr, "\n");
  }
  s->h_ran = true;
  return 0;
}

int ci_ll_session_hmc_fetch(ci_ll_session* s, double* draws, double* accept_rate, double* step_size,
                            ci_outputs* o) {
  if (!s) return fail("session is NULL");
  if (!s->h_ran) return fail("ci_ll_session_hmc_fetch needs a finished ci_ll_session_hmc_run");
  HIP_TRY(hipSetDevice(s->device));
  if (draws) HIP_TRY(hipMemcpy(draws, s->h_draws.p, s->h_draws.n * sizeof(double), hipMemcpyDeviceToHost));
  if (accept_rate) HIP_TRY(hipMemcpy(accept_rate, s->h_acc.p, s->h_acc.n * sizeof(double), hipMemcpyDeviceToHost));
  if (step_size) HIP_TRY(hipMemcpy(step_size, s->h_eps.p, s->h_eps.n * sizeof(double), hipMemcpyDeviceToHost));
  if (o) return copy_outputs(o, s->outputs());
  return 0;
}

int ci_ll_session_kernel_name(const ci_ll_session* s, char* buf, int32_t buflen) {
  if (!s) return fail("session is NULL");
  char nm[64];
  if (s->wide) snprintf(nm, sizeof(nm), "ci::hmc_wide_kernel<%d,%d>", s->D, s->wide_ns);
  else if (s->seq) snprintf(nm, sizeof(nm), "ci::hmc_seq_kernel");
  else if (s->P > ci::MAXP) snprintf(nm, sizeof(nm), "ci::hmc_kernel<%d,%d,wide>", s->D, s->L);
  else snprintf(nm, sizeof(nm), "ci::hmc_kernel<%d,%d>", s->D, s->L);
  return copy_name(nm, buf, buflen);
}

int ci_ll_session_algorithmic_bytes(const ci_ll_session* s, double* bytes) {
  if (!s || !bytes) return fail("NULL argument");
  if (s->h_C < 1) return fail("no HMC fit has been configured on this session");
  // latent / trajectory draws are produced for every HMC draw, so
  // the per-draw figure is the Gibbs one: 4 T (d_out + 1) + 4 (P + 2 + slope); inputs once per chain.
  const double T = s->T, P = s->P, slope = s->D == 2 ? 1.0 : 0.0, K = s->K;
  const double per_draw = 4.0 * T * (1.0 + slope + K + 1.0) + 4.0 * (P + 2.0 + slope + K);
  const double per_chain = 4.0 * T * (P + 1.0) + T;
  *bytes = (double)s->B * s->h_C * ((double)s->h_S * per_draw + per_chain);
  return 0;
}

int ci_ll_session_eval(ci_ll_session* s, int32_t num_evals, const double* theta, double* loglik,
                       double* grad) {
  if (!s || !theta || !loglik) return fail("NULL argument");
  if (s->B > 1) return fail("ci_ll_session_eval: one series per session only (this session holds %d)", s->B);
  if (num_evals < 1 || num_evals > s->max_evals) return fail("num_evals out of range");
  HIP_TRY(hipSetDevice(s->device));
  const int T = s->T, P = s->P, D = s->D, E = num_evals;
  const int dimt = 3 + s->K + P;
  HIP_TRY(hipMemcpy(s->theta.p, theta, (size_t)E * dimt * sizeof(double), hipMemcpyHostToDevice));
  if (s->seq) {
    ci::SeqScoreArgs qa;
    qa.T = T; qa.P = P; qa.K = s->K; qa.has_slope = D == 2 ? 1 : 0; qa.E = E;
    for (int k = 0; k < ci::SMAXK; ++k) qa.nseas[k] = k < s->K ? s->nseas[k] : 0;
    qa.y = s->y.p; qa.mask = s->mask.p; qa.Xt = s->xt.p; qa.season_change = s->season_change.p;
    qa.theta = s->theta.p; qa.a1 = s->a1; qa.p10 = s->p10; qa.p11 = s->p11; qa.p1e = s->p1e;
    qa.out_ll = s->ll.p; qa.out_grad = grad ? s->grad.p : nullptr; qa.ws = s->seq_ws.p;
    if (s->wide) {
      ci::WideScoreArgs wa;
      wa.q = qa; wa.Lc = s->Lc; wa.ws = s->seq_ws.p;
      s->winst->launch_score(&wa, 0);
    } else {
      ci_launch_seq_score(&qa, s->D_full, 0);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(loglik, s->ll.p, E * sizeof(double), hipMemcpyDeviceToHost));
    if (grad) HIP_TRY(hipMemcpy(grad, s->grad.p, (size_t)E * dimt * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
  }
  if (grad)
    s->inst->launch_llgrad(T, P, E, s->y.p, s->mask.p, s->xt.p, s->theta.p, s->a1, s->p10, s->p11, s->ll.p,
                           s->grad.p, 0);
  else
    s->inst->launch_loglik(T, P, E, s->y.p, s->mask.p, s->xt.p, s->theta.p, s->a1, s->p10, s->p11, s->ll.p, 0);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(loglik, s->ll.p, E * sizeof(double), hipMemcpyDeviceToHost));
  if (grad)
    HIP_TRY(hipMemcpy(grad, s->grad.p, (size_t)E * (3 + P) * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int ci_ll_session_draw_latents(ci_ll_session* s, int32_t num_draws, const double* theta,
                               const uint32_t seed[2], uint32_t rng_chain, uint32_t iter0,
                               float* level, float* slope, float* loc, float* traj) {
  if (!s || !theta || !seed || !level || !loc || !traj) return fail("NULL argument");
  if (s->seq) return fail("ci_ll_session_draw_latents: trend models with T <= 4096 only");
  if (s->B > 1)
    return fail("ci_ll_session_draw_latents: one series per session only (this session holds %d)", s->B);
  if (num_draws < 1 || num_draws > s->max_evals) return fail("num_draws out of range");
  HIP_TRY(hipSetDevice(s->device));
  const int T = s->T, P = s->P, D = s->D, E = num_draws;
  const size_t need = (size_t)E * T;
  if (need > s->draw_cap) {
    HIP_TRY(s->level.alloc(need)); HIP_TRY(s->slope.alloc(need));
    HIP_TRY(s->loc.alloc(need)); HIP_TRY(s->traj.alloc(need));
    s->draw_cap = need;
  }
  HIP_TRY(hipMemcpy(s->theta.p, theta, (size_t)E * (3 + P) * sizeof(double), hipMemcpyHostToDevice));
  s->inst->launch_latents(T, P, E, s->y.p, s->mask.p, s->xt.p, s->theta.p, s->a1, s->p10, s->p11, seed[0],
                          seed[1], rng_chain, iter0, 0, 1, 0, -1, nullptr, s->level.p, s->slope.p, s->loc.p,
                          s->traj.p, nullptr, 0);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(level, s->level.p, need * sizeof(float), hipMemcpyDeviceToHost));
  if (slope) {
    if (D == 2) HIP_TRY(hipMemcpy(slope, s->slope.p, need * sizeof(float), hipMemcpyDeviceToHost));
    else memset(slope, 0, need * sizeof(float));
  }
  HIP_TRY(hipMemcpy(loc, s->loc.p, need * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(traj, s->traj.p, need * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// The buffers free themselves (DevBuf) once the stream they were used on has been parked, that is,
// synchronised.
int ci_ll_session_destroy(ci_ll_session* s) {
  if (!s) return 0;
  (void)hipSetDevice(s->device);
  pool_event_put(s->ev0, s->device);
  pool_event_put(s->ev1, s->device);
  pool_event_put(s->ev2, s->device);
  pool_stream_put(s->stream, s->device);
  delete s;
  return 0;
}

int ci_kalman_loglik(const ci_problem* pb, const ci_series_params* params, const float* y,
                     const uint8_t* mask, const float* X, int32_t num_evals, const double* theta,
                     double* loglik) {
  ci_ll_session* s = nullptr;
  if (ci_ll_session_create(pb, params, y, mask, X, num_evals, &s)) return 1;
  const int rc = ci_ll_session_eval(s, num_evals, theta, loglik, nullptr);
  ci_ll_session_destroy(s);
  return rc;
}

}  // extern "C"
