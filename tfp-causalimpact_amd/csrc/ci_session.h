// ci_session.h -- the two session structs of the C-ABI and the validation / staging helpers their
// units share (ci_stage.hip).  Internal: not installed.
#pragma once
#ifndef CI_SEASONAL_DECL_ONLY
#define CI_SEASONAL_DECL_ONLY      // host units take the argument structs and layouts, not the kernels
#endif
#include <cmath>
#include <string>
#include <vector>

#include "ci_host.h"
#include "ci_inst.h"
#include "ci_kernels.h"
#include "ci_seasonal.h"

using namespace cih;

using KernelFn = void (*)(ci::KArgs);

// Scratch of the on-device summary (ci_summary.h) of a session's resident trajectories.
struct SummScratch {
  DevBuf<double> value, cum, obs, order, draw;
  DevBuf<uint8_t> flags;
  DevBuf<int> ranks;
};

struct ci_session {
  ci_problem pb;
  int L = 0, x_in_lds = 0, pm = 0;
  bool eight_waves = false;    // dispatching to the eight-wave latency kernel (ci_kernels8.h)
  int sched_word = 0;          // $CI_SCHED_WORD, read and validated once at session creation (0: the kernel's default)
  size_t lds_bytes = 0;
  size_t lds_prof = 0;         // LDS of fn_prof: always the four-wave kernel, its own layout
  KernelFn fn = nullptr, fn_prof = nullptr, fn_prof8 = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  DevBuf<float> y, Xt, o_obs, o_lscale, o_sscale, o_w, o_level, o_slope, o_pm, o_traj;
  DevBuf<uint8_t> mask;
  DevBuf<double> xtx, omega, wps;      // wps [B]: ci_series_params.weights_prior_scale
  DevBuf<ci::DevSeriesParams> sp;
  DevBuf<long long> prof;
  bool profile = false;
  // ragged sessions (ci_session_create_ragged, ci_session_create_ragged_seasonal): pb.T is the row
  // stride, series b has lengths[b] steps
  bool ragged = false;
  std::vector<int> lengths;
  std::vector<int> ids;          // the series ids handed to a ragged session (empty: none were)
  DevBuf<int> series_T, series_ids;
  // seasonal models
  int D_full = 0, dred = 0;
  DevBuf<uint8_t> season_change;
  DevBuf<ci::DevSeasonalParams> ssp;
  DevBuf<float> p1_chol, o_drift, o_seasonal;
  // time-parallel seasonal kernel
  bool wide = false;
  bool seasonal_gws = false;           // sequential seasonal kernel with its arrays over time in HBM
  bool mw = false;                     // ... its multi-wavefront build (ci_seasonal_mw.h)
  size_t seasonal_ws_bytes = 0;
  int Lc = 0;
  DevBuf<float> ws;
  int cluster = 1;            // time-parallel seasonal kernel: workgroups per chain
  int dk_lds = 0;             //   its DK workers keep the draw's per-step rows in LDS (clusters of 16)
  bool tp = false;            // general seasonal models / trend + P > MAXP on ci_seasonal_tp.h
  size_t tp_ws_bytes = 0;     //   its per-chain HBM workspace
  DevBuf<int> csync;
  DevBuf<float> cpart, cw;
  DevBuf<double> cv;
  SummScratch summ;          // on-device summarisation (ci_summary.h)
  int link = 0;              // ci_session_set_link: the outcome link of the summaries (ci_link.h)
  // ci_session_summarize_predictions: the B parameter blocks the session was created with, and on
  // the device (first call) [B, 4] initial moments followed by [B] ones (ci_predict.h)
  std::vector<ci_series_params> params;
  DevBuf<double> pred_init;
  bool ran = false;
  // A session MADE FROM DRAWS (ci_session_create_from_draws[_f64], ci_forecast.hip): the inputs and the
  // pooled parameter draws the forecast entries read, no fit -- `ran` is true from the start.  Float32
  // draws lie where a fit leaves them (y, Xt, o_obs, o_lscale, o_sscale, o_drift, o_w); with `f64`
  // the inputs and the draws are float64, in the buffers below, and the float64-input builds of the
  // filters read them.
  bool from_draws = false, f64 = false;
  DevBuf<double> y64, Xt64, d_obs64, d_lscale64, d_sscale64, d_drift64, d_w64;
  ci_problem kpb;          // what the kernel runs (== pb except for long trend-only series)
  bool inert_block = false;
  std::string kernel_name; // the Gibbs kernel this session dispatches to (as rocprofv3 names it)
  // streamed fetch (ci_session_run_streamed)
  hipStream_t copy_stream = nullptr;
  unsigned int* progress = nullptr;   // host-coherent pinned [B * C]
  int progress_every = 0;             // != 0 only while a streamed run is in flight

  OutBufs<float> outputs() const {
    return {o_obs, o_lscale, o_sscale, o_w, o_level, o_slope, o_pm, o_traj, o_drift, o_seasonal,
            pb.has_slope != 0};
  }
};

struct ci_ll_session {
  int T = 0, P = 0, D = 1, L = 1, device = 0, max_evals = 0;
  float a1 = 0, p10 = 0, p11 = 0, p1e = 0;
  const CiInst* inst = nullptr;     // the (D, L) object of the register-resident route (null on the sequential one)
  // seasonal blocks and / or T > 4096: the sequential one-wavefront route (ci_score_seq.h)
  bool seq = false;
  int K = 0, D_full = 1, nseas[CI_MAX_BLOCKS] = {0};
  DevBuf<uint8_t> season_change;
  DevBuf<float> seq_ws;
  size_t seq_ws_evals = 0;          // evaluations seq_ws has room for
  bool wide = false;                // ... on the time-parallel scans (ci_wide_score.h): d <= 8
  const CiWideInst* winst = nullptr;   //     their (TR, NS) object
  int wide_ns = 2, Lc = 0;
  int dred = 1;
  ci_problem spb;                   // the problem (geometry) for the latent pass
  DevBuf<ci::DevSeriesParams> d_sp;
  DevBuf<ci::DevSeasonalParams> d_ssp;
  DevBuf<float> p1_chol, lat_ws, h_seasonal, h_drift, h_loc;
  DevBuf<float> y, xt, level, slope, loc, traj;
  DevBuf<uint8_t> mask;
  DevBuf<double> theta, ll, grad;
  size_t draw_cap = 0;
  // on-device HMC (ci_hmc.h): the fit stays resident until ci_ll_session_hmc_fetch
  DevBuf<double> omega, h_draws, h_acc, h_eps, h_init;
  DevBuf<float> h_level, h_slope, h_part, h_traj, h_pm, h_obs, h_lscale, h_sscale, h_w;
  int h_C = 0, h_S = 0;
  bool h_ran = false;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
  ci_series_params prm;
  // B series (ci_ll_session_create_batch; 1 otherwise): y, mask [B, T], xt [B, P, T], omega [B, P, P]
  // and the fit's outputs with a leading series axis.  Series b draws from the Philox key of series
  // id series_stream_base + b, or from the seed itself when series_stream_base < 0.
  int B = 1, series_stream_base = -1;
  std::vector<ci_series_params> prms;       // [B]
  DevBuf<ci::HmcSeries> h_ser;              // [B]: what hmc_kernel / latents_kernel read per series
  SummScratch summ;                         // ci_ll_session_hmc_summarize

  OutBufs<float> outputs() const {
    return {h_obs, h_lscale, h_sscale, h_w, h_level, h_slope, h_pm, h_traj, h_drift, h_seasonal, D == 2};
  }
};

// The entries that need a fit refuse a session made from draws, before any device call.
inline int refuse_draws_session(const ci_session* s, const char* entry) {
  if (s->from_draws)
    return fail("%s: the session was made from draws (ci_session_create_from_draws) and holds no fit", entry);
  return 0;
}

// ---- ci_stage.hip: what is checked and staged on the host, before any device call ---------------
int validate(const ci_problem* pb);
// Steps per thread of the register-resident kernels (1, 2, 4, 8, 16; 0: the series is too long).
int steps_per_thread(int T);
int wide_steps_per_thread(int T);
// Routes of the time-parallel trend + one-block kernel (ci_wide.h) and of its BIGP build.
bool use_wide(const ci_problem* pb);
bool wide_bigp_ok(const ci_problem* pb);

int check_weights_prior_scale(const ci_series_params* params, int B);
int copy_name(const std::string& name, char* buf, int32_t buflen);

// Lower Cholesky factor of the prior covariance of x_0 in the (n-1)-effect coordinates, row-major [dr, dr].
std::vector<double> prior_chol_reduced_d(const ci_problem* pb, const ci_series_params& q, int dr,
                                         bool inert_blocks);
std::vector<float> prior_chol_reduced(const ci_problem* pb, const ci_series_params& q, int dr,
                                      bool inert_blocks);
ci::DevSeriesParams dev_series_params(const ci_series_params& q, double n_obs);
// `inert`: the block a long trend-only series carries (zero initial variance; its drift scale is
// drawn but never used).
ci::DevSeasonalParams dev_seasonal_params(const ci_series_params& q, bool inert);

// Outcomes of B series of stride T (series b has lengths[b] steps when `lengths` is given: the rows
// behind are padding): yh = y with the masked steps zeroed, n_obs[b] = the unmasked steps, which
// must be finite.
template <class F>
int stage_outcomes(int B, int T, const int32_t* lengths, const F* y, const uint8_t* mask,
                   std::vector<F>& yh, std::vector<double>& n_obs) {
  yh.assign((size_t)B * T, (F)0);
  n_obs.assign(B, 0.0);
  for (int b = 0; b < B; ++b) {
    const int Tb = lengths ? lengths[b] : T;
    for (int t = 0; t < Tb; ++t) {
      const size_t i = (size_t)b * T + t;
      if (mask[i]) continue;
      if (!std::isfinite(y[i])) return fail("y[%d, %d] is not finite but unmasked", b, t);
      yh[i] = y[i];
      n_obs[b] += 1;
    }
  }
  return 0;
}

// The designs [B, T, P] feature-major: [B, P, T].
template <class F> std::vector<F> transpose_design(int B, int T, int P, const F* X) {
  std::vector<F> xt((size_t)B * P * T);
  for (int b = 0; b < B; ++b)
    for (int t = 0; t < T; ++t)
      for (int j = 0; j < P; ++j) xt[((size_t)b * P + j) * T + t] = X[((size_t)b * T + t) * P + j];
  return xt;
}

// The launch geometry and the Philox streams of ci::KArgs / ci::K64.
template <class K>
void fill_kargs(K& k, int T, int P, int W, int S, int C, int B, int chain_offset, int series_stream_base,
                const uint32_t seed[2]) {
  k.T = T; k.P = P; k.W = W; k.S = S; k.C = C; k.B = B; k.chain_offset = chain_offset;
  k.series_stream_base = series_stream_base;
  k.seed0 = seed[0]; k.seed1 = seed[1];
}
inline int series_stream_base(const ci_problem& pb) {
  return (pb.flags & CI_FLAG_SHARED_SERIES_STREAMS) ? -1 : pb.series_offset;
}
// ... its inputs and the result arrays it writes.
template <class K, class F>
void fill_kargs_buffers(K& k, const F* y, const uint8_t* mask, const F* Xt, const double* xtx,
                        const double* omega, const ci::DevSeriesParams* sp, const OutBufs<F>& o) {
  k.y = y; k.mask = mask; k.Xt = Xt; k.xtx = xtx; k.omega = omega; k.sp = sp;
  k.out_obs = o.obs.p; k.out_level_scale = o.lscale.p; k.out_slope_scale = o.sscale.p;
  k.out_weights = o.w.p; k.out_level = o.level.p; k.out_slope = o.slope.p;
  k.out_pred_mean = o.pm.p; k.out_traj = o.traj.p;
  k.prof = nullptr;
}
