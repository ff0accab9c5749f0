// ci_fit64.hip -- ci_fit_gibbs_f64: the stand-alone float64 fit (kernels: ci_gibbs64.h, launched by
// ci_seasonal.hip).  Every buffer is float64 and lives for the one call.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ci_session.h"
#include "ci_gibbs64.h"
#include "ci_setup.h"

static thread_local float g_f64_kernel_ms = 0.f;   // duration of the last ci_fit_gibbs_f64 kernel on this thread

// The route of a float64 fit of a validated problem: where its arrays live and which kernel runs.
struct F64Route {
  int dfull, dred, gws, reg_lds;
  ci::Layout64 lay;
};
// LDS first: arrays over time AND the regression block (P <= 32) when both fit, then the arrays
// over time alone; else the HBM workspace for the arrays (regression still in LDS if small).
// Host arithmetic only (ci_fit_gibbs_f64_route answers without a device).
static int f64_route(const ci_problem* pb, F64Route* r) {
  const int T = pb->T, P = pb->P, K = pb->num_blocks, has_slope = pb->has_slope ? 1 : 0;
  int dfull = has_slope ? 2 : 1, dred = dfull;
  for (int k = 0; k < K; ++k) { dfull += pb->num_seasons[k]; dred += pb->num_seasons[k] - 1; }
  if (dfull > 64)
    return fail("seasonal state too wide for one wavefront: %d > 64 (dtype=float64 holds states of at "
                "most 64 components; the float32 Gibbs sampler up to %d)", dfull, ci::MW_MAXD);
  int gws = 0, reg_lds = P <= 32 ? 1 : 0;
  if (ci::make_layout64(T, P, K, dfull, dred, has_slope, 0, reg_lds).total > 150 * 1024) {
    reg_lds = 0;
    if (ci::make_layout64(T, P, K, dfull, dred, has_slope, 0, 0).total > 150 * 1024) {
      gws = 1;
      reg_lds = P <= 32 ? 1 : 0;
    }
  }
  r->dfull = dfull; r->dred = dred; r->gws = gws; r->reg_lds = reg_lds;
  r->lay = ci::make_layout64(T, P, K, dfull, dred, has_slope, gws, reg_lds);
  if (r->lay.total > 160 * 1024) return fail("float64 fit needs %zu bytes of LDS (max 163840)", r->lay.total);
  return 0;
}

extern "C" {

int ci_fit_gibbs_f64_route(const ci_problem* pb, int32_t* global_ws, int32_t* reg_lds,
                           int32_t* trend_kernel, int64_t* lds_bytes) {
  if (validate(pb)) return 1;
  if (!global_ws || !reg_lds || !trend_kernel || !lds_bytes) return fail("NULL argument");
  F64Route r;
  if (f64_route(pb, &r)) return 1;
  *global_ws = r.gws;
  *reg_lds = r.reg_lds;
  *trend_kernel = pb->num_blocks == 0 ? 1 : 0;   // (ci_launch_gibbs64: gibbs64_trend_kernel without blocks)
  *lds_bytes = (int64_t)r.lay.total;
  return 0;
}

int ci_fit_gibbs_f64(const ci_problem* pb, const double* y, const uint8_t* mask, const double* X,
                     const uint8_t* season_change, const ci_series_params* params,
                     ci_outputs_f64* o) {
  if (validate(pb)) return 1;
  if (!y || !mask || !params || !o) return fail("NULL argument");
  if (pb->num_blocks > 0 && !season_change) return fail("season_change is NULL but num_blocks > 0");
  if (pb->P > 0 && !X) return fail("X is NULL but P=%d", pb->P);
  const int T = pb->T, P = pb->P, B = pb->num_series, C = pb->num_chains, S = pb->num_results;
  const int K = pb->num_blocks, has_slope = pb->has_slope ? 1 : 0;
  F64Route route;
  if (f64_route(pb, &route)) return 1;
  const int dfull = route.dfull, dred = route.dred, gws = route.gws, reg_lds = route.reg_lds;
  const ci::Layout64& lay = route.lay;
  const size_t ws_stride = ci::gibbs64_ws_bytes(T, P, K, dfull, dred, has_slope, gws, reg_lds);
  const size_t BT = (size_t)B * T, BCS = (size_t)B * C * S;
  // staged and checked on the host before the first device call
  std::vector<double> yh, n_obs;
  if (stage_outcomes<double>(B, T, nullptr, y, mask, yh, n_obs)) return 1;
  if (check_weights_prior_scale(params, B)) return 1;
  std::vector<double> wps(B), ch((size_t)B * dred * dred);
  std::vector<ci::DevSeriesParams> sph(B);
  std::vector<ci::DevSeasonalParams> ssh(B);
  for (int b = 0; b < B; ++b) {
    wps[b] = params[b].weights_prior_scale;
    sph[b] = dev_series_params(params[b], n_obs[b]);
    ssh[b] = dev_seasonal_params(params[b], false);
    const std::vector<double> cf = prior_chol_reduced_d(pb, params[b], dred, false);
    std::copy(cf.begin(), cf.end(), ch.begin() + (size_t)b * dred * dred);
  }
  HIP_TRY(hipSetDevice(pb->device));
  DevBuf<double> d_y, d_xt, d_xtx, d_om, d_wps, d_chol, o_obs, o_ls, o_ss, o_dr, o_w, o_lev, o_slp, o_sea,
      o_pm, o_tr;
  DevBuf<uint8_t> d_mask, d_sc, d_ws;
  DevBuf<ci::DevSeriesParams> d_sp;
  DevBuf<ci::DevSeasonalParams> d_ssp;
  HIP_TRY(d_y.alloc(BT)); HIP_TRY(d_mask.alloc(BT)); HIP_TRY(d_xt.alloc((size_t)B * P * T));
  HIP_TRY(d_xtx.alloc((size_t)B * P * P)); HIP_TRY(d_om.alloc((size_t)B * P * P));
  HIP_TRY(d_wps.alloc(B)); HIP_TRY(d_sp.alloc(B)); HIP_TRY(d_ssp.alloc(B));
  HIP_TRY(d_chol.alloc((size_t)B * dred * dred)); HIP_TRY(d_sc.alloc((size_t)K * T));
  HIP_TRY(d_ws.alloc((size_t)B * C * ws_stride));
  HIP_TRY(o_obs.alloc(BCS)); HIP_TRY(o_ls.alloc(BCS)); HIP_TRY(o_ss.alloc(BCS));
  HIP_TRY(o_dr.alloc(BCS * K)); HIP_TRY(o_w.alloc(BCS * P)); HIP_TRY(o_lev.alloc(BCS * T));
  HIP_TRY(o_slp.alloc(has_slope ? BCS * T : 0)); HIP_TRY(o_sea.alloc(BCS * T * K));
  HIP_TRY(o_pm.alloc((size_t)B * C * T)); HIP_TRY(o_tr.alloc(BCS * T));
  HIP_TRY(hipMemcpy(d_y.p, yh.data(), BT * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_mask.p, mask, BT, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_wps.p, wps.data(), B * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_sp.p, sph.data(), B * sizeof(ci::DevSeriesParams), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_ssp.p, ssh.data(), B * sizeof(ci::DevSeasonalParams), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_chol.p, ch.data(), ch.size() * sizeof(double), hipMemcpyHostToDevice));
  if (K > 0) HIP_TRY(hipMemcpy(d_sc.p, season_change, (size_t)K * T, hipMemcpyHostToDevice));
  if (P > 0) {
    const std::vector<double> xt = transpose_design<double>(B, T, P, X);
    HIP_TRY(hipMemcpy(d_xt.p, xt.data(), xt.size() * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(ci::setup_regression_kernel<double>, dim3(B * P * P), dim3(64), 0, 0, T, P,
                       d_xt.p, d_mask.p, d_wps.p, d_xtx.p, d_om.p);
    HIP_TRY(hipGetLastError());
  }
  const OutBufs<double> outs{o_obs, o_ls, o_ss, o_w, o_lev, o_slp, o_pm, o_tr, o_dr, o_sea, has_slope != 0};
  ci::G64Args a;
  memset(&a, 0, sizeof(a));
  fill_kargs(a.k, T, P, pb->num_warmup, S, C, B, pb->chain_offset, series_stream_base(*pb), pb->seed);
  fill_kargs_buffers(a.k, (const double*)d_y.p, d_mask.p, (const double*)d_xt.p, d_xtx.p, d_om.p, d_sp.p, outs);
  a.K = K; a.has_slope = has_slope; a.dred = dred;
  for (int k = 0; k < ci::SMAXK; ++k) a.nseas[k] = k < K ? pb->num_seasons[k] : 0;
  a.season_change = d_sc.p; a.ssp = d_ssp.p; a.p1_chol = d_chol.p;
  a.out_drift = o_dr.p; a.out_seasonal = o_sea.p;
  a.ws = d_ws.p; a.ws_stride = ws_stride; a.lat_theta = nullptr; a.lat_S = 1; a.reg_lds = reg_lds;
  // CI_F64_PROF=1 (diagnostic): per-phase shader-clock totals of chain 0's thread 0 on stderr
  DevBuf<long long> d_prof;
  const bool want_prof = getenv("CI_F64_PROF") != nullptr;
  if (want_prof) {
    HIP_TRY(d_prof.alloc(32));
    HIP_TRY(hipMemset(d_prof.p, 0, 32 * sizeof(long long)));
    a.k.prof = d_prof.p;
  }
  {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    (void)hipEventRecord(e0, 0);
    ci_launch_gibbs64(&a, B * C, lay.total, gws, 0);
    (void)hipEventRecord(e1, 0);
    const hipError_t le = hipGetLastError();
    const hipError_t se = hipDeviceSynchronize();
    g_f64_kernel_ms = 0.f;
    if (le == hipSuccess && se == hipSuccess) (void)hipEventElapsedTime(&g_f64_kernel_ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    HIP_TRY(le);
    HIP_TRY(se);
  }
  if (want_prof) {
    long long h[32];
    HIP_TRY(hipMemcpy(h, d_prof.p, sizeof(h), hipMemcpyDeviceToHost));
    const double it = (double)(pb->num_warmup + S);
    fprintf(stderr, "ci_fit_gibbs_f64 phases (cycles per iteration):");
    for (int i = 0; i < 32; ++i) if (h[i]) fprintf(stderr, " [%d] %.0f", i, (double)h[i] / it);
    fprintf(stderr, "\n");
  }
  return copy_outputs(o, outs);
}

int ci_fit_gibbs_f64_kernel_ms(float* kernel_ms) {
  if (!kernel_ms) return fail("NULL argument");
  *kernel_ms = g_f64_kernel_ms;
  return 0;
}


}  // extern "C"
