// ci_summary.hip -- the on-device summaries of trajectories behind the C-ABI (kernels: ci_summary.h,
// ci_components.h): ci_session_summarize, ci_session_summarize_components,
// ci_session_summarize_windows, ci_ll_session_summarize_windows
// (kernel: ci_windows.h), ci_session_summarize_paths, ci_ll_session_summarize_paths (kernels: ci_paths.h),
// ci_session_set_link and ci_session_value_mean (the outcome link: ci_link.h),
// ci_ll_session_hmc_summarize on the trajectories a session holds, ci_summarize_draws[_f64] and
// ci_summarize_draw_paths_f64 on draws the caller hands in; ci_session_pool_trajectories, ci_ll_session_pool_trajectories and
// ci_session_pool_event_trajectories (kernels: ci_pool.h) on the trajectories a session holds.
// The Kalman-filter entries (prediction errors, placebo forecasts) are ci_forecast.hip's; the helpers
// it takes from here -- and with launch_select the select kernels, instantiated in this unit alone --
// are declared in ci_summary_host.h.
#include <cmath>
#include <vector>

#include "ci_session.h"
#include "ci_components.h"
#include "ci_paths.h"
#include "ci_pool.h"
#include "ci_summary.h"
#include "ci_summary_host.h"
#include "ci_windows.h"

int check_ranks(int32_t num_ranks, const int32_t* ranks, int N) {
  if (num_ranks < 1 || num_ranks > ci::SUMM_MAX_RANKS)
    return fail("num_ranks must be in [1, %d], got %d", ci::SUMM_MAX_RANKS, num_ranks);
  for (int r = 0; r < num_ranks; ++r)
    if (ranks[r] < 0 || ranks[r] >= N) return fail("rank %d out of range [0, %d)", ranks[r], N);
  return 0;
}

// Order statistics of the rows of two [rows, N] matrices in one launch (M1 may be NULL: one
// matrix); out[(row / T) * R + r][row % T].  Rows of up to 16384 values (every fit_causalimpact
// shape: N = chains x draws) are selected from registers; longer rows by the L2 digit sweeps of
// summ_select_kernel.
#ifndef CI_SEL_NT
#define CI_SEL_NT 256
#endif
hipError_t launch_select(hipStream_t stream, int N, int T, int rows, int R, const int* d_ranks,
                         const double* M0, const double* M1, double* out0, double* out1) {
  const int grid = M1 ? 2 * rows : rows;
  if (N <= 8192) {
    hipLaunchKernelGGL((ci::summ_select_reg_kernel<CI_SEL_NT, 8192 / CI_SEL_NT>), dim3(grid),
                       dim3(CI_SEL_NT), 0, stream, N, T, R, rows, d_ranks, M0, M1, out0, out1);
  } else if (N <= 16384) {
    hipLaunchKernelGGL((ci::summ_select_reg_kernel<512, 32>), dim3(grid), dim3(512), 0, stream,
                       N, T, R, rows, d_ranks, M0, M1, out0, out1);
  } else {
    hipLaunchKernelGGL(ci::summ_select_kernel, dim3(rows), dim3(256), 0, stream, N, T, R, d_ranks,
                       M0, out0);
    if (M1)
      hipLaunchKernelGGL(ci::summ_select_kernel, dim3(rows), dim3(256), 0, stream, N, T, R, d_ranks,
                         M1, out1);
  }
  return hipGetLastError();
}

// The scratch of a summary of B series of N draws over T steps: allocated on first use and kept
// (ci_session_summarize and ci_session_summarize_components share it).
int summ_scratch_alloc(SummScratch& w, int B, int T, int N) {
  if (w.value.p) return 0;
  const size_t BTN = (size_t)B * T * N;
  HIP_TRY(w.value.alloc(BTN));
  HIP_TRY(w.cum.alloc(BTN));
  HIP_TRY(w.obs.alloc((size_t)B * T + 2 * B));
  HIP_TRY(w.flags.alloc((size_t)B * T));
  HIP_TRY(w.ranks.alloc(ci::SUMM_MAX_RANKS));
  HIP_TRY(w.order.alloc((size_t)2 * B * ci::SUMM_MAX_RANKS * T));
  HIP_TRY(w.draw.alloc((size_t)B * 2 * N + (size_t)B * 2 * ci::SUMM_MAX_RANKS));
  return 0;
}

// The transpose of one link (ci_link.h) of B series' [B, N, T] trajectories into value [B, T, N].
template <class TIn>
static void launch_transpose(hipStream_t stream, int link, int B, int T, int N, const TIn* traj,
                             const double* d_scale, const double* d_shift, double* value) {
  const dim3 grid((T + 63) / 64, (N + 63) / 64, B), block(64, 4);
  if (link == ci::LINK_LOG)
    hipLaunchKernelGGL((ci::summ_transpose_kernel<TIn, ci::LINK_LOG>), grid, block, 0, stream, N, T, traj,
                       d_scale, d_shift, value);
  else if (link == ci::LINK_LOG1P)
    hipLaunchKernelGGL((ci::summ_transpose_kernel<TIn, ci::LINK_LOG1P>), grid, block, 0, stream, N, T, traj,
                       d_scale, d_shift, value);
  else
    hipLaunchKernelGGL((ci::summ_transpose_kernel<TIn, ci::LINK_IDENTITY>), grid, block, 0, stream, N, T, traj,
                       d_scale, d_shift, value);
}

// The summary of B series' [B, N, T] trajectories resident in HBM (ci_session_summarize,
// ci_ll_session_hmc_summarize; ci_summarize_draws after its upload): transpose with value = trajectory * scale + shift, running sums,
// order statistics; the scratch is allocated on first use and kept.  Nothing in the scratch outlives
// a call, so a change of the link between two calls finds nothing stale.
template <class TIn>
static int summarize_resident(hipStream_t stream, SummScratch& w, int link, int B, int T, int N, const TIn* traj,
                              const double* scale, const double* shift, const double* observed,
                              const uint8_t* flags, int32_t num_ranks, const int32_t* ranks,
                              double* value_order, double* cum_order, double* per_draw,
                              double* per_draw_order) {
  if (check_ranks(num_ranks, ranks, N)) return 1;
  if (summ_scratch_alloc(w, B, T, N)) return 1;
  double* d_scale = w.obs.p + (size_t)B * T;
  double* d_shift = d_scale + B;
  HIP_TRY(hipMemcpyAsync(w.obs.p, observed, (size_t)B * T * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_scale, scale, B * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_shift, shift, B * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(w.flags.p, flags, (size_t)B * T, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(w.ranks.p, ranks, num_ranks * sizeof(int), hipMemcpyHostToDevice, stream));
  launch_transpose<TIn>(stream, link, B, T, N, traj, d_scale, d_shift, w.value.p);
  hipLaunchKernelGGL(ci::summ_cumsum_kernel, dim3((N + 63) / 64, B), dim3(64), 0, stream, N, T,
                     w.value.p, w.obs.p, w.flags.p, w.cum.p, w.draw.p);
  double* ord_value = w.order.p;
  double* ord_cum = w.order.p + (size_t)B * ci::SUMM_MAX_RANKS * T;
  HIP_TRY(launch_select(stream, N, T, B * T, num_ranks, w.ranks.p, w.value.p, w.cum.p,
                        ord_value, ord_cum));
  double* ord_draw = w.draw.p + (size_t)B * 2 * N;
  if (per_draw_order)
    HIP_TRY(launch_select(stream, N, 1, 2 * B, num_ranks, w.ranks.p, w.draw.p, nullptr,
                          ord_draw, nullptr));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(stream));
  const size_t ord_bytes = (size_t)B * num_ranks * T * sizeof(double);
  if (value_order) HIP_TRY(hipMemcpy(value_order, ord_value, ord_bytes, hipMemcpyDeviceToHost));
  if (cum_order) HIP_TRY(hipMemcpy(cum_order, ord_cum, ord_bytes, hipMemcpyDeviceToHost));
  if (per_draw)
    HIP_TRY(hipMemcpy(per_draw, w.draw.p, (size_t)B * 2 * N * sizeof(double), hipMemcpyDeviceToHost));
  if (per_draw_order)
    HIP_TRY(hipMemcpy(per_draw_order, ord_draw, (size_t)B * 2 * num_ranks * sizeof(double),
                      hipMemcpyDeviceToHost));
  return 0;
}

// The window tables of ci_session_summarize_windows and ci_session_summarize_paths: first, count
// [B, W] inside the session's T steps, the error naming the offending window.  unit, whose: what the
// B rows are called and whose steps they are (ci_summarize_draw_paths_f64: groups of draws).
static int check_window_table(const char* what, int B, int T, int32_t W, int max_windows,
                              const int32_t* first, const int32_t* count, const char* unit = "series",
                              const char* whose = "the session's") {
  if (W < 1 || W > max_windows)
    return fail("%s: num_windows must be in [1, %d], got %d", what, max_windows, W);
  for (int b = 0; b < B; ++b)
    for (int w = 0; w < W; ++w) {
      const int f = first[(size_t)b * W + w], c = count[(size_t)b * W + w];
      if (f < 0) return fail("%s: window %d of %s %d: first step %d is negative", what, w, unit, b, f);
      if (c < 0) return fail("%s: window %d of %s %d: count %d is negative", what, w, unit, b, c);
      if ((long long)f + c > T)
        return fail("%s: window %d of %s %d: steps %d .. %lld end beyond %s %d steps",
                    what, w, unit, b, f, (long long)f + c - 1, whose, T);
    }
  return 0;
}

// The window totals of B series' [B, N, T] float32 trajectories resident in HBM
// (ci_session_summarize_windows, ci_ll_session_summarize_windows): everything is checked before the
// first device call; one streaming pass over the windows' own columns, then the order statistics of
// the 2 * B * W rows of totals.  The call's device memory -- the tables and 2 * (N + 8) doubles per
// (series, window) -- is its own and goes back on every return path; the summary's scratch is
// neither built nor touched.
static int windows_resident(const char* what, int device, hipStream_t stream, int link, int B, int T, int N,
                            const float* traj, const double* scale, const double* shift,
                            const double* observed, int32_t W, const int32_t* first,
                            const int32_t* count, int32_t num_ranks, const int32_t* ranks,
                            double* per_draw, double* per_draw_order) {
  if (check_window_table(what, B, T, W, 1024, first, count)) return 1;
  if (check_ranks(num_ranks, ranks, N)) return 1;
  HIP_TRY(hipSetDevice(device));
  const int R = ci::SUMM_MAX_RANKS;
  const size_t BW = (size_t)B * W, BT = (size_t)B * T;
  DevBuf<double> d_f64;       // observed [B, T], scale [B], shift [B], totals [B, W, 2, N], order [B, W, 2, 8]
  DevBuf<int> d_i32;          // first [B, W], count [B, W], ranks [8]
  HIP_TRY(d_f64.alloc(BT + 2 * (size_t)B + 2 * BW * ((size_t)N + R)));
  HIP_TRY(d_i32.alloc(2 * BW + R));
  double* d_scale = d_f64.p + BT;
  double* d_shift = d_scale + B;
  double* d_draw = d_shift + B;
  double* d_order = d_draw + 2 * BW * N;
  int* d_count = d_i32.p + BW;
  int* d_ranks = d_count + BW;
  HIP_TRY(hipMemcpyAsync(d_f64.p, observed, BT * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_scale, scale, B * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_shift, shift, B * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_i32.p, first, BW * sizeof(int), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_count, count, BW * sizeof(int), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_ranks, ranks, num_ranks * sizeof(int), hipMemcpyHostToDevice, stream));
  HIP_TRY(ci::windows_launch(stream, link, B, N, T, W, traj, d_f64.p, d_scale, d_shift, d_i32.p, d_count,
                             d_draw));
  if (per_draw_order)
    HIP_TRY(launch_select(stream, N, 1, (int)(2 * BW), num_ranks, d_ranks, d_draw, nullptr, d_order,
                          nullptr));
  if (per_draw)
    HIP_TRY(hipMemcpyAsync(per_draw, d_draw, 2 * BW * N * sizeof(double), hipMemcpyDeviceToHost, stream));
  if (per_draw_order)
    HIP_TRY(hipMemcpyAsync(per_draw_order, d_order, 2 * BW * num_ranks * sizeof(double),
                           hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return 0;
}

// The path excursions of B series' [B, N, T] float32 trajectories resident in HBM
// (ci_session_summarize_paths, ci_ll_session_summarize_paths; kernels: ci_paths.h): everything is
// checked before the first device call.  The (series, window) pairs are computed alone, so they are
// taken in chunks of consecutive pairs whose device memory -- the tables, and per pair of `count`
// steps the doubles paths_pair_doubles counts -- stays within max_bytes; the results cannot depend on
// the chunking.  All of it is the call's own and goes back on every return path; the summary's
// scratch is neither built nor touched.  num_chunks (may be NULL): how many chunks it took.
// host_draws != NULL (ci_summarize_draw_paths_f64; traj is then NULL): the B rows are groups of float64
// draws [B, N, T] on the host.  The draws of the groups a chunk's pairs belong to are uploaded for
// that chunk and count N * T doubles each against max_bytes, so a chunk may end inside a group (whose
// draws the next chunk uploads again); a pair is still computed alone.
static size_t paths_pair_doubles(int N, int count) {
  // X [count, 2, N], moments [count, 4], excursion [2, N], order [2, 8], observed_excursion [2],
  // at and exceed [2] int32 each
  return (size_t)count * (2 * (size_t)N + 4) + 2 * (size_t)N + 2 * ci::SUMM_MAX_RANKS + 2 + 2;
}

static int paths_resident(const char* what, int device, hipStream_t stream, int link, int B, int T, int N,
                          const float* traj, const double* scale, const double* shift,
                          const double* observed, int32_t W, const int32_t* first, const int32_t* count,
                          int32_t num_ranks, const int32_t* ranks, double* center, double* spread,
                          double* excursion, double* excursion_order, double* observed_excursion,
                          int32_t* at, int32_t* exceed, int64_t max_bytes, int32_t* num_chunks,
                          const double* host_draws = nullptr) {
  const char* unit = host_draws ? "group" : "series";
  if (check_window_table(what, B, T, W, 64, first, count, unit, host_draws ? "the draws'" : "the session's"))
    return 1;
  if (check_ranks(num_ranks, ranks, N)) return 1;
  const int R = ci::SUMM_MAX_RANKS;
  const size_t group_doubles = host_draws ? (size_t)N * T : 0;      // the uploaded draws of one group
  const size_t BW = (size_t)B * W, BT = (size_t)B * T;
  const size_t table_bytes = (BT + 2 * (size_t)B) * sizeof(double) + 2 * BW * sizeof(int) +
                             (BW + 1) * sizeof(long long) + R * sizeof(int);
  if (max_bytes < 0 || (size_t)max_bytes < table_bytes)
    return fail("%s: the tables alone take %zu bytes of device memory, the limit is %lld", what,
                table_bytes, (long long)max_bytes);
  const size_t budget = ((size_t)max_bytes - table_bytes) / sizeof(double);
  // chunks of consecutive pairs: [starts[i], starts[i + 1])
  std::vector<long long> steps_before(BW + 1, 0);
  std::vector<size_t> starts(1, 0);
  size_t used = 0, most_steps = 0, most_pairs = 0, most_groups = 0;
  for (size_t p = 0; p < BW; ++p) {
    steps_before[p + 1] = steps_before[p] + count[p];
    size_t need = paths_pair_doubles(N, count[p]);
    if (need + group_doubles > budget)
      return fail("%s: window %d of %s %d: its %d steps of %d draws%s take %zu bytes of device memory "
                  "beside %zu of tables, the limit is %lld", what, (int)(p % W), unit, (int)(p / W), count[p],
                  N, host_draws ? " and the group's own draws" : "", (need + group_doubles) * sizeof(double),
                  table_bytes, (long long)max_bytes);
    if (p > 0 && p / W != (p - 1) / W) need += group_doubles;       // (the first pair of its group in this chunk)
    if (used + need > budget || p - starts.back() == 65535) {
      starts.push_back(p);
      used = 0;
      need = paths_pair_doubles(N, count[p]);
    }
    if (used == 0) need += group_doubles;                            // (the first pair of a chunk)
    used += need;
    const size_t groups = p / W - starts.back() / W + 1;
    most_groups = groups > most_groups ? groups : most_groups;
    const size_t steps = (size_t)(steps_before[p + 1] - steps_before[starts.back()]);
    most_steps = steps > most_steps ? steps : most_steps;
    most_pairs = p + 1 - starts.back() > most_pairs ? p + 1 - starts.back() : most_pairs;
  }
  starts.push_back(BW);
  if (num_chunks) *num_chunks = (int32_t)(starts.size() - 1);
  HIP_TRY(hipSetDevice(device));
  DevBuf<double> d_f64, d_X;  // observed [B, T], scale, shift [B]; per chunk: moments, excursion, order, observed_excursion
  DevBuf<int> d_i32;          // first, count [B, W], ranks [8]; per chunk: at, exceed [pairs, 2]
  DevBuf<long long> d_steps;
  DevBuf<double> d_draws;     // (host_draws) per chunk: the draws of its groups [groups, N, T]
  if (host_draws) HIP_TRY(d_draws.alloc(most_groups * group_doubles));
  HIP_TRY(d_f64.alloc(BT + 2 * (size_t)B + most_steps * 4 + most_pairs * 2 * ((size_t)N + R + 1)));
  HIP_TRY(d_X.alloc(most_steps * 2 * N + 1));
  HIP_TRY(d_i32.alloc(2 * BW + R + 4 * most_pairs));
  HIP_TRY(d_steps.alloc(BW + 1));
  double* d_scale = d_f64.p + BT;
  double* d_shift = d_scale + B;
  double* d_mom = d_shift + B;
  double* d_exc = d_mom + most_steps * 4;
  double* d_order = d_exc + most_pairs * 2 * N;
  double* d_obsexc = d_order + most_pairs * 2 * R;
  int* d_count = d_i32.p + BW;
  int* d_ranks = d_count + BW;
  int* d_at = d_ranks + R;
  int* d_exceed = d_at + 2 * most_pairs;
  HIP_TRY(hipMemcpyAsync(d_f64.p, observed, BT * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_scale, scale, B * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_shift, shift, B * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_i32.p, first, BW * sizeof(int), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_count, count, BW * sizeof(int), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_ranks, ranks, num_ranks * sizeof(int), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_steps.p, steps_before.data(), (BW + 1) * sizeof(long long), hipMemcpyHostToDevice,
                         stream));
  std::vector<double> mom;
  const double nan = std::nan("");
  for (size_t i = 0; i + 1 < starts.size(); ++i) {
    const size_t p0 = starts[i], pairs = starts[i + 1] - p0;
    if (pairs == 0) continue;
    const size_t steps = (size_t)(steps_before[p0 + pairs] - steps_before[p0]);
    int max_count = 0;
    for (size_t p = p0; p < p0 + pairs; ++p) max_count = count[p] > max_count ? count[p] : max_count;
    if (host_draws) {
      const size_t g0 = p0 / W, groups = (p0 + pairs - 1) / W - g0 + 1;
      HIP_TRY(hipMemcpyAsync(d_draws.p, host_draws + g0 * group_doubles, groups * group_doubles * sizeof(double),
                             hipMemcpyHostToDevice, stream));
      HIP_TRY(ci::paths_launch_f64(stream, N, T, W, (int)p0, (int)pairs, max_count, d_draws.p, (int)g0, d_f64.p,
                                   d_scale, d_shift, d_i32.p, d_count, d_steps.p, d_X.p, d_mom, d_obsexc, d_at,
                                   d_exc, d_exceed));
    } else {
      HIP_TRY(ci::paths_launch(stream, link, N, T, W, (int)p0, (int)pairs, max_count, traj, d_f64.p, d_scale, d_shift,
                               d_i32.p, d_count, d_steps.p, d_X.p, d_mom, d_obsexc, d_at, d_exc, d_exceed));
    }
    if (excursion_order)
      HIP_TRY(launch_select(stream, N, 1, (int)(2 * pairs), num_ranks, d_ranks, d_exc, nullptr, d_order,
                            nullptr));
    auto fetch = [&](void* dst, const void* src, size_t bytes) {
      return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) : hipSuccess;
    };
    mom.resize(steps * 4);
    if (center || spread) HIP_TRY(fetch(mom.data(), d_mom, steps * 4 * sizeof(double)));
    HIP_TRY(fetch(excursion ? excursion + p0 * 2 * N : nullptr, d_exc, pairs * 2 * N * sizeof(double)));
    HIP_TRY(fetch(excursion_order ? excursion_order + p0 * 2 * num_ranks : nullptr, d_order,
                  pairs * 2 * num_ranks * sizeof(double)));
    HIP_TRY(fetch(observed_excursion ? observed_excursion + p0 * 2 : nullptr, d_obsexc, pairs * 2 * sizeof(double)));
    HIP_TRY(fetch(at ? at + p0 * 2 : nullptr, d_at, pairs * 2 * sizeof(int)));
    HIP_TRY(fetch(exceed ? exceed + p0 * 2 : nullptr, d_exceed, pairs * 2 * sizeof(int)));
    HIP_TRY(hipStreamSynchronize(stream));
    // center, spread [B, W, 2, T]: NaN outside the window and, for the cumulative path, at the steps
    // without an observation
    for (size_t p = p0; p < p0 + pairs && (center || spread); ++p) {
      const int f = first[p], n = count[p];
      const double* obs = observed + (p / W) * (size_t)T;
      const double* m = mom.data() + (size_t)(steps_before[p] - steps_before[p0]) * 4;
      for (int k = 0; k < 2; ++k) {
        double* rows[2] = {center ? center + (p * 2 + k) * T : nullptr, spread ? spread + (p * 2 + k) * T : nullptr};
        for (int j = 0; j < 2; ++j) {
          if (!rows[j]) continue;
          for (int t = 0; t < T; ++t) rows[j][t] = nan;
          for (int s = 0; s < n; ++s)
            if (k == 0 || obs[f + s] == obs[f + s]) rows[j][f + s] = m[((size_t)k * 2 + j) * n + s];
        }
      }
    }
  }
  return 0;
}

// ci_summarize_draws / ci_summarize_draws_f64: one series of draws from the host, uploaded into a
// scratch of its own, summarised on the null stream and given back.
template <class TIn>
static int summarize_draws_impl(int32_t device, int32_t num_draws, int32_t T, const TIn* trajectories,
                                double scale, double shift, const double* observed, const uint8_t* flags,
                                int32_t num_ranks, const int32_t* ranks, double* value_order,
                                double* cum_order, double* per_draw, double* per_draw_order) {
  if (!trajectories || !observed || !flags || !ranks) return fail("NULL argument");
  if (num_draws < 1 || T < 1) return fail("need num_draws >= 1 and T >= 1");
  if (check_ranks(num_ranks, ranks, num_draws)) return 1;
  HIP_TRY(hipSetDevice(device));
  const size_t TN = (size_t)T * num_draws;
  DevBuf<TIn> d_traj;
  SummScratch w;
  HIP_TRY(d_traj.alloc(TN));
  HIP_TRY(hipMemcpy(d_traj.p, trajectories, TN * sizeof(TIn), hipMemcpyHostToDevice));
  return summarize_resident<TIn>(nullptr, w, ci::LINK_IDENTITY, 1, T, num_draws, d_traj.p, &scale, &shift, observed, flags,
                                 num_ranks, ranks, value_order, cum_order, per_draw, per_draw_order);
}

// The group table of the pool entry points (CSR over the positions of the session's B series).
int check_groups(int B, int32_t G, const int32_t* offsets, const int32_t* members, const double* weights) {
  if (G < 1) return fail("num_groups must be >= 1, got %d", G);
  if (offsets[0] != 0) return fail("offsets[0] must be 0, got %d", offsets[0]);
  for (int g = 0; g < G; ++g) {
    if (offsets[g + 1] < offsets[g])
      return fail("offsets must not decrease: offsets[%d] = %d after %d", g + 1, offsets[g + 1], offsets[g]);
    if (offsets[g + 1] - offsets[g] > B)
      return fail("group %d has %d members, the session %d series", g, offsets[g + 1] - offsets[g], B);
    for (int k = offsets[g]; k < offsets[g + 1]; ++k) {
      if (members[k] < 0 || members[k] >= B)
        return fail("group %d: member %d out of range [0, %d)", g, members[k], B);
      if (k > offsets[g] && members[k] <= members[k - 1])
        return fail("group %d: members must be strictly ascending (%d after %d)", g, members[k], members[k - 1]);
      if (!std::isfinite(weights[k])) return fail("group %d: the weight of member %d is not finite", g, members[k]);
    }
  }
  return 0;
}

// The windows of ci_session_pool_event_trajectories: member k of a group from its step first[k] on,
// width[g] columns per group, in accumulators of S = out_stride columns.
static int check_windows(int T, int32_t G, const int32_t* offsets, const int32_t* members,
                         const int32_t* first, const int32_t* width, int32_t S) {
  if (S < 1) return fail("out_stride must be >= 1, got %d", S);
  for (int g = 0; g < G; ++g) {
    if (width[g] < 1 || width[g] > S)
      return fail("group %d: width %d outside [1, out_stride = %d]", g, width[g], S);
    if (width[g] > T)        // (a group without a member too: no row on the device is longer)
      return fail("group %d: width %d exceeds the session's %d steps", g, width[g], T);
    for (int k = offsets[g]; k < offsets[g + 1]; ++k) {
      if (first[k] < 0) return fail("group %d: the first step of member %d is negative (%d)", g, members[k], first[k]);
      if ((long long)first[k] + width[g] > T)
        return fail("group %d: member %d from step %d over %d columns ends beyond the session's %d steps",
                    g, members[k], first[k], width[g], T);
    }
  }
  return 0;
}

// The pool entry points: weighted sums over groups of series of the [B, N, T] float32 trajectories
// resident in HBM.  Everything is checked before the first device call.  The groups pass through the
// summary's `value` matrix (B * N*T doubles, allocated on first use and kept), as many at a time as
// fit it: no device memory beyond the scratch but the tables.
// first == NULL (ci_session_pool_trajectories / ci_ll_session_pool_trajectories): calendar time, a
// group is ONE row of N*T doubles on the device and on the host.
// Otherwise (ci_session_pool_event_trajectories): a group is N rows of S = out_stride doubles on the
// host and of min(S, T) on the device -- no width exceeds T, so min(num_groups, B) groups fit `value`
// at a time either way -- and the columns of a wider host row are zeroed on the host.
// link: one of ci::LINK_* (ci_link.h).
template <int LINK>
static void pool_launch(hipStream_t stream, bool event, bool aligned, dim3 grid, int N, int T, long long NT,
                        long long total, const float* traj, const int* d_off, const ci::PoolEntry* d_entries,
                        const int* d_width, int Sd, int has_init, double* pooled) {
  const dim3 block(ci::POOL_NT);
  if (!event && aligned)
    hipLaunchKernelGGL((ci::pool_kernel<true, LINK>), grid, block, 0, stream, NT, traj, d_off, d_entries,
                       has_init, pooled);
  else if (!event)
    hipLaunchKernelGGL((ci::pool_kernel<false, LINK>), grid, block, 0, stream, NT, traj, d_off, d_entries,
                       has_init, pooled);
  else if (aligned)
    hipLaunchKernelGGL((ci::pool_event_kernel<true, LINK>), grid, block, 0, stream, N, T, total, traj,
                       d_off, d_entries, d_width, Sd, has_init, pooled);
  else
    hipLaunchKernelGGL((ci::pool_event_kernel<false, LINK>), grid, block, 0, stream, N, T, total, traj,
                       d_off, d_entries, d_width, Sd, has_init, pooled);
}

static int pool_resident(int device, hipStream_t stream, SummScratch& w, int link, int B, int T, int N,
                         const float* traj, const double* scale, const double* shift, int32_t G,
                         const int32_t* offsets, const int32_t* members, const double* weights,
                         const int32_t* first, const int32_t* width, int32_t S,
                         const double* init, double* out) {
  if (check_groups(B, G, offsets, members, weights)) return 1;
  if (first && check_windows(T, G, offsets, members, first, width, S)) return 1;
  const long long NT = (long long)N * T;
  const size_t group_rows = first ? N : 1;                          // rows per group
  const long long Sh = first ? S : NT, Sd = first && T < S ? T : Sh;  // row length: host, device
  bool aligned = (first ? T : NT) % 4 == 0 && (reinterpret_cast<uintptr_t>(traj) & 15u) == 0u;
  std::vector<ci::PoolEntry> entries((size_t)offsets[G]);
  for (int k = 0; k < offsets[G]; ++k) {
    const int b = members[k], f = first ? first[k] : 0;
    entries[k] = ci::PoolEntry{(long long)b * NT + f, weights[k], scale[b], shift[b]};
    aligned = aligned && f % 4 == 0;
  }
  HIP_TRY(hipSetDevice(device));
  if (summ_scratch_alloc(w, B, T, N)) return 1;
  const int per_pass = G < B ? G : (B < 65535 ? B : 65535);       // groups that fit `value` (grid.y)
  DevBuf<ci::PoolEntry> d_entries;
  DevBuf<int> d_tables;                                             // offsets [G + 1], widths [G]
  HIP_TRY(d_entries.alloc(entries.size() ? entries.size() : 1));
  HIP_TRY(d_tables.alloc((size_t)2 * G + 1));
  if (!entries.empty())
    HIP_TRY(hipMemcpyAsync(d_entries.p, entries.data(), entries.size() * sizeof(ci::PoolEntry),
                           hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_tables.p, offsets, ((size_t)G + 1) * sizeof(int), hipMemcpyHostToDevice, stream));
  if (first)
    HIP_TRY(hipMemcpyAsync(d_tables.p + G + 1, width, (size_t)G * sizeof(int), hipMemcpyHostToDevice, stream));
  const long long quads = (long long)group_rows * ((Sd + 3) / 4);   // four elements per thread
  const unsigned blocks = (unsigned)((quads + ci::POOL_NT - 1) / ci::POOL_NT);
  const size_t host_pitch = (size_t)Sh * sizeof(double), dev_pitch = (size_t)Sd * sizeof(double);
  // `rows` rows between the host (pitch host_pitch) and `value`: one block when the pitches agree
  auto copy = [&](void* dst, const void* src, size_t rows, bool to_device) {
    const hipMemcpyKind kind = to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    if (Sd == Sh) return hipMemcpyAsync(dst, src, rows * dev_pitch, kind, stream);
    return hipMemcpy2DAsync(dst, to_device ? dev_pitch : host_pitch, src, to_device ? host_pitch : dev_pitch,
                            dev_pitch, rows, kind, stream);
  };
  for (int g0 = 0; g0 < G; g0 += per_pass) {
    const int ng = G - g0 < per_pass ? G - g0 : per_pass;
    const size_t rows = (size_t)ng * group_rows, at = (size_t)g0 * group_rows * Sh;
    if (init) HIP_TRY(copy(w.value.p, init + at, rows, true));
    const dim3 grid(blocks, ng);
    const int* d_off = d_tables.p + g0;
    const int* d_width = d_tables.p + G + 1 + g0;
    const int has_init = init ? 1 : 0;
    const auto launch = link == ci::LINK_LOG ? pool_launch<ci::LINK_LOG>
                        : link == ci::LINK_LOG1P ? pool_launch<ci::LINK_LOG1P> : pool_launch<ci::LINK_IDENTITY>;
    launch(stream, first != nullptr, aligned, grid, N, T, NT, (long long)B * NT, traj, d_off, d_entries.p,
           d_width, (int)Sd, has_init, w.value.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(copy(out + at, w.value.p, rows, false));
    HIP_TRY(hipStreamSynchronize(stream));
    for (size_t row = 0; Sd < Sh && row < rows; ++row)               // no width reaches these columns
      for (long long c = Sd; c < Sh; ++c) out[at + row * Sh + c] = 0.0;
  }
  return 0;
}

extern "C" {

int ci_session_set_link(ci_session* s, int32_t link) {
  if (!s) return fail("NULL argument");
  if (link < 0 || link >= ci::NUM_LINKS)
    return fail("ci_session_set_link: unknown link %d (CI_LINK_IDENTITY = 0, CI_LINK_LOG = 1, CI_LINK_LOG1P = 2)",
                link);
  s->link = link;
  return 0;
}

// The means over the draws of value[b, n, t] under the session's link: the transpose into `value`,
// its row means in `obs` -- the passes of a component of ci_session_summarize_components.
int ci_session_value_mean(ci_session* s, const double* scale, const double* shift, double* value_mean) {
  if (!s || !scale || !shift || !value_mean) return fail("NULL argument");
  if (refuse_draws_session(s, "ci_session_value_mean")) return 1;
  if (!s->ran) return fail("ci_session_value_mean needs a finished ci_session_run");
  const ci_problem& pb = s->pb;
  const int B = pb.num_series, T = pb.T, N = pb.num_chains * pb.num_results;
  HIP_TRY(hipSetDevice(pb.device));
  SummScratch& w = s->summ;
  if (summ_scratch_alloc(w, B, T, N)) return 1;
  hipStream_t stream = s->stream;
  double* d_scale = w.obs.p + (size_t)B * T;
  double* d_shift = d_scale + B;
  HIP_TRY(hipMemcpyAsync(d_scale, scale, B * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_shift, shift, B * sizeof(double), hipMemcpyHostToDevice, stream));
  launch_transpose<float>(stream, s->link, B, T, N, s->o_traj.p, d_scale, d_shift, w.value.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(ci::comp_launch_row_stats(stream, (size_t)B * T, N, w.value.p, w.obs.p, nullptr));
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipMemcpy(value_mean, w.obs.p, (size_t)B * T * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int ci_session_pool_event_trajectories(ci_session* s, const double* scale, const double* shift,
                                       int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                       const double* weights, const int32_t* first, const int32_t* width,
                                       int32_t out_stride, const double* init, double* out) {
  if (!s || !scale || !shift || !offsets || !members || !weights || !first || !width || !out)
    return fail("NULL argument");
  if (refuse_draws_session(s, "ci_session_pool_event_trajectories")) return 1;
  if (!s->ran) return fail("ci_session_pool_event_trajectories needs a finished ci_session_run");
  const ci_problem& pb = s->pb;
  return pool_resident(pb.device, s->stream, s->summ, s->link, pb.num_series, pb.T, pb.num_chains * pb.num_results,
                       s->o_traj.p, scale, shift, num_groups, offsets, members, weights, first, width,
                       out_stride, init, out);
}

int ci_session_pool_trajectories(ci_session* s, const double* scale, const double* shift,
                                 int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                 const double* weights, const double* init, double* out) {
  if (!s || !scale || !shift || !offsets || !members || !weights || !out) return fail("NULL argument");
  if (refuse_draws_session(s, "ci_session_pool_trajectories")) return 1;
  if (!s->ran) return fail("ci_session_pool_trajectories needs a finished ci_session_run");
  const ci_problem& pb = s->pb;
  return pool_resident(pb.device, s->stream, s->summ, s->link, pb.num_series, pb.T, pb.num_chains * pb.num_results,
                       s->o_traj.p, scale, shift, num_groups, offsets, members, weights, nullptr, nullptr, 0,
                       init, out);
}

int ci_ll_session_pool_trajectories(ci_ll_session* s, const double* scale, const double* shift,
                                    int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                    const double* weights, const double* init, double* out) {
  if (!s || !scale || !shift || !offsets || !members || !weights || !out) return fail("NULL argument");
  if (!s->h_ran) return fail("ci_ll_session_pool_trajectories needs a finished ci_ll_session_hmc_run");
  return pool_resident(s->device, s->stream, s->summ, ci::LINK_IDENTITY, s->B, s->T, s->h_C * s->h_S, s->h_traj.p, scale,
                       shift, num_groups, offsets, members, weights, nullptr, nullptr, 0, init, out);
}

int ci_session_summarize(ci_session* s, const double* scale, const double* shift,
                         const double* observed, const uint8_t* flags, int32_t num_ranks,
                         const int32_t* ranks, double* value_order, double* cum_order,
                         double* per_draw, double* per_draw_order) {
  if (!s || !scale || !shift || !observed || !flags || !ranks) return fail("NULL argument");
  if (refuse_draws_session(s, "ci_session_summarize")) return 1;
  if (!s->ran) return fail("ci_session_summarize needs a finished ci_session_run");
  const ci_problem& pb = s->pb;
  HIP_TRY(hipSetDevice(pb.device));
  return summarize_resident(s->stream, s->summ, s->link, pb.num_series, pb.T, pb.num_chains * pb.num_results,
                            s->o_traj.p, scale, shift, observed, flags, num_ranks, ranks, value_order,
                            cum_order, per_draw, per_draw_order);
}

int ci_session_summarize_windows(ci_session* s, const double* scale, const double* shift,
                                 const double* observed, int32_t num_windows, const int32_t* first,
                                 const int32_t* count, int32_t num_ranks, const int32_t* ranks,
                                 double* per_draw, double* per_draw_order) {
  if (!s || !scale || !shift || !observed || !first || !count || !ranks) return fail("NULL argument");
  if (refuse_draws_session(s, "ci_session_summarize_windows")) return 1;
  if (!s->ran) return fail("ci_session_summarize_windows needs a finished ci_session_run");
  const ci_problem& pb = s->pb;
  return windows_resident("ci_session_summarize_windows", pb.device, s->stream, s->link, pb.num_series, pb.T,
                          pb.num_chains * pb.num_results, s->o_traj.p, scale, shift, observed,
                          num_windows, first, count, num_ranks, ranks, per_draw, per_draw_order);
}

int ci_ll_session_summarize_windows(ci_ll_session* s, const double* scale, const double* shift,
                                    const double* observed, int32_t num_windows, const int32_t* first,
                                    const int32_t* count, int32_t num_ranks, const int32_t* ranks,
                                    double* per_draw, double* per_draw_order) {
  if (!s || !scale || !shift || !observed || !first || !count || !ranks) return fail("NULL argument");
  if (!s->h_ran) return fail("ci_ll_session_summarize_windows needs a finished ci_ll_session_hmc_run");
  return windows_resident("ci_ll_session_summarize_windows", s->device, s->stream, ci::LINK_IDENTITY, s->B, s->T,
                          s->h_C * s->h_S, s->h_traj.p, scale, shift, observed, num_windows, first,
                          count, num_ranks, ranks, per_draw, per_draw_order);
}

int ci_session_summarize_paths(ci_session* s, const double* scale, const double* shift,
                               const double* observed, int32_t num_windows, const int32_t* first,
                               const int32_t* count, int32_t num_ranks, const int32_t* ranks,
                               double* center, double* spread, double* excursion, double* excursion_order,
                               double* observed_excursion, int32_t* at, int32_t* exceed) {
  return ci_test_session_summarize_paths(s, scale, shift, observed, num_windows, first, count, num_ranks,
                                         ranks, center, spread, excursion, excursion_order,
                                         observed_excursion, at, exceed, CI_PATHS_MAX_BYTES, nullptr);
}

int ci_test_session_summarize_paths(ci_session* s, const double* scale, const double* shift,
                                    const double* observed, int32_t num_windows, const int32_t* first,
                                    const int32_t* count, int32_t num_ranks, const int32_t* ranks,
                                    double* center, double* spread, double* excursion,
                                    double* excursion_order, double* observed_excursion, int32_t* at,
                                    int32_t* exceed, int64_t max_bytes, int32_t* num_chunks) {
  if (!s || !scale || !shift || !observed || !first || !count || !ranks) return fail("NULL argument");
  if (refuse_draws_session(s, "ci_session_summarize_paths")) return 1;
  if (!s->ran) return fail("ci_session_summarize_paths needs a finished ci_session_run");
  const ci_problem& pb = s->pb;
  return paths_resident("ci_session_summarize_paths", pb.device, s->stream, s->link, pb.num_series, pb.T,
                        pb.num_chains * pb.num_results, s->o_traj.p, scale, shift, observed, num_windows,
                        first, count, num_ranks, ranks, center, spread, excursion, excursion_order,
                        observed_excursion, at, exceed, max_bytes, num_chunks);
}

int ci_ll_session_summarize_paths(ci_ll_session* s, const double* scale, const double* shift,
                                  const double* observed, int32_t num_windows, const int32_t* first,
                                  const int32_t* count, int32_t num_ranks, const int32_t* ranks,
                                  double* center, double* spread, double* excursion,
                                  double* excursion_order, double* observed_excursion, int32_t* at,
                                  int32_t* exceed) {
  if (!s || !scale || !shift || !observed || !first || !count || !ranks) return fail("NULL argument");
  if (!s->h_ran) return fail("ci_ll_session_summarize_paths needs a finished ci_ll_session_hmc_run");
  return paths_resident("ci_ll_session_summarize_paths", s->device, s->stream, ci::LINK_IDENTITY, s->B, s->T, s->h_C * s->h_S,
                        s->h_traj.p, scale, shift, observed, num_windows, first, count, num_ranks, ranks,
                        center, spread, excursion, excursion_order, observed_excursion, at, exceed,
                        CI_PATHS_MAX_BYTES, nullptr);
}

int ci_session_summarize_components(ci_session* s, const double* scale, const double* shift,
                                    int32_t num_ranks, const int32_t* ranks, double* trend_mean,
                                    double* trend_order, double* seasonal_mean, double* seasonal_order,
                                    double* regression_mean, double* regression_order,
                                    double* inclusion_prob, double* weight_mean, double* weight_order) {
  if (!s || !scale || !shift || !ranks) return fail("NULL argument");
  if (refuse_draws_session(s, "ci_session_summarize_components")) return 1;
  if (!s->ran) return fail("ci_session_summarize_components needs a finished ci_session_run");
  const ci_problem& pb = s->pb;
  const int B = pb.num_series, T = pb.T, P = pb.P, N = pb.num_chains * pb.num_results;
  const int K = s->o_seasonal.n ? pb.num_blocks : 0;
  const int R = num_ranks;
  if (check_ranks(R, ranks, N)) return 1;
  HIP_TRY(hipSetDevice(pb.device));
  SummScratch& w = s->summ;
  if (summ_scratch_alloc(w, B, T, N)) return 1;
  hipStream_t stream = s->stream;
  double* d_scale = w.obs.p + (size_t)B * T;
  double* d_shift = d_scale + B;
  HIP_TRY(hipMemcpyAsync(d_scale, scale, B * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_shift, shift, B * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(w.ranks.p, ranks, R * sizeof(int), hipMemcpyHostToDevice, stream));
  // One component at a time through the scratch: the [B*T, N] matrix in `value`, its row means in
  // `obs` (the observations ci_session_summarize keeps there are uploaded by every call of it), its
  // order statistics [B, R, T] in `order`.  `dst + off` of series b lies `pitch` doubles after
  // that of series b - 1 (the seasonal outputs interleave the blocks).
  auto reduce = [&](const double* M, double* d_mean, double* d_order, int Tc, double* mean_dst,
                    size_t mean_pitch, double* order_dst, size_t order_pitch) -> int {
    if (mean_dst) HIP_TRY(ci::comp_launch_row_stats(stream, (size_t)B * Tc, N, M, d_mean, nullptr));
    if (order_dst)
      HIP_TRY(launch_select(stream, N, Tc, B * Tc, R, w.ranks.p, M, nullptr, d_order, nullptr));
    HIP_TRY(hipStreamSynchronize(stream));
    if (mean_dst)
      HIP_TRY(hipMemcpy2D(mean_dst, mean_pitch * sizeof(double), d_mean, (size_t)Tc * sizeof(double),
                          (size_t)Tc * sizeof(double), B, hipMemcpyDeviceToHost));
    if (order_dst)
      HIP_TRY(hipMemcpy2D(order_dst, order_pitch * sizeof(double), d_order,
                          (size_t)R * Tc * sizeof(double), (size_t)R * Tc * sizeof(double), B,
                          hipMemcpyDeviceToHost));
    return 0;
  };
  if (trend_mean || trend_order) {
    HIP_TRY(ci::comp_launch_gather(stream, B, N, T, 1, 0, s->o_level.p, d_scale, d_shift, w.value.p));
    if (reduce(w.value.p, w.obs.p, w.order.p, T, trend_mean, T, trend_order, (size_t)R * T)) return 1;
  }
  for (int k = 0; k < K && (seasonal_mean || seasonal_order); ++k) {
    HIP_TRY(ci::comp_launch_gather(stream, B, N, T, K, k, s->o_seasonal.p, d_scale, nullptr, w.value.p));
    if (reduce(w.value.p, w.obs.p, w.order.p, T, seasonal_mean ? seasonal_mean + (size_t)k * T : nullptr,
               (size_t)K * T, seasonal_order ? seasonal_order + (size_t)k * R * T : nullptr,
               (size_t)K * R * T))
      return 1;
  }
  if (P > 0 && (regression_mean || regression_order)) {
    HIP_TRY(ci::comp_launch_regression(stream, B, N, T, P, s->Xt.p, s->o_w.p,
                                       s->ragged ? s->series_T.p : nullptr, d_scale, w.value.p));
    if (reduce(w.value.p, w.obs.p, w.order.p, T, regression_mean, T, regression_order, (size_t)R * T))
      return 1;
  }
  if (P > 0 && (inclusion_prob || weight_mean || weight_order)) {
    // the weights: the design columns take the place of the steps.  More columns than steps do not
    // fit the scratch: such a call takes a buffer of its own and gives it back.
    const size_t BP = (size_t)B * P;
    DevBuf<double> big;
    double *M = w.value.p, *d_mean = w.obs.p, *d_order = w.order.p;
    int* d_count = reinterpret_cast<int*>(w.cum.p);
    if (P > T) {
      hipError_t e = big.alloc(BP * N + BP * R + 2 * BP);
      if (e != hipSuccess) return fail("allocating the weight summary failed: %s", hipGetErrorString(e));
      M = big.p; d_order = M + BP * N; d_mean = d_order + BP * R;
      d_count = reinterpret_cast<int*>(d_mean + BP);
    }
    std::vector<int> count(BP);
    HIP_TRY(ci::comp_launch_gather(stream, B, N, P, 1, 0, s->o_w.p, nullptr, nullptr, M));
    HIP_TRY(ci::comp_launch_row_stats(stream, BP, N, M, d_mean, d_count));
    if (weight_order)
      HIP_TRY(launch_select(stream, N, P, B * P, R, w.ranks.p, M, nullptr, d_order, nullptr));
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy(count.data(), d_count, BP * sizeof(int), hipMemcpyDeviceToHost));
    if (weight_mean) HIP_TRY(hipMemcpy(weight_mean, d_mean, BP * sizeof(double), hipMemcpyDeviceToHost));
    if (weight_order)
      HIP_TRY(hipMemcpy(weight_order, d_order, BP * R * sizeof(double), hipMemcpyDeviceToHost));
    if (inclusion_prob)
      for (size_t e = 0; e < BP; ++e) inclusion_prob[e] = (double)count[e] / (double)N;
  }
  return 0;
}

int ci_summarize_draws(int32_t device, int32_t num_draws, int32_t T, const float* trajectories,
                       double scale, double shift, const double* observed, const uint8_t* flags,
                       int32_t num_ranks, const int32_t* ranks, double* value_order,
                       double* cum_order, double* per_draw, double* per_draw_order) {
  return summarize_draws_impl<float>(device, num_draws, T, trajectories, scale, shift, observed, flags,
                                     num_ranks, ranks, value_order, cum_order, per_draw, per_draw_order);
}

int ci_summarize_draws_f64(int32_t device, int32_t num_draws, int32_t T, const double* trajectories,
                           double scale, double shift, const double* observed, const uint8_t* flags,
                           int32_t num_ranks, const int32_t* ranks, double* value_order,
                           double* cum_order, double* per_draw, double* per_draw_order) {
  return summarize_draws_impl<double>(device, num_draws, T, trajectories, scale, shift, observed, flags,
                                      num_ranks, ranks, value_order, cum_order, per_draw, per_draw_order);
}

int ci_summarize_draw_paths_f64(int32_t device, int32_t num_groups, int32_t num_draws, int32_t T,
                                const double* draws, const double* scale, const double* shift,
                                const double* observed, int32_t num_windows, const int32_t* first,
                                const int32_t* count, int32_t num_ranks, const int32_t* ranks,
                                double* center, double* spread, double* excursion, double* excursion_order,
                                double* observed_excursion, int32_t* at, int32_t* exceed) {
  return ci_test_summarize_draw_paths_f64(device, num_groups, num_draws, T, draws, scale, shift, observed,
                                          num_windows, first, count, num_ranks, ranks, center, spread,
                                          excursion, excursion_order, observed_excursion, at, exceed,
                                          CI_PATHS_MAX_BYTES, nullptr);
}

int ci_test_summarize_draw_paths_f64(int32_t device, int32_t num_groups, int32_t num_draws, int32_t T,
                                     const double* draws, const double* scale, const double* shift,
                                     const double* observed, int32_t num_windows, const int32_t* first,
                                     const int32_t* count, int32_t num_ranks, const int32_t* ranks,
                                     double* center, double* spread, double* excursion,
                                     double* excursion_order, double* observed_excursion, int32_t* at,
                                     int32_t* exceed, int64_t max_bytes, int32_t* num_chunks) {
  const char* what = "ci_summarize_draw_paths_f64";
  if (!draws || !scale || !shift || !observed || !first || !count || !ranks)
    return fail("%s: NULL argument", what);
  if (num_groups < 1) return fail("%s: num_groups must be >= 1, got %d", what, num_groups);
  if (num_draws < 2) return fail("%s: num_draws must be >= 2, got %d", what, num_draws);
  if (T < 1) return fail("%s: T must be >= 1, got %d", what, T);
  for (int g = 0; g < num_groups; ++g) {
    if (!std::isfinite(scale[g])) return fail("%s: the scale of group %d is not finite", what, g);
    if (!std::isfinite(shift[g])) return fail("%s: the shift of group %d is not finite", what, g);
  }
  // (the null stream, as ci_summarize_draws: the call has no session)
  return paths_resident(what, device, nullptr, ci::LINK_IDENTITY, num_groups, T, num_draws, nullptr, scale, shift, observed,
                        num_windows, first, count, num_ranks, ranks, center, spread, excursion,
                        excursion_order, observed_excursion, at, exceed, max_bytes, num_chunks, draws);
}

int ci_ll_session_hmc_summarize(ci_ll_session* s, const double* scale, const double* shift,
                                const double* observed, const uint8_t* flags, int32_t num_ranks,
                                const int32_t* ranks, double* value_order, double* cum_order,
                                double* per_draw, double* per_draw_order) {
  if (!s || !scale || !shift || !observed || !flags || !ranks) return fail("NULL argument");
  if (!s->h_ran) return fail("ci_ll_session_hmc_summarize needs a finished ci_ll_session_hmc_run");
  HIP_TRY(hipSetDevice(s->device));
  return summarize_resident(s->stream, s->summ, ci::LINK_IDENTITY, s->B, s->T, s->h_C * s->h_S, s->h_traj.p, scale, shift,
                            observed, flags, num_ranks, ranks, value_order, cum_order, per_draw,
                            per_draw_order);
}

}  // extern "C"
