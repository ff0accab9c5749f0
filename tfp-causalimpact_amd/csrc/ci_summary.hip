// ci_summary.hip -- the on-device summaries behind the C-ABI (kernels: ci_summary.h,
// ci_components.h, ci_predict.h): ci_session_summarize, ci_session_summarize_components,
// ci_session_summarize_predictions, ci_session_summarize_placebo, ci_session_pool_placebo,
// ci_session_pool_placebo_blocks, ci_session_simulate_placebo[_blocks], ci_session_pool_simulated_placebo[_blocks]
// (kernels: ci_placebo.h, ci_placebo_blocks.h),
// ci_session_summarize_windows, ci_ll_session_summarize_windows
// (kernel: ci_windows.h), ci_session_summarize_paths, ci_ll_session_summarize_paths (kernels: ci_paths.h),
// ci_session_set_link and ci_session_value_mean (the outcome link: ci_link.h),
// ci_ll_session_hmc_summarize on the trajectories a session holds, ci_summarize_draws[_f64] and
// ci_summarize_draw_paths_f64 on draws the caller hands in; ci_session_pool_trajectories, ci_ll_session_pool_trajectories and
// ci_session_pool_event_trajectories (kernels: ci_pool.h) on the trajectories a session holds.
#include <cmath>
#include <vector>

#include "ci_placebo.h"
#include "ci_placebo_blocks.h"
#include "ci_pool.h"
#include "ci_predict.h"
#include "ci_predict_blocks.h"
#include "ci_session.h"
#include "ci_summary.h"

static int check_ranks(int32_t num_ranks, const int32_t* ranks, int N) {
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
static hipError_t launch_select(hipStream_t stream, int N, int T, int rows, int R, const int* d_ranks,
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
static int summ_scratch_alloc(SummScratch& w, int B, int T, int N) {
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

// The launches of ci_components.hip (kernels: ci_components.h).
namespace ci {
hipError_t comp_launch_gather(hipStream_t stream, int B, int N, int T, int K, int k, const float* in,
                              const double* scales, const double* shifts, double* out);
hipError_t comp_launch_regression(hipStream_t stream, int B, int N, int T, int P, const float* Xt,
                                  const float* w, const int* series_T, const double* scales,
                                  double* out);
hipError_t comp_launch_row_stats(hipStream_t stream, size_t rows, int N, const double* M,
                                 double* mean, int* nonzero);
// The launch of ci_predict.hip (kernels: ci_predict.h).
hipError_t predict_launch(hipStream_t stream, int B, int has_slope, int num_seasons, int out,
                          const PredArgs& args);
// The launch of ci_placebo.hip (kernels: ci_placebo.h).
hipError_t placebo_launch(hipStream_t stream, int B, int has_slope, int num_seasons, int out,
                          const PlaceboArgs& args);
// The launches of ci_predict_blocks.hip and ci_placebo_blocks.hip (kernels: ci_predict_blocks.h,
// ci_placebo_blocks.h).
hipError_t predict_blocks_launch(hipStream_t stream, int B, int out, const PredBlocksArgs& args);
hipError_t placebo_blocks_launch(hipStream_t stream, int B, int out, const PlaceboBlocksArgs& args);
hipError_t placebo_blocks_pool_launch(hipStream_t stream, int E, const PlaceboBlocksPoolArgs& args);
hipError_t placebo_sim_launch(hipStream_t stream, int nb, int has_slope, int num_seasons, int link,
                              const PlaceboSimArgs& args);
hipError_t placebo_blocks_sim_launch(hipStream_t stream, int nb, int link, const PlaceboBlocksSimArgs& args);
hipError_t placebo_sim_entries_launch(hipStream_t stream, int E, int has_slope, int num_seasons, int link,
                                      const PlaceboSimArgs& args);
hipError_t placebo_blocks_sim_entries_launch(hipStream_t stream, int E, int link, const PlaceboBlocksSimArgs& args);
hipError_t placebo_pool_totals_launch(hipStream_t stream, int N, int O, int G, int c0, int c1,
                                      const int* offsets, const double* weights, const double* M, double* acc);
hipError_t placebo_sim_seen_launch(hipStream_t stream, size_t rows, int N, double* M, const double* seen,
                                   const int* counted, double* below, int rewrite);
hipError_t placebo_pool_launch(hipStream_t stream, int N, int O, int G, int which, int c0, int c1,
                               const int* offsets, const double* weights, const double* M, double* acc);
hipError_t placebo_finish_launch(hipStream_t stream, int N, size_t r0, size_t rows, int out,
                                 const double* acc, const double* seen, double* M);
// The launch of ci_windows.hip (kernel: ci_windows.h).
hipError_t windows_launch(hipStream_t stream, int link, int B, int N, int T, int W, const float* traj,
                          const double* obs, const double* scales, const double* shifts,
                          const int* first, const int* count, double* out);
// The launch of ci_paths.hip (kernels: ci_paths.h).
hipError_t paths_launch(hipStream_t stream, int link, int N, int T, int W, int p0, int pairs, int max_count,
                        const float* traj, const double* obs, const double* scales, const double* shifts,
                        const int* first, const int* count, const long long* steps_before, double* X,
                        double* mom, double* observed_excursion, int* at, double* excursion, int* exceed);
hipError_t paths_launch_f64(hipStream_t stream, int N, int T, int W, int p0, int pairs, int max_count,
                            const double* draws, int g0, const double* obs, const double* scales,
                            const double* shifts, const int* first, const int* count,
                            const long long* steps_before, double* X, double* mom,
                            double* observed_excursion, int* at, double* excursion, int* exceed);
}  // namespace ci

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
static int check_groups(int B, int32_t G, const int32_t* offsets, const int32_t* members,
                        const double* weights) {
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

// What ci_session_summarize_predictions and ci_session_summarize_placebo ask of a session: a trend
// with at most one block of 2 to 7 seasons, and a finished run.
static int pred_check_session(const ci_session* s, const char* who) {
  const ci_problem& pb = s->pb;
  if (pb.num_blocks > 1 || (pb.num_blocks == 1 && (pb.num_seasons[0] < 2 || pb.num_seasons[0] > 7))) {
    std::string blocks;
    for (int k = 0; k < pb.num_blocks; ++k) blocks += (k ? ", " : "") + std::to_string(pb.num_seasons[k]);
    return fail("%s takes a trend with at most one block of 2 to 7 seasons, "
                "this session has the blocks (%s)", who, blocks.c_str());
  }
  if (!s->ran) return fail("%s needs a finished ci_session_run", who);
  return 0;
}

// What ci_session_summarize_predictions_blocks and ci_session_summarize_placebo_blocks ask of a
// session: not ragged, a state of at most 64 components, and a finished run.
static int pred_blocks_check_session(const ci_session* s, const char* who) {
  const ci_problem& pb = s->pb;
  if (s->ragged) {
    const std::string name(who), tail("_blocks");
    const bool cut = name.size() > tail.size() && name.compare(name.size() - tail.size(), tail.size(), tail) == 0;
    return fail("%s takes no ragged session: their models (one block of 2 to 7 seasons at most) "
                "belong to the entry without _blocks, %s", who,
                (cut ? name.substr(0, name.size() - tail.size()) : name).c_str());
  }
  int d = 1 + (pb.has_slope ? 1 : 0);
  for (int k = 0; k < pb.num_blocks; ++k) d += pb.num_seasons[k] - 1;
  if (d > ci::PB_MAX_STATE) {
    std::string blocks;
    for (int k = 0; k < pb.num_blocks; ++k) blocks += (k ? ", " : "") + std::to_string(pb.num_seasons[k]);
    return fail("%s takes a state of at most %d components, this session has %d with the blocks (%s)",
                who, ci::PB_MAX_STATE, d, blocks.c_str());
  }
  if (!s->ran) return fail("%s needs a finished ci_session_run", who);
  return 0;
}

// The block list of a session as the block-model filters read it.
static ci::BlockModel pred_block_model(const ci_problem& pb) {
  ci::BlockModel m = {};
  m.has_slope = pb.has_slope ? 1 : 0;
  m.K = pb.num_blocks;
  m.d = 1 + m.has_slope;
  m.zmask = 1ull;
  for (int k = 0; k < m.K; ++k) {
    m.off[k] = m.d;
    m.ns[k] = pb.num_seasons[k];
    m.zmask |= 1ull << m.d;
    m.d += pb.num_seasons[k] - 1;
  }
  return m;
}

// On the device, once per session: per series the initial moments of its ci_series_params [B, 4],
// then [B] times the 1.0 the regression term is scaled by.
static int pred_init_upload(ci_session* s) {
  if (s->pred_init.p) return 0;
  const int B = s->pb.num_series;
  std::vector<double> init((size_t)5 * B, 1.0);
  for (int b = 0; b < B; ++b) {
    const ci_series_params& q = s->params[b];
    init[4 * b + 0] = q.init_level_loc;
    init[4 * b + 1] = q.init_level_scale * q.init_level_scale;
    init[4 * b + 2] = q.init_slope_scale * q.init_slope_scale;
    init[4 * b + 3] = q.init_seasonal_scale * q.init_seasonal_scale;
  }
  HIP_TRY(s->pred_init.alloc(init.size()));
  HIP_TRY(hipMemcpy(s->pred_init.p, init.data(), init.size() * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

// ci_session_summarize_predictions and, with `blocks`, ci_session_summarize_predictions_blocks: they
// differ in the sessions they take and in the filter they launch, in nothing else.
static int summarize_predictions(ci_session* s, bool blocks, const double* scale, const double* shift,
                                 int32_t num_ranks, const int32_t* ranks, double* forecast_mean,
                                 double* forecast_order, double* variance_mean, double* pit_mean,
                                 double* loglik) {
  if (!s || !scale || !shift || !ranks) return fail("NULL argument");
  const ci_problem& pb = s->pb;          // (not kpb: the inert block of a long trend-only series is no part of the model)
  if (blocks ? pred_blocks_check_session(s, "ci_session_summarize_predictions_blocks")
             : pred_check_session(s, "ci_session_summarize_predictions"))
    return 1;
  const int B = pb.num_series, T = pb.T, P = pb.P, N = pb.num_chains * pb.num_results;
  const int NS = pb.num_blocks ? pb.num_seasons[0] : 0, R = num_ranks;
  if (check_ranks(R, ranks, N)) return 1;
  HIP_TRY(hipSetDevice(pb.device));
  SummScratch& w = s->summ;
  if (summ_scratch_alloc(w, B, T, N)) return 1;
  hipStream_t stream = s->stream;
  double* d_scale = w.obs.p + (size_t)B * T;
  double* d_shift = d_scale + B;
  if (pred_init_upload(s)) return 1;
  HIP_TRY(hipMemcpyAsync(d_scale, scale, B * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_shift, shift, B * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(w.ranks.p, ranks, R * sizeof(int), hipMemcpyHostToDevice, stream));
  // The regression term of every draw and step in `cum`, once; then one filter pass per requested
  // matrix through `value`, its row means in `obs`, its order statistics in `order`, the per-draw
  // log-likelihoods (with the first pass) in `draw`.
  const int* d_series_T = s->ragged ? s->series_T.p : nullptr;
  if (P > 0)
    HIP_TRY(ci::comp_launch_regression(stream, B, N, T, P, s->Xt.p, s->o_w.p, d_series_T,
                                       s->pred_init.p + (size_t)4 * B, w.cum.p));
  ci::PredArgs a;
  a.N = N; a.T = T;
  a.y = s->y.p; a.mask = s->mask.p; a.season_change = s->season_change.p; a.series_T = d_series_T;
  a.obs = s->o_obs.p; a.lscale = s->o_lscale.p; a.sscale = s->o_sscale.p; a.drift = s->o_drift.p;
  a.init = s->pred_init.p; a.scales = d_scale; a.shifts = d_shift;
  a.reg = P > 0 ? w.cum.p : nullptr;
  a.out = w.value.p;
  ci::PredBlocksArgs ab;
  if (blocks) ab.m = pred_block_model(pb);
  bool ll_pending = loglik != nullptr;
  auto pass = [&](int which, double* mean_dst, double* order_dst) -> int {
    a.ll = ll_pending ? w.draw.p : nullptr;
    if (blocks) {
      ab.p = a;
      HIP_TRY(ci::predict_blocks_launch(stream, B, which, ab));
    } else {
      HIP_TRY(ci::predict_launch(stream, B, pb.has_slope, NS, which, a));
    }
    if (mean_dst) HIP_TRY(ci::comp_launch_row_stats(stream, (size_t)B * T, N, w.value.p, w.obs.p, nullptr));
    if (order_dst)
      HIP_TRY(launch_select(stream, N, T, B * T, R, w.ranks.p, w.value.p, nullptr, w.order.p, nullptr));
    HIP_TRY(hipStreamSynchronize(stream));
    if (mean_dst)
      HIP_TRY(hipMemcpy(mean_dst, w.obs.p, (size_t)B * T * sizeof(double), hipMemcpyDeviceToHost));
    if (order_dst)
      HIP_TRY(hipMemcpy(order_dst, w.order.p, (size_t)B * R * T * sizeof(double), hipMemcpyDeviceToHost));
    if (ll_pending)
      HIP_TRY(hipMemcpy(loglik, w.draw.p, (size_t)B * N * sizeof(double), hipMemcpyDeviceToHost));
    ll_pending = false;
    return 0;
  };
  if ((forecast_mean || forecast_order) && pass(ci::PRED_FORECAST, forecast_mean, forecast_order)) return 1;
  if (variance_mean && pass(ci::PRED_VARIANCE, variance_mean, nullptr)) return 1;
  if ((pit_mean || ll_pending) && pass(ci::PRED_PIT, pit_mean, nullptr)) return 1;
  return 0;
}

int ci_session_summarize_predictions(ci_session* s, const double* scale, const double* shift,
                                     int32_t num_ranks, const int32_t* ranks, double* forecast_mean,
                                     double* forecast_order, double* variance_mean, double* pit_mean,
                                     double* loglik) {
  return summarize_predictions(s, false, scale, shift, num_ranks, ranks, forecast_mean, forecast_order,
                               variance_mean, pit_mean, loglik);
}

int ci_session_summarize_predictions_blocks(ci_session* s, const double* scale, const double* shift,
                                            int32_t num_ranks, const int32_t* ranks, double* forecast_mean,
                                            double* forecast_order, double* variance_mean, double* pit_mean,
                                            double* loglik) {
  return summarize_predictions(s, true, scale, shift, num_ranks, ranks, forecast_mean, forecast_order,
                               variance_mean, pit_mean, loglik);
}

// The origin table of ci_session_summarize_placebo and ci_session_simulate_placebo: max_origins in
// [1, T], horizon >= 1, every row ascending with -1 only at the end, o + H_b <= T_b.
static int check_placebo_plan(const ci_session* s, int O, const int32_t* origins, const int32_t* horizon) {
  const int B = s->pb.num_series, T = s->pb.T;
  if (O < 1 || O > T) return fail("max_origins must be in [1, %d], got %d", T, O);
  for (int b = 0; b < B; ++b) {
    const int Tb = s->ragged ? s->lengths[b] : T, Hb = horizon[b];
    if (Hb < 1) return fail("horizon[%d] must be at least 1, got %d", b, Hb);
    const int32_t* row = origins + (size_t)b * O;
    bool ended = false;
    for (int i = 0; i < O; ++i) {
      const int o = row[i];
      if (o == -1) { ended = true; continue; }
      if (o < 0) return fail("origins[%d, %d] must be a step or -1 (unused), got %d", b, i, o);
      if (ended || (i > 0 && o <= row[i - 1]))
        return fail("origins[%d] must be strictly ascending with the unused slots (-1) at the end "
                    "(slot %d holds %d)", b, i, o);
      if ((long long)o + Hb > Tb)
        return fail("origins[%d, %d] = %d with horizon %d reaches beyond the series' %d steps", b, i, o, Hb, Tb);
    }
  }
  return 0;
}

// ci_session_summarize_placebo and, with `blocks`, ci_session_summarize_placebo_blocks, likewise.
static int summarize_placebo(ci_session* s, bool blocks, const double* scale, const double* shift,
                             int32_t max_origins, const int32_t* origins, const int32_t* horizon,
                             double* predicted_mean, double* spread_mean, double* pit_mean) {
  if (!s || !scale || !shift || !origins || !horizon) return fail("NULL argument");
  const ci_problem& pb = s->pb;          // (not kpb: the inert block of a long trend-only series is no part of the model)
  if (blocks ? pred_blocks_check_session(s, "ci_session_summarize_placebo_blocks")
             : pred_check_session(s, "ci_session_summarize_placebo"))
    return 1;
  const int B = pb.num_series, T = pb.T, P = pb.P, N = pb.num_chains * pb.num_results;
  const int NS = pb.num_blocks ? pb.num_seasons[0] : 0, O = max_origins;
  if (check_placebo_plan(s, O, origins, horizon)) return 1;
  HIP_TRY(hipSetDevice(pb.device));
  SummScratch& w = s->summ;
  if (summ_scratch_alloc(w, B, T, N)) return 1;
  hipStream_t stream = s->stream;
  double* d_scale = w.obs.p + (size_t)B * T;
  double* d_shift = d_scale + B;
  if (pred_init_upload(s)) return 1;
  DevBuf<int> d_plan;                    // origins [B, O], then horizon [B]
  HIP_TRY(d_plan.alloc((size_t)B * O + B));
  HIP_TRY(hipMemcpyAsync(d_plan.p, origins, (size_t)B * O * sizeof(int), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_plan.p + (size_t)B * O, horizon, B * sizeof(int), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_scale, scale, B * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_shift, shift, B * sizeof(double), hipMemcpyHostToDevice, stream));
  // The regression term of every draw and step in `cum`, once; then one pass per requested matrix
  // [B * O, N] through `value` (O <= T: it fits), its row means in `obs`.
  const int* d_series_T = s->ragged ? s->series_T.p : nullptr;
  if (P > 0)
    HIP_TRY(ci::comp_launch_regression(stream, B, N, T, P, s->Xt.p, s->o_w.p, d_series_T,
                                       s->pred_init.p + (size_t)4 * B, w.cum.p));
  ci::PlaceboArgs a;
  a.p.N = N; a.p.T = T;
  a.p.y = s->y.p; a.p.mask = s->mask.p; a.p.season_change = s->season_change.p; a.p.series_T = d_series_T;
  a.p.obs = s->o_obs.p; a.p.lscale = s->o_lscale.p; a.p.sscale = s->o_sscale.p; a.p.drift = s->o_drift.p;
  a.p.init = s->pred_init.p; a.p.scales = d_scale; a.p.shifts = d_shift;
  a.p.reg = P > 0 ? w.cum.p : nullptr;
  a.p.out = w.value.p; a.p.ll = nullptr;
  a.O = O; a.origins = d_plan.p; a.horizon = d_plan.p + (size_t)B * O;
  ci::PlaceboBlocksArgs ab;
  if (blocks) { ab.q = a; ab.m = pred_block_model(pb); }
  auto pass = [&](int which, double* mean_dst) -> int {
    if (blocks) HIP_TRY(ci::placebo_blocks_launch(stream, B, which, ab));
    else HIP_TRY(ci::placebo_launch(stream, B, pb.has_slope, NS, which, a));
    HIP_TRY(ci::comp_launch_row_stats(stream, (size_t)B * O, N, w.value.p, w.obs.p, nullptr));
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy(mean_dst, w.obs.p, (size_t)B * O * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
  };
  if (predicted_mean && pass(ci::PLACEBO_SUM, predicted_mean)) return 1;
  if (spread_mean && pass(ci::PLACEBO_SPREAD, spread_mean)) return 1;
  if (pit_mean && pass(ci::PLACEBO_PIT, pit_mean)) return 1;
  HIP_TRY(hipStreamSynchronize(stream));   // (the uploads of a call that asks for nothing)
  return 0;
}

int ci_session_summarize_placebo(ci_session* s, const double* scale, const double* shift,
                                 int32_t max_origins, const int32_t* origins, const int32_t* horizon,
                                 double* predicted_mean, double* spread_mean, double* pit_mean) {
  return summarize_placebo(s, false, scale, shift, max_origins, origins, horizon, predicted_mean, spread_mean,
                           pit_mean);
}

int ci_session_summarize_placebo_blocks(ci_session* s, const double* scale, const double* shift,
                                        int32_t max_origins, const int32_t* origins, const int32_t* horizon,
                                        double* predicted_mean, double* spread_mean, double* pit_mean) {
  return summarize_placebo(s, true, scale, shift, max_origins, origins, horizon, predicted_mean, spread_mean,
                           pit_mean);
}

// ci_session_simulate_placebo and, with `blocks`, ci_session_simulate_placebo_blocks: the filter runs
// ONCE per chunk of series whose rows [nb * O, N] fit the scratch -- simulate into `value`, its row
// means and order statistics, the rows' download when `totals` is wanted, the count below `seen`,
// the rewrite to (x - seen)^2 in place and its row means.  TOTAL is a function of (b, slot, n) alone
// and every statistic one of its row, so nothing depends on where the chunks are cut.  max_rows
// (tests; 0: the scratch's B * T rows, which hold every call's B * O): the rows of a chunk;
// num_chunks (may be NULL): how many it took.
static int simulate_placebo(ci_session* s, bool blocks, const double* scale, const double* shift,
                            int32_t max_origins, const int32_t* origins, const int32_t* horizon, int32_t link,
                            const double* seen, int32_t num_ranks, const int32_t* ranks, double* predicted_mean,
                            double* spread_mean, double* below, double* total_order, double* totals,
                            int64_t max_rows, int32_t* num_chunks) {
  if (!s || !scale || !shift || !origins || !horizon || !ranks) return fail("NULL argument");
  const ci_problem& pb = s->pb;          // (not kpb: the inert block of a long trend-only series is no part of the model)
  const char* who = blocks ? "ci_session_simulate_placebo_blocks" : "ci_session_simulate_placebo";
  if (blocks ? pred_blocks_check_session(s, who) : pred_check_session(s, who)) return 1;
  const int B = pb.num_series, T = pb.T, P = pb.P, N = pb.num_chains * pb.num_results;
  const int NS = pb.num_blocks ? pb.num_seasons[0] : 0, O = max_origins, R = num_ranks;
  if (check_placebo_plan(s, O, origins, horizon)) return 1;
  if (link < 0 || link >= ci::NUM_LINKS)
    return fail("link must be CI_LINK_IDENTITY, CI_LINK_LOG or CI_LINK_LOG1P (0 to %d), got %d", ci::NUM_LINKS - 1, link);
  if (check_ranks(R, ranks, N)) return 1;
  if (!seen && (spread_mean || below)) return fail("spread_mean and below need `seen`, which is NULL");
  const size_t BO = (size_t)B * O;
  if (max_rows < 0 || (max_rows > 0 && max_rows < O))
    return fail("max_rows must hold the %d rows of one series, got %lld", O, (long long)max_rows);
  const size_t cap = max_rows > 0 && (size_t)max_rows < (size_t)B * T ? (size_t)max_rows : (size_t)B * T;
  const int nb_max = (int)(cap / O);     // (O <= T: at least one series)
  if (num_chunks) *num_chunks = (B + nb_max - 1) / nb_max;
  // the Philox key every series' fit ran on (ci_series_stream_key of its id, or the seed itself)
  std::vector<uint32_t> keys((size_t)2 * B);
  const int shared = (pb.flags & CI_FLAG_SHARED_SERIES_STREAMS) ? -1 : 0;
  for (int b = 0; b < B; ++b) {
    const int sid = s->ids.empty() ? pb.series_offset + b : s->ids[b];
    keys[2 * b] = ci::stream_key0(pb.seed[0], shared, sid);
    keys[2 * b + 1] = ci::stream_key1(pb.seed[1], shared, sid);
  }
  HIP_TRY(hipSetDevice(pb.device));
  SummScratch& w = s->summ;
  if (summ_scratch_alloc(w, B, T, N)) return 1;
  hipStream_t stream = s->stream;
  double* d_scale = w.obs.p + (size_t)B * T;
  double* d_shift = d_scale + B;
  if (pred_init_upload(s)) return 1;
  DevBuf<int> d_plan;                    // origins [B, O], horizon [B], counted [B, O]
  DevBuf<uint32_t> d_keys;               // [B, 2]
  DevBuf<double> d_stat;                 // seen, mean, spread, below: [B, O] each
  HIP_TRY(d_plan.alloc(2 * BO + B));
  HIP_TRY(d_keys.alloc((size_t)2 * B));
  HIP_TRY(d_stat.alloc(4 * BO));
  int* d_counted = d_plan.p + BO + B;
  double *d_seen = d_stat.p, *d_mean = d_stat.p + BO, *d_spread = d_stat.p + 2 * BO, *d_below = d_stat.p + 3 * BO;
  HIP_TRY(hipMemcpyAsync(d_plan.p, origins, BO * sizeof(int), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_plan.p + BO, horizon, B * sizeof(int), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_keys.p, keys.data(), keys.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  if (seen) HIP_TRY(hipMemcpyAsync(d_seen, seen, BO * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_scale, scale, B * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_shift, shift, B * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(w.ranks.p, ranks, R * sizeof(int), hipMemcpyHostToDevice, stream));
  const int* d_series_T = s->ragged ? s->series_T.p : nullptr;
  if (P > 0)
    HIP_TRY(ci::comp_launch_regression(stream, B, N, T, P, s->Xt.p, s->o_w.p, d_series_T,
                                       s->pred_init.p + (size_t)4 * B, w.cum.p));
  ci::PlaceboBlocksSimArgs ab;
  ci::PlaceboSimArgs& a = ab.s;
  a.q.p.N = N; a.q.p.T = T;
  a.q.p.y = s->y.p; a.q.p.mask = s->mask.p; a.q.p.season_change = s->season_change.p; a.q.p.series_T = d_series_T;
  a.q.p.obs = s->o_obs.p; a.q.p.lscale = s->o_lscale.p; a.q.p.sscale = s->o_sscale.p; a.q.p.drift = s->o_drift.p;
  a.q.p.init = s->pred_init.p; a.q.p.scales = d_scale; a.q.p.shifts = d_shift;
  a.q.p.reg = P > 0 ? w.cum.p : nullptr;
  a.q.p.out = w.value.p; a.q.p.ll = nullptr;
  a.q.O = O; a.q.origins = d_plan.p; a.q.horizon = d_plan.p + BO;
  a.kept = pb.num_results; a.chain_offset = (uint32_t)pb.chain_offset; a.keys = d_keys.p;
  if (blocks) ab.m = pred_block_model(pb);
  for (int b0 = 0; b0 < B; b0 += nb_max) {
    const int nb = B - b0 < nb_max ? B - b0 : nb_max;
    const size_t rows = (size_t)nb * O, off = (size_t)b0 * O;
    a.b0 = b0;
    a.counted = d_counted + off;
    if (blocks) HIP_TRY(ci::placebo_blocks_sim_launch(stream, nb, link, ab));
    else HIP_TRY(ci::placebo_sim_launch(stream, nb, pb.has_slope, NS, link, a));
    if (predicted_mean) HIP_TRY(ci::comp_launch_row_stats(stream, rows, N, w.value.p, d_mean + off, nullptr));
    if (total_order)
      HIP_TRY(launch_select(stream, N, O, (int)rows, R, w.ranks.p, w.value.p, nullptr,
                            w.order.p + (size_t)b0 * R * O, nullptr));
    if (totals) {
      HIP_TRY(hipStreamSynchronize(stream));
      HIP_TRY(hipMemcpy(totals + off * N, w.value.p, rows * N * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (spread_mean || below) {
      HIP_TRY(ci::placebo_sim_seen_launch(stream, rows, N, w.value.p, d_seen + off, d_counted + off,
                                          below ? d_below + off : nullptr, spread_mean != nullptr));
      if (spread_mean) HIP_TRY(ci::comp_launch_row_stats(stream, rows, N, w.value.p, d_spread + off, nullptr));
    }
  }
  HIP_TRY(hipStreamSynchronize(stream));
  if (predicted_mean) HIP_TRY(hipMemcpy(predicted_mean, d_mean, BO * sizeof(double), hipMemcpyDeviceToHost));
  if (spread_mean) HIP_TRY(hipMemcpy(spread_mean, d_spread, BO * sizeof(double), hipMemcpyDeviceToHost));
  if (below) HIP_TRY(hipMemcpy(below, d_below, BO * sizeof(double), hipMemcpyDeviceToHost));
  if (total_order)
    HIP_TRY(hipMemcpy(total_order, w.order.p, BO * R * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int ci_session_simulate_placebo(ci_session* s, const double* scale, const double* shift, int32_t max_origins,
                                const int32_t* origins, const int32_t* horizon, int32_t link, const double* seen,
                                int32_t num_ranks, const int32_t* ranks, double* predicted_mean,
                                double* spread_mean, double* below, double* total_order, double* totals) {
  return simulate_placebo(s, false, scale, shift, max_origins, origins, horizon, link, seen, num_ranks, ranks,
                          predicted_mean, spread_mean, below, total_order, totals, 0, nullptr);
}

int ci_session_simulate_placebo_blocks(ci_session* s, const double* scale, const double* shift,
                                       int32_t max_origins, const int32_t* origins, const int32_t* horizon,
                                       int32_t link, const double* seen, int32_t num_ranks, const int32_t* ranks,
                                       double* predicted_mean, double* spread_mean, double* below,
                                       double* total_order, double* totals) {
  return simulate_placebo(s, true, scale, shift, max_origins, origins, horizon, link, seen, num_ranks, ranks,
                          predicted_mean, spread_mean, below, total_order, totals, 0, nullptr);
}

int ci_test_session_simulate_placebo(ci_session* s, int32_t blocks, const double* scale, const double* shift,
                                     int32_t max_origins, const int32_t* origins, const int32_t* horizon,
                                     int32_t link, const double* seen, int32_t num_ranks, const int32_t* ranks,
                                     double* predicted_mean, double* spread_mean, double* below,
                                     double* total_order, double* totals, int64_t max_rows, int32_t* num_chunks) {
  return simulate_placebo(s, blocks != 0, scale, shift, max_origins, origins, horizon, link, seen, num_ranks, ranks,
                          predicted_mean, spread_mean, below, total_order, totals, max_rows, num_chunks);
}

// The plan of a pooled placebo call (ci_session_pool_placebo, ci_session_pool_simulated_placebo):
// one horizon >= 1 per group, every entry's origin row ascending with -1 only at the end and
// o + H_g <= T_b of its member; entry_horizon [K] is the group's horizon per entry.
static int check_pool_plan(const ci_session* s, int G, const int32_t* offsets, const int32_t* members, int O,
                           const int32_t* origins, const int32_t* horizon, std::vector<int>& entry_horizon) {
  const int T = s->pb.T, K = offsets[G];
  entry_horizon.assign((size_t)(K ? K : 1), 0);
  for (int g = 0; g < G; ++g) {
    const int Hg = horizon[g];
    if (Hg < 1) return fail("group %d: the horizon must be at least 1, got %d", g, Hg);
    for (int k = offsets[g]; k < offsets[g + 1]; ++k) {
      const int b = members[k], Tb = s->ragged ? s->lengths[b] : T;
      const int32_t* row = origins + (size_t)k * O;
      entry_horizon[k] = Hg;
      bool ended = false;
      for (int i = 0; i < O; ++i) {
        const int o = row[i];
        if (o == -1) { ended = true; continue; }
        if (o < 0)
          return fail("group %d, entry %d (member %d): slot %d must hold a step or -1 (unused), got %d", g, k, b, i, o);
        if (ended || (i > 0 && o <= row[i - 1]))
          return fail("group %d, entry %d (member %d): the origins must be strictly ascending with the unused "
                      "slots (-1) at the end (slot %d holds %d)", g, k, b, i, o);
        if ((long long)o + Hg > Tb)
          return fail("group %d, entry %d (member %d): the origin %d of slot %d with horizon %d reaches beyond "
                      "the series' %d steps", g, k, b, o, i, Hg, Tb);
      }
    }
  }
  return 0;
}

// The placebo forecasts of POOLED sums: per group, slot and draw the weighted sum S of the members'
// forecasts and the sum U of their predictive variances (include/causalimpact_amd.h).  The entries
// of the group table pass through `value` at most B at a time, a SUM pass and its accumulate, then a
// VAR pass and its accumulate; the accumulators [G, O, 2, N] and the tables are the call's own.
// With `blocks` ci_session_pool_placebo_blocks: the sessions and the filter of the block models, ONE
// pass per chunk that stores SUM into `value` and VAR into a buffer of the call's own, then the same
// two accumulates.  chunk_entries (tests; 0: B): the entries of a chunk, in [1, B].
static int pool_placebo(ci_session* s, bool blocks, const double* scale, const double* shift,
                        int32_t num_groups, const int32_t* offsets, const int32_t* members,
                        const double* weights, int32_t max_origins, const int32_t* origins,
                        const int32_t* horizon, const double* init, double* out,
                        const double* seen, double* predicted_mean, double* spread_mean,
                        double* pit_mean, int32_t chunk_entries) {
  if (!s || !scale || !shift || !offsets || !members || !weights || !origins || !horizon || !out)
    return fail("NULL argument");
  const ci_problem& pb = s->pb;
  if (blocks ? pred_blocks_check_session(s, "ci_session_pool_placebo_blocks")
             : pred_check_session(s, "ci_session_pool_placebo"))
    return 1;
  const int B = pb.num_series, T = pb.T, P = pb.P, N = pb.num_chains * pb.num_results;
  const int NS = pb.num_blocks ? pb.num_seasons[0] : 0, O = max_origins, G = num_groups;
  if (chunk_entries < 0 || chunk_entries > B)
    return fail("chunk_entries must be in [1, %d] (the session's series), got %d", B, chunk_entries);
  const int chunk = chunk_entries ? chunk_entries : B;
  if (check_groups(B, G, offsets, members, weights)) return 1;
  if (O < 1 || O > T) return fail("max_origins must be in [1, %d], got %d", T, O);
  if (!seen && (predicted_mean || spread_mean || pit_mean))
    return fail("predicted_mean, spread_mean and pit_mean need `seen`, the pooled observed sums");
  const int K = offsets[G];
  std::vector<int> entry_horizon;
  if (check_pool_plan(s, G, offsets, members, O, origins, horizon, entry_horizon)) return 1;
  HIP_TRY(hipSetDevice(pb.device));
  SummScratch& w = s->summ;
  if (summ_scratch_alloc(w, B, T, N)) return 1;
  hipStream_t stream = s->stream;
  double* d_scale = w.obs.p + (size_t)B * T;
  double* d_shift = d_scale + B;
  if (pred_init_upload(s)) return 1;
  const size_t rows = (size_t)G * O, acc_n = rows * 2 * N, Ka = K ? K : 1;
  DevBuf<int> d_int;                     // offsets [G + 1], members [K], horizon [K], origins [K, O]
  DevBuf<double> d_dbl;                  // acc [G, O, 2, N], seen [G, O], weights [K]
  DevBuf<double> d_var;                  // (blocks) VAR of a chunk [chunk, O, N]
  HIP_TRY(d_int.alloc((size_t)G + 1 + 2 * Ka + Ka * O));
  HIP_TRY(d_dbl.alloc(acc_n + rows + Ka));
  if (blocks && K > 0) HIP_TRY(d_var.alloc((size_t)(K < chunk ? K : chunk) * O * N));
  int* d_off = d_int.p;
  int* d_members = d_off + G + 1;
  int* d_horizon = d_members + Ka;
  int* d_origins = d_horizon + Ka;
  double* d_acc = d_dbl.p;
  double* d_seen = d_acc + acc_n;
  double* d_weights = d_seen + rows;
  HIP_TRY(hipMemcpyAsync(d_off, offsets, ((size_t)G + 1) * sizeof(int), hipMemcpyHostToDevice, stream));
  if (K > 0) {
    HIP_TRY(hipMemcpyAsync(d_members, members, (size_t)K * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_horizon, entry_horizon.data(), (size_t)K * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_origins, origins, (size_t)K * O * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_weights, weights, (size_t)K * sizeof(double), hipMemcpyHostToDevice, stream));
  }
  if (init)
    HIP_TRY(hipMemcpyAsync(d_acc, init, acc_n * sizeof(double), hipMemcpyHostToDevice, stream));
  else
    HIP_TRY(hipMemsetAsync(d_acc, 0, acc_n * sizeof(double), stream));
  if (seen) HIP_TRY(hipMemcpyAsync(d_seen, seen, rows * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_scale, scale, B * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_shift, shift, B * sizeof(double), hipMemcpyHostToDevice, stream));
  const int* d_series_T = s->ragged ? s->series_T.p : nullptr;
  if (P > 0 && K > 0)
    HIP_TRY(ci::comp_launch_regression(stream, B, N, T, P, s->Xt.p, s->o_w.p, d_series_T,
                                       s->pred_init.p + (size_t)4 * B, w.cum.p));
  ci::PlaceboArgs a;
  a.p.N = N; a.p.T = T;
  a.p.y = s->y.p; a.p.mask = s->mask.p; a.p.season_change = s->season_change.p; a.p.series_T = d_series_T;
  a.p.obs = s->o_obs.p; a.p.lscale = s->o_lscale.p; a.p.sscale = s->o_sscale.p; a.p.drift = s->o_drift.p;
  a.p.init = s->pred_init.p; a.p.scales = d_scale; a.p.shifts = d_shift;
  a.p.reg = P > 0 ? w.cum.p : nullptr;
  a.p.out = w.value.p; a.p.ll = nullptr;
  a.O = O;
  ci::PlaceboBlocksPoolArgs ab;
  if (blocks) { ab.m = pred_block_model(pb); ab.var = d_var.p; }
  // at most B entries at a time: [B * O, N] with O <= T fits `value`
  for (int c0 = 0; c0 < K; c0 += chunk) {
    const int c1 = K - c0 < chunk ? K : c0 + chunk;
    a.series_of = d_members + c0; a.origins = d_origins + (size_t)c0 * O; a.horizon = d_horizon + c0;
    if (blocks) {
      ab.q = a;
      HIP_TRY(ci::placebo_blocks_pool_launch(stream, c1 - c0, ab));
      HIP_TRY(ci::placebo_pool_launch(stream, N, O, G, 0, c0, c1, d_off, d_weights, w.value.p, d_acc));
      HIP_TRY(ci::placebo_pool_launch(stream, N, O, G, 1, c0, c1, d_off, d_weights, d_var.p, d_acc));
      continue;
    }
    for (int which = 0; which < 2; ++which) {
      HIP_TRY(ci::placebo_launch(stream, c1 - c0, pb.has_slope, NS, which ? ci::PLACEBO_VAR : ci::PLACEBO_SUM, a));
      HIP_TRY(ci::placebo_pool_launch(stream, N, O, G, which, c0, c1, d_off, d_weights, w.value.p, d_acc));
    }
  }
  HIP_TRY(hipMemcpyAsync(out, d_acc, acc_n * sizeof(double), hipMemcpyDeviceToHost, stream));
  // the means over the draws, one matrix at a time and as many rows as `value` and `obs` hold
  const size_t per_pass = (size_t)B * T;
  auto finish = [&](int which, double* mean_dst) -> int {
    for (size_t r0 = 0; r0 < rows; r0 += per_pass) {
      const size_t nr = rows - r0 < per_pass ? rows - r0 : per_pass;
      HIP_TRY(ci::placebo_finish_launch(stream, N, r0, nr, which, d_acc, d_seen, w.value.p));
      HIP_TRY(ci::comp_launch_row_stats(stream, nr, N, w.value.p, w.obs.p, nullptr));
      HIP_TRY(hipMemcpyAsync(mean_dst + r0, w.obs.p, nr * sizeof(double), hipMemcpyDeviceToHost, stream));
    }
    return 0;
  };
  if (predicted_mean && finish(ci::PLACEBO_SUM, predicted_mean)) return 1;
  if (spread_mean && finish(ci::PLACEBO_SPREAD, spread_mean)) return 1;
  if (pit_mean && finish(ci::PLACEBO_PIT, pit_mean)) return 1;
  HIP_TRY(hipStreamSynchronize(stream));
  return 0;
}

int ci_session_pool_placebo(ci_session* s, const double* scale, const double* shift,
                            int32_t num_groups, const int32_t* offsets, const int32_t* members,
                            const double* weights, int32_t max_origins, const int32_t* origins,
                            const int32_t* horizon, const double* init, double* out,
                            const double* seen, double* predicted_mean, double* spread_mean,
                            double* pit_mean) {
  return pool_placebo(s, false, scale, shift, num_groups, offsets, members, weights, max_origins, origins,
                      horizon, init, out, seen, predicted_mean, spread_mean, pit_mean, 0);
}

int ci_session_pool_placebo_blocks(ci_session* s, const double* scale, const double* shift,
                                   int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                   const double* weights, int32_t max_origins, const int32_t* origins,
                                   const int32_t* horizon, const double* init, double* out,
                                   const double* seen, double* predicted_mean, double* spread_mean,
                                   double* pit_mean) {
  return pool_placebo(s, true, scale, shift, num_groups, offsets, members, weights, max_origins, origins,
                      horizon, init, out, seen, predicted_mean, spread_mean, pit_mean, 0);
}

int ci_test_session_pool_placebo_blocks(ci_session* s, const double* scale, const double* shift,
                                        int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                        const double* weights, int32_t max_origins, const int32_t* origins,
                                        const int32_t* horizon, const double* init, double* out,
                                        const double* seen, double* predicted_mean, double* spread_mean,
                                        double* pit_mean, int32_t chunk_entries) {
  if (!s) return fail("NULL argument");
  if (chunk_entries < 1)
    return fail("chunk_entries must be in [1, %d] (the session's series), got %d", s->pb.num_series, chunk_entries);
  return pool_placebo(s, true, scale, shift, num_groups, offsets, members, weights, max_origins, origins,
                      horizon, init, out, seen, predicted_mean, spread_mean, pit_mean, chunk_entries);
}

// The SIMULATED placebo forecasts of pooled sums (include/causalimpact_amd.h): the entries of the group
// table pass through `value` at most `chunk` at a time -- ONE simulation pass (the entry-table build
// of simulate_placebo's kernel; TOTAL is a function of (series, origin, slot, horizon, n) alone) and
// its accumulate into POOL [G, O, N], the call's own.  `out` is downloaded, then the statistics of
// simulate_placebo are taken over the accumulators' rows, copied through `value` at most B * T rows
// at a time (whole groups, so that the selection's [G, R, O] layout holds per chunk): row means,
// order statistics, the count below `seen`, the rewrite to squares and its row means.  Nothing
// depends on where either kind of chunk is cut.  chunk_entries (tests; 0: B): in [1, B].
static int pool_simulated_placebo(ci_session* s, bool blocks, const double* scale, const double* shift,
                                  int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                  const double* weights, int32_t max_origins, const int32_t* origins,
                                  const int32_t* horizon, int32_t link, const double* init, double* out,
                                  const double* seen, const int32_t* counted, int32_t num_ranks,
                                  const int32_t* ranks, double* predicted_mean, double* spread_mean,
                                  double* below, double* total_order, int32_t chunk_entries) {
  if (!s || !scale || !shift || !offsets || !members || !weights || !origins || !horizon || !out || !ranks)
    return fail("NULL argument");
  const ci_problem& pb = s->pb;
  const char* who = blocks ? "ci_session_pool_simulated_placebo_blocks" : "ci_session_pool_simulated_placebo";
  if (blocks ? pred_blocks_check_session(s, who) : pred_check_session(s, who)) return 1;
  const int B = pb.num_series, T = pb.T, P = pb.P, N = pb.num_chains * pb.num_results;
  const int NS = pb.num_blocks ? pb.num_seasons[0] : 0, O = max_origins, G = num_groups, R = num_ranks;
  if (chunk_entries < 0 || chunk_entries > B)
    return fail("chunk_entries must be in [1, %d] (the session's series), got %d", B, chunk_entries);
  const int chunk = chunk_entries ? chunk_entries : B;
  if (check_groups(B, G, offsets, members, weights)) return 1;
  if (O < 1 || O > T) return fail("max_origins must be in [1, %d], got %d", T, O);
  if (link < 0 || link >= ci::NUM_LINKS)
    return fail("link must be CI_LINK_IDENTITY, CI_LINK_LOG or CI_LINK_LOG1P (0 to %d), got %d", ci::NUM_LINKS - 1, link);
  if (check_ranks(R, ranks, N)) return 1;
  const bool stats = predicted_mean || spread_mean || below || total_order;
  if (stats && (!seen || !counted))
    return fail("predicted_mean, spread_mean, below and total_order need `seen` and `counted`, the pooled "
                "observed totals and the member-steps they count");
  const int K = offsets[G];
  std::vector<int> entry_horizon;
  if (check_pool_plan(s, G, offsets, members, O, origins, horizon, entry_horizon)) return 1;
  // the Philox key every series' fit ran on (simulate_placebo's)
  std::vector<uint32_t> keys((size_t)2 * B);
  const int shared = (pb.flags & CI_FLAG_SHARED_SERIES_STREAMS) ? -1 : 0;
  for (int b = 0; b < B; ++b) {
    const int sid = s->ids.empty() ? pb.series_offset + b : s->ids[b];
    keys[2 * b] = ci::stream_key0(pb.seed[0], shared, sid);
    keys[2 * b + 1] = ci::stream_key1(pb.seed[1], shared, sid);
  }
  HIP_TRY(hipSetDevice(pb.device));
  SummScratch& w = s->summ;
  if (summ_scratch_alloc(w, B, T, N)) return 1;
  hipStream_t stream = s->stream;
  double* d_scale = w.obs.p + (size_t)B * T;
  double* d_shift = d_scale + B;
  if (pred_init_upload(s)) return 1;
  const size_t rows = (size_t)G * O, acc_n = rows * N, Ka = K ? K : 1;
  const size_t chunk_rows = (size_t)(K < chunk ? (K ? K : 1) : chunk) * O;
  DevBuf<int> d_int;                     // offsets [G + 1], members [K], horizon [K], origins [K, O],
                                         // cnt of a chunk's rows [chunk, O], counted [G, O]
  DevBuf<double> d_dbl;                  // acc [G, O, N], seen, mean, spread, below [G, O] each, order [G, R, O], weights [K]
  DevBuf<uint32_t> d_keys;               // [B, 2]
  HIP_TRY(d_int.alloc((size_t)G + 1 + 2 * Ka + Ka * O + chunk_rows + rows));
  HIP_TRY(d_dbl.alloc(acc_n + 4 * rows + rows * R + Ka));
  HIP_TRY(d_keys.alloc((size_t)2 * B));
  int* d_off = d_int.p;
  int* d_members = d_off + G + 1;
  int* d_horizon = d_members + Ka;
  int* d_origins = d_horizon + Ka;
  int* d_cnt = d_origins + Ka * O;
  int* d_counted = d_cnt + chunk_rows;
  double* d_acc = d_dbl.p;
  double* d_seen = d_acc + acc_n;
  double *d_mean = d_seen + rows, *d_spread = d_mean + rows, *d_below = d_spread + rows;
  double* d_order = d_below + rows;
  double* d_weights = d_order + rows * R;
  HIP_TRY(hipMemcpyAsync(d_off, offsets, ((size_t)G + 1) * sizeof(int), hipMemcpyHostToDevice, stream));
  if (K > 0) {
    HIP_TRY(hipMemcpyAsync(d_members, members, (size_t)K * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_horizon, entry_horizon.data(), (size_t)K * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_origins, origins, (size_t)K * O * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_weights, weights, (size_t)K * sizeof(double), hipMemcpyHostToDevice, stream));
  }
  if (init)
    HIP_TRY(hipMemcpyAsync(d_acc, init, acc_n * sizeof(double), hipMemcpyHostToDevice, stream));
  else
    HIP_TRY(hipMemsetAsync(d_acc, 0, acc_n * sizeof(double), stream));
  if (stats) {
    HIP_TRY(hipMemcpyAsync(d_seen, seen, rows * sizeof(double), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_counted, counted, rows * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(w.ranks.p, ranks, R * sizeof(int), hipMemcpyHostToDevice, stream));
  }
  HIP_TRY(hipMemcpyAsync(d_keys.p, keys.data(), keys.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_scale, scale, B * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_shift, shift, B * sizeof(double), hipMemcpyHostToDevice, stream));
  const int* d_series_T = s->ragged ? s->series_T.p : nullptr;
  if (P > 0 && K > 0)
    HIP_TRY(ci::comp_launch_regression(stream, B, N, T, P, s->Xt.p, s->o_w.p, d_series_T,
                                       s->pred_init.p + (size_t)4 * B, w.cum.p));
  ci::PlaceboBlocksSimArgs ab;
  ci::PlaceboSimArgs& a = ab.s;
  a.q.p.N = N; a.q.p.T = T;
  a.q.p.y = s->y.p; a.q.p.mask = s->mask.p; a.q.p.season_change = s->season_change.p; a.q.p.series_T = d_series_T;
  a.q.p.obs = s->o_obs.p; a.q.p.lscale = s->o_lscale.p; a.q.p.sscale = s->o_sscale.p; a.q.p.drift = s->o_drift.p;
  a.q.p.init = s->pred_init.p; a.q.p.scales = d_scale; a.q.p.shifts = d_shift;
  a.q.p.reg = P > 0 ? w.cum.p : nullptr;
  a.q.p.out = w.value.p; a.q.p.ll = nullptr;
  a.q.O = O;
  a.b0 = 0; a.kept = pb.num_results; a.chain_offset = (uint32_t)pb.chain_offset; a.keys = d_keys.p;
  a.counted = d_cnt;
  if (blocks) ab.m = pred_block_model(pb);
  // at most B entries at a time: [B * O, N] with O <= T fits `value`
  for (int c0 = 0; c0 < K; c0 += chunk) {
    const int c1 = K - c0 < chunk ? K : c0 + chunk;
    a.q.series_of = d_members + c0; a.q.origins = d_origins + (size_t)c0 * O; a.q.horizon = d_horizon + c0;
    if (blocks) HIP_TRY(ci::placebo_blocks_sim_entries_launch(stream, c1 - c0, link, ab));
    else HIP_TRY(ci::placebo_sim_entries_launch(stream, c1 - c0, pb.has_slope, NS, link, a));
    HIP_TRY(ci::placebo_pool_totals_launch(stream, N, O, G, c0, c1, d_off, d_weights, w.value.p, d_acc));
  }
  HIP_TRY(hipMemcpyAsync(out, d_acc, acc_n * sizeof(double), hipMemcpyDeviceToHost, stream));
  if (stats) {
    // whole groups, as many as `value` holds: (B * T / O) * O rows, at least O
    const size_t per_pass = ((size_t)B * T / O) * O;
    for (size_t r0 = 0; r0 < rows; r0 += per_pass) {
      const size_t nr = rows - r0 < per_pass ? rows - r0 : per_pass;
      HIP_TRY(hipMemcpyAsync(w.value.p, d_acc + r0 * N, nr * N * sizeof(double), hipMemcpyDeviceToDevice, stream));
      if (predicted_mean) HIP_TRY(ci::comp_launch_row_stats(stream, nr, N, w.value.p, d_mean + r0, nullptr));
      if (total_order)
        HIP_TRY(launch_select(stream, N, O, (int)nr, R, w.ranks.p, w.value.p, nullptr, d_order + r0 * R, nullptr));
      if (spread_mean || below) {
        HIP_TRY(ci::placebo_sim_seen_launch(stream, nr, N, w.value.p, d_seen + r0, d_counted + r0,
                                            below ? d_below + r0 : nullptr, spread_mean != nullptr));
        if (spread_mean) HIP_TRY(ci::comp_launch_row_stats(stream, nr, N, w.value.p, d_spread + r0, nullptr));
      }
    }
  }
  HIP_TRY(hipStreamSynchronize(stream));
  if (predicted_mean) HIP_TRY(hipMemcpy(predicted_mean, d_mean, rows * sizeof(double), hipMemcpyDeviceToHost));
  if (spread_mean) HIP_TRY(hipMemcpy(spread_mean, d_spread, rows * sizeof(double), hipMemcpyDeviceToHost));
  if (below) HIP_TRY(hipMemcpy(below, d_below, rows * sizeof(double), hipMemcpyDeviceToHost));
  if (total_order) HIP_TRY(hipMemcpy(total_order, d_order, rows * R * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int ci_session_pool_simulated_placebo(ci_session* s, const double* scale, const double* shift,
                                      int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                      const double* weights, int32_t max_origins, const int32_t* origins,
                                      const int32_t* horizon, int32_t link, const double* init, double* out,
                                      const double* seen, const int32_t* counted, int32_t num_ranks,
                                      const int32_t* ranks, double* predicted_mean, double* spread_mean,
                                      double* below, double* total_order) {
  return pool_simulated_placebo(s, false, scale, shift, num_groups, offsets, members, weights, max_origins,
                                origins, horizon, link, init, out, seen, counted, num_ranks, ranks,
                                predicted_mean, spread_mean, below, total_order, 0);
}

int ci_session_pool_simulated_placebo_blocks(ci_session* s, const double* scale, const double* shift,
                                             int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                             const double* weights, int32_t max_origins, const int32_t* origins,
                                             const int32_t* horizon, int32_t link, const double* init, double* out,
                                             const double* seen, const int32_t* counted, int32_t num_ranks,
                                             const int32_t* ranks, double* predicted_mean, double* spread_mean,
                                             double* below, double* total_order) {
  return pool_simulated_placebo(s, true, scale, shift, num_groups, offsets, members, weights, max_origins,
                                origins, horizon, link, init, out, seen, counted, num_ranks, ranks,
                                predicted_mean, spread_mean, below, total_order, 0);
}

int ci_test_session_pool_simulated_placebo(ci_session* s, int32_t blocks, const double* scale, const double* shift,
                                           int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                           const double* weights, int32_t max_origins, const int32_t* origins,
                                           const int32_t* horizon, int32_t link, const double* init, double* out,
                                           const double* seen, const int32_t* counted, int32_t num_ranks,
                                           const int32_t* ranks, double* predicted_mean, double* spread_mean,
                                           double* below, double* total_order, int32_t chunk_entries) {
  if (!s) return fail("NULL argument");
  if (chunk_entries < 1)
    return fail("chunk_entries must be in [1, %d] (the session's series), got %d", s->pb.num_series, chunk_entries);
  return pool_simulated_placebo(s, blocks != 0, scale, shift, num_groups, offsets, members, weights, max_origins,
                                origins, horizon, link, init, out, seen, counted, num_ranks, ranks,
                                predicted_mean, spread_mean, below, total_order, chunk_entries);
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
