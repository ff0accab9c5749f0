// Instantiation unit of the path excursions (ci_paths.h) and their launches;
// ci_session_summarize_paths, ci_ll_session_summarize_paths and ci_summarize_draw_paths_f64
// (ci_summary.hip) call them.
#include "ci_paths.h"

namespace ci {

// One chunk: the `pairs` (series, window) pairs from p0 on (in the order [B, W]), the longest of
// `max_count` steps: traj [B, N, T] float32, obs [B, T], scales, shifts [B], first, count [B, W],
// steps_before [B * W + 1] (the running total of count); X [steps of the chunk, 2, N], mom [steps of the chunk, 4], observed_excursion, at, exceed
// [pairs, 2], excursion [pairs, 2, N]; all device pointers.  The windows were checked by the caller
// (0 <= first, 0 <= count, first + count <= T), and 1 <= pairs <= 65535.
// draws64 != NULL (ci_summarize_draw_paths_f64): the first pass reads these float64 draws
// [groups of the chunk, N, T] instead, row 0 of them group g0's, and traj is not looked at.
// link: one of ci::LINK_* (checked by the caller), for the float32 trajectories of a session only.
template <bool ALIGNED>
static void path_values_launch(hipStream_t stream, int link, dim3 grid, const PathsChunk& c, const float* traj,
                               double* X) {
  if (link == LINK_LOG)
    hipLaunchKernelGGL((path_values_kernel<ALIGNED, LINK_LOG>), grid, dim3(PATHS_TILE), 0, stream, c, traj, X);
  else if (link == LINK_LOG1P)
    hipLaunchKernelGGL((path_values_kernel<ALIGNED, LINK_LOG1P>), grid, dim3(PATHS_TILE), 0, stream, c, traj, X);
  else
    hipLaunchKernelGGL((path_values_kernel<ALIGNED, LINK_IDENTITY>), grid, dim3(PATHS_TILE), 0, stream, c, traj, X);
}

static hipError_t paths_launch_any(hipStream_t stream, int link, int N, int T, int W, int p0, int pairs, int max_count,
                                   const float* traj, const double* draws64, int g0, const double* obs,
                                   const double* scales, const double* shifts, const int* first,
                                   const int* count, const long long* steps_before, double* X, double* mom,
                                   double* observed_excursion, int* at, double* excursion, int* exceed) {
  const PathsChunk c{N, T, W, p0, first, count, steps_before, obs, scales, shifts};
  const bool aligned = draws64 ? c.T % 2 == 0 && (reinterpret_cast<uintptr_t>(draws64) & 15u) == 0u
                               : c.T % 4 == 0 && (reinterpret_cast<uintptr_t>(traj) & 15u) == 0u;
  hipError_t e = hipMemsetAsync(exceed, 0, (size_t)2 * pairs * sizeof(int), stream);
  if (e != hipSuccess) return e;
  if (max_count > 0) {
    const dim3 grid((c.N + PATHS_TILE - 1) / PATHS_TILE, pairs);
    if (draws64 && aligned)
      hipLaunchKernelGGL(path_values_f64_kernel<true>, grid, dim3(PATHS_TILE), 0, stream, c, g0, draws64, X);
    else if (draws64)
      hipLaunchKernelGGL(path_values_f64_kernel<false>, grid, dim3(PATHS_TILE), 0, stream, c, g0, draws64, X);
    else if (aligned)
      path_values_launch<true>(stream, link, grid, c, traj, X);
    else
      path_values_launch<false>(stream, link, grid, c, traj, X);
    hipLaunchKernelGGL(path_moments_kernel, dim3(2 * max_count, pairs), dim3(PATHS_NT), 0, stream, c, X, mom);
  }
  hipLaunchKernelGGL(path_observed_kernel, dim3((2 * pairs + 63) / 64), dim3(64), 0, stream, c, pairs, mom,
                     observed_excursion, at);
  hipLaunchKernelGGL(path_excursion_kernel, dim3(2 * ((c.N + PATHS_NT - 1) / PATHS_NT), pairs),
                     dim3(PATHS_NT), 0, stream, c, X, mom, observed_excursion, excursion, exceed);
  return hipGetLastError();
}

hipError_t paths_launch(hipStream_t stream, int link, int N, int T, int W, int p0, int pairs, int max_count,
                        const float* traj, const double* obs, const double* scales, const double* shifts,
                        const int* first, const int* count, const long long* steps_before, double* X,
                        double* mom, double* observed_excursion, int* at, double* excursion, int* exceed) {
  return paths_launch_any(stream, link, N, T, W, p0, pairs, max_count, traj, nullptr, 0, obs, scales, shifts, first,
                          count, steps_before, X, mom, observed_excursion, at, excursion, exceed);
}

// The same chunk over float64 draws [groups of the chunk, N, T] on the device, the first of them group
// g0 = p0 / W's or an earlier one's; obs, scales, shifts and the window tables are those of all groups.
hipError_t paths_launch_f64(hipStream_t stream, int N, int T, int W, int p0, int pairs, int max_count,
                            const double* draws, int g0, const double* obs, const double* scales,
                            const double* shifts, const int* first, const int* count,
                            const long long* steps_before, double* X, double* mom,
                            double* observed_excursion, int* at, double* excursion, int* exceed) {
  return paths_launch_any(stream, LINK_IDENTITY, N, T, W, p0, pairs, max_count, nullptr, draws, g0, obs, scales, shifts, first,
                          count, steps_before, X, mom, observed_excursion, at, excursion, exceed);
}

}  // namespace ci
