// Instantiation unit of the window totals (ci_windows.h) and their launch;
// ci_session_summarize_windows and ci_ll_session_summarize_windows (ci_summary.hip) call it.
#include "ci_windows.h"

namespace ci {

// The totals of W windows of each of B series: traj [B, N, T] float32, obs [B, T], scales, shifts
// [B], first, count [B, W] (checked by the caller: 0 <= first, 0 <= count, first + count <= T), out
// [B, W, 2, N]; all device pointers.  link: one of ci::LINK_* (checked by the caller).
template <int LINK>
static void windows_launch_link(hipStream_t stream, int B, int N, int T, int W, const float* traj,
                                const double* obs, const double* scales, const double* shifts,
                                const int* first, const int* count, double* out) {
  const dim3 grid((N + WIN_TILE - 1) / WIN_TILE, W, B), block(WIN_TILE);
  const bool aligned = T % 4 == 0 && (reinterpret_cast<uintptr_t>(traj) & 15u) == 0u;
  if (aligned)
    hipLaunchKernelGGL((window_totals_kernel<true, LINK>), grid, block, 0, stream, N, T, W, traj, obs, scales,
                       shifts, first, count, out);
  else
    hipLaunchKernelGGL((window_totals_kernel<false, LINK>), grid, block, 0, stream, N, T, W, traj, obs, scales,
                       shifts, first, count, out);
}

hipError_t windows_launch(hipStream_t stream, int link, int B, int N, int T, int W, const float* traj,
                          const double* obs, const double* scales, const double* shifts,
                          const int* first, const int* count, double* out) {
  if (link == LINK_LOG)
    windows_launch_link<LINK_LOG>(stream, B, N, T, W, traj, obs, scales, shifts, first, count, out);
  else if (link == LINK_LOG1P)
    windows_launch_link<LINK_LOG1P>(stream, B, N, T, W, traj, obs, scales, shifts, first, count, out);
  else
    windows_launch_link<LINK_IDENTITY>(stream, B, N, T, W, traj, obs, scales, shifts, first, count, out);
  return hipGetLastError();
}

}  // namespace ci
