// ci_windows.h -- per-draw totals over SUB-WINDOWS of the session's steps, straight from the
// [B, N, T] float32 trajectories resident in HBM (ci_session_summarize_windows,
// ci_ll_session_summarize_windows).  For series b, window w = (first, count) and pooled draw n,
// all in float64:
//   pred_sum = 0.0; point_sum = 0.0
//   for t = first .. first + count - 1, ascending:
//     v        = trajectory[b, n, t] * scale[b] + shift[b]      (two roundings, no FMA)
//     pred_sum = pred_sum + v
//     point    = -(v - observed[b, t])
//     if point == point: point_sum = point_sum + point         (NaN: no observation, skipped)
//   out[b, w, 0, n] = pred_sum;  out[b, w, 1, n] = point_sum
// -- the expressions of summ_cumsum_kernel (ci_summary.h) over the steps whose flag bit 1 is set, so
// a window equal to the post-period reproduces ci_session_summarize's per_draw bit for bit.
//
// One streaming pass: no [B, T, N] float64 matrix is built, and only the 64-step tiles a window
// intersects are read (a step outside the window is never loaded unless it shares a 16-byte quad with
// one inside).  The trajectories are coalesced along t and the sums run along t per draw, so a tile
// of 64 draws x 64 steps passes through LDS: loaded row by row, summed column by column with one
// lane per draw.  The tile stays float32 (widening is exact, the scaler is applied by the summing
// lane) and is padded to 65 columns: lane l reads bank (l + t) % 32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ci_link.h"

namespace ci {

constexpr int WIN_TILE = 64;

// The launch (ci_windows.hip): window_totals_kernel over W windows of B series under `link`.
hipError_t windows_launch(hipStream_t stream, int link, int B, int N, int T, int W, const float* traj,
                          const double* obs, const double* scales, const double* shifts,
                          const int* first, const int* count, double* out);

// grid (ceil(N/64), W, B), one wavefront per workgroup: (draw tile, window, series).
// ALIGNED (T % 4 == 0 and a 16-byte aligned base: every row then starts on a 16-byte boundary):
// float4 loads, 16 lanes per row and 4 rows per instruction; otherwise one float per lane.
// first, count [B, W]; out [B, W, 2, N].  Requires 0 <= first, 0 <= count, first + count <= T.
// LINK (ci_link.h): v is link(that); the identity is the code without it.
template <bool ALIGNED, int LINK = LINK_IDENTITY>
__global__ __launch_bounds__(64) void window_totals_kernel(int N, int T, int W,
                                                           const float* __restrict__ traj_all,
                                                           const double* __restrict__ obs_all,
                                                           const double* __restrict__ scales,
                                                           const double* __restrict__ shifts,
                                                           const int* __restrict__ first_all,
                                                           const int* __restrict__ count_all,
                                                           double* __restrict__ out_all) {
  __shared__ float tile[WIN_TILE][WIN_TILE + 1];
  __shared__ double obs_tile[WIN_TILE];
  const int lane = threadIdx.x, w = blockIdx.y;
  const size_t b = blockIdx.z;
  const int n0 = blockIdx.x * WIN_TILE, n = n0 + lane;
  const int rows = N - n0 < WIN_TILE ? N - n0 : WIN_TILE;        // draws of this tile
  const int first = first_all[b * W + w], end = first + count_all[b * W + w];
  const float* traj = traj_all + (b * N + n0) * (size_t)T;
  const double* obs = obs_all + b * T;
  const double scale = scales[b], shift = shifts[b];
  double pred_sum = 0.0, point_sum = 0.0;
  for (int t0 = first / WIN_TILE * WIN_TILE; t0 < end; t0 += WIN_TILE) {
    const int lo = first > t0 ? first : t0;                      // the window's steps in this tile
    const int hi = end < t0 + WIN_TILE ? end : t0 + WIN_TILE;    // (lo < hi <= T)
    if (ALIGNED) {
      const int c = 4 * (lane & 15), r0 = lane >> 4, t = t0 + c; // t % 4 == 0, so t < T => t + 3 < T
      if (t < hi && t + 3 >= lo) {
#pragma unroll 8
        for (int r = r0; r < rows; r += 4) {
          const float4 q = *reinterpret_cast<const float4*>(traj + (size_t)r * T + t);
          tile[r][c] = q.x; tile[r][c + 1] = q.y; tile[r][c + 2] = q.z; tile[r][c + 3] = q.w;
        }
      }
    } else {
      const int t = t0 + lane;
      if (t >= lo && t < hi) {
#pragma unroll 16
        for (int r = 0; r < rows; ++r) tile[r][lane] = traj[(size_t)r * T + t];
      }
    }
    if (t0 + lane >= lo && t0 + lane < hi) obs_tile[lane] = obs[t0 + lane];   // once per tile
    __syncthreads();
    if (n < N) {
      for (int t = lo; t < hi; ++t) {
        const double v = link_value<LINK>(__dadd_rn(__dmul_rn((double)tile[lane][t - t0], scale), shift));
        pred_sum = __dadd_rn(pred_sum, v);
        const double point = -__dsub_rn(v, obs_tile[t - t0]);
        point_sum = __dadd_rn(point_sum, (point != point) ? 0.0 : point);
      }
    }
    __syncthreads();                                             // the next tile overwrites both
  }
  if (n < N) {
    double* out = out_all + (b * W + w) * 2 * (size_t)N;
    out[n] = pred_sum;
    out[(size_t)N + n] = point_sum;
  }
}

}  // namespace ci
