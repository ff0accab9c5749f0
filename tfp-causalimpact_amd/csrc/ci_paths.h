// ci_paths.h -- per-draw MAXIMAL STANDARDISED EXCURSIONS of whole paths over sub-windows of the
// session's steps, straight from the [B, N, T] float32 trajectories resident in HBM
// (ci_session_summarize_paths, ci_ll_session_summarize_paths): what a simultaneous band and a
// whole-path test of the effect are made of.  For series b, window w = (first, count) and pooled
// draw n, all in float64, with v[n, t] = trajectory[b, n, t] * scale[b] + shift[b] (two roundings, no
// FMA, as in ci_windows.h):
//   path 0 (prediction)         x0[n, t] = v[n, t]                               target observed[b, t]
//   path 1 (cumulative effect)  x1[n, t] = the running sum over s = first .. t, ascending, of
//                               point = -(v[n, s] - observed[b, s]), NaN points skipped   target 0.0
//     (the expressions of window_totals_kernel: x1 at the window's last step is its point_sum)
//   center_k[t] = (sum_n x_k[n, t]) / N       spread_k[t] = sqrt(sum_n (x_k[n, t] - center_k[t])^2 / (N - 1))
//   counted steps of path k: the window's steps with an observation and spread_k[t] > 0
//   excursion_k[n] = max over the counted t of |x_k[n, t] - center_k[t]| / spread_k[t]   (0.0: none)
//   observed_excursion_k = max over the counted t of |target_k[t] - center_k[t]| / spread_k[t]
//     (NaN: none), at_k the first t that attains it (-1: none)
//   exceed_k = #{n : excursion_k[n] >= observed_excursion_k}
// Subtract, abs and divide are rounded once each, so given center and spread a plain loop on the host
// reproduces the excursions, observed_excursion, at and exceed bit for bit.
//
// ORDER OF THE ADDITIONS OVER THE DRAWS (a fixed function of N alone, for both sums of a step): thread
// i of PATHS_NT = 256 adds the draws i, i + 256, i + 512, ... in ascending order starting from 0.0;
// the 64 partial sums of a wavefront are added pairwise at distances 32, 16, 8, 4, 2, 1 (lane l takes
// l + l', the lane above: __shfl_down); the four wavefronts' sums are added in ascending order.
//
// Three passes over a (series, window)'s own steps, none over the whole series:
//   path_values_kernel    the 64-step tiles a window intersects pass through LDS exactly as in
//                         window_totals_kernel (coalesced along t, then one lane per draw walks t in
//                         order); both paths go to a float64 scratch X[k][step][n] of the window's
//                         own steps, 64 consecutive draws per store;
//   path_moments_kernel   one workgroup per (window, path, step): the row of N draws, two sweeps;
//   path_excursion_kernel one thread per (window, path, draw) down the window's steps: coalesced
//                         rows of X, center and spread of a step the same address for every lane.
// path_observed_kernel (one thread per (window, path)) runs between the last two.
// No [B, T, N] matrix of the whole series is built; no load reaches outside the trajectories,
// observed and the tables (the trajectory loads are those of window_totals_kernel).
// path_values_f64_kernel is the first pass for float64 draws [G, N, T] handed in by the caller
// (ci_summarize_draw_paths_f64); the other passes, hence the order of the additions and every rounding
// after the first pass, are shared.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ci_link.h"

namespace ci {

constexpr int PATHS_TILE = 64;
constexpr int PATHS_NT = 256;

// The (series, window) pairs p0 .. p0 + gridDim.y - 1 of one chunk, in the order [B, W].  steps_before
// [B * W + 1]: the running total of count over the pairs, so that pair p keeps its values at
// X + (steps_before[p] - steps_before[p0]) * 2 * N and its moments at
// mom + (steps_before[p] - steps_before[p0]) * 4.
struct PathsChunk {
  int N, T, W, p0;
  const int* first;
  const int* count;
  const long long* steps_before;
  const double* obs;            // [B, T]
  const double* scales;         // [B]
  const double* shifts;
};

// The launches (ci_paths.hip) of one chunk's four passes -- `pairs` pairs from p0, max_count the
// longest window among them -- from the resident float32 trajectories under `link`, and from float64
// draws [groups, N, T] whose first group is g0.
hipError_t paths_launch(hipStream_t stream, int link, int N, int T, int W, int p0, int pairs, int max_count,
                        const float* traj, const double* obs, const double* scales, const double* shifts,
                        const int* first, const int* count, const long long* steps_before, double* X,
                        double* mom, double* observed_excursion, int* at, double* excursion, int* exceed);
hipError_t paths_launch_f64(hipStream_t stream, int N, int T, int W, int p0, int pairs, int max_count,
                            const double* draws, int g0, const double* obs, const double* scales,
                            const double* shifts, const int* first, const int* count,
                            const long long* steps_before, double* X, double* mom,
                            double* observed_excursion, int* at, double* excursion, int* exceed);

// grid (ceil(N / 64), pairs), one wavefront per workgroup.  X of a pair: [2][count][N].
// ALIGNED as in window_totals_kernel (T % 4 == 0 and a 16-byte aligned base).
// LINK (ci_link.h): v is link(that); the identity is the code without it.
template <bool ALIGNED, int LINK = LINK_IDENTITY>
__global__ __launch_bounds__(64) void path_values_kernel(PathsChunk c, const float* __restrict__ traj_all,
                                                         double* __restrict__ X_all) {
  __shared__ float tile[PATHS_TILE][PATHS_TILE + 1];      // 65 columns: lane l reads bank (l + t) % 32
  __shared__ double obs_tile[PATHS_TILE];
  const int lane = threadIdx.x, p = c.p0 + blockIdx.y, N = c.N, T = c.T;
  const size_t b = p / c.W;
  const int n0 = blockIdx.x * PATHS_TILE, n = n0 + lane;
  const int rows = N - n0 < PATHS_TILE ? N - n0 : PATHS_TILE;
  const int first = c.first[p], count = c.count[p], end = first + count;
  const float* traj = traj_all + (b * N + n0) * (size_t)T;
  const double* obs = c.obs + b * T;
  const double scale = c.scales[b], shift = c.shifts[b];
  double* X0 = X_all + (size_t)(c.steps_before[p] - c.steps_before[c.p0]) * 2 * N;
  double* X1 = X0 + (size_t)count * N;
  double point_sum = 0.0;
  for (int t0 = first / PATHS_TILE * PATHS_TILE; t0 < end; t0 += PATHS_TILE) {
    const int lo = first > t0 ? first : t0;
    const int hi = end < t0 + PATHS_TILE ? end : t0 + PATHS_TILE;    // (lo < hi <= T)
    if (ALIGNED) {
      const int q = 4 * (lane & 15), r0 = lane >> 4, t = t0 + q;     // t % 4 == 0, so t < T => t + 3 < T
      if (t < hi && t + 3 >= lo) {
#pragma unroll 8
        for (int r = r0; r < rows; r += 4) {
          const float4 f = *reinterpret_cast<const float4*>(traj + (size_t)r * T + t);
          tile[r][q] = f.x; tile[r][q + 1] = f.y; tile[r][q + 2] = f.z; tile[r][q + 3] = f.w;
        }
      }
    } else {
      const int t = t0 + lane;
      if (t >= lo && t < hi) {
#pragma unroll 16
        for (int r = 0; r < rows; ++r) tile[r][lane] = traj[(size_t)r * T + t];
      }
    }
    if (t0 + lane >= lo && t0 + lane < hi) obs_tile[lane] = obs[t0 + lane];
    __syncthreads();
    if (n < N) {
      for (int t = lo; t < hi; ++t) {
        const double v = link_value<LINK>(__dadd_rn(__dmul_rn((double)tile[lane][t - t0], scale), shift));
        const double point = -__dsub_rn(v, obs_tile[t - t0]);
        point_sum = __dadd_rn(point_sum, (point != point) ? 0.0 : point);
        X0[(size_t)(t - first) * N + n] = v;
        X1[(size_t)(t - first) * N + n] = point_sum;
      }
    }
    __syncthreads();                                                 // the next tile overwrites both
  }
}

// path_values_kernel for float64 draws [groups, N, T] that the caller uploaded
// (ci_summarize_draw_paths_f64: the pooled draws of a group of series): the same expressions, the same
// X.  `draws` holds the groups g0, g0 + 1, ... of the chunk only; obs, scales and shifts are indexed by
// the group itself.  A 64 x 64 float64 tile is 32 KiB; its rows are padded by one access width (65
// doubles: 33280 bytes, with obs_tile 33792 of static LDS), so that the walk down t -- lane l reads
// tile[l][j], 8 bytes at dword 130 l + 2 j -- takes each 32-lane half of a ds_read_b64 through 32
// distinct bank pairs.  A row's 64 steps are 512 contiguous bytes.  ALIGNED (T % 2 == 0 and a 16-byte
// aligned base): 16 bytes per lane, 32 lanes per row and two rows per load; t is even, so t < T
// implies t + 1 < T; the two 8-byte LDS stores of a lane are 16 bytes from its neighbour's (two-way on
// ds_write_b64, behind the global loads they wait for).  Otherwise one lane per step, 8 bytes each,
// consecutive doubles into LDS.  No load reaches outside draws, observed and the tables.
template <bool ALIGNED>
__global__ __launch_bounds__(64) void path_values_f64_kernel(PathsChunk c, int g0,
                                                             const double* __restrict__ draws,
                                                             double* __restrict__ X_all) {
  __shared__ double tile[PATHS_TILE][PATHS_TILE + 1];
  __shared__ double obs_tile[PATHS_TILE];
  const int lane = threadIdx.x, p = c.p0 + blockIdx.y, N = c.N, T = c.T;
  const size_t b = p / c.W;
  const int n0 = blockIdx.x * PATHS_TILE, n = n0 + lane;
  const int rows = N - n0 < PATHS_TILE ? N - n0 : PATHS_TILE;
  const int first = c.first[p], count = c.count[p], end = first + count;
  const double* traj = draws + ((b - g0) * N + n0) * (size_t)T;
  const double* obs = c.obs + b * T;
  const double scale = c.scales[b], shift = c.shifts[b];
  double* X0 = X_all + (size_t)(c.steps_before[p] - c.steps_before[c.p0]) * 2 * N;
  double* X1 = X0 + (size_t)count * N;
  double point_sum = 0.0;
  for (int t0 = first / PATHS_TILE * PATHS_TILE; t0 < end; t0 += PATHS_TILE) {
    const int lo = first > t0 ? first : t0;
    const int hi = end < t0 + PATHS_TILE ? end : t0 + PATHS_TILE;    // (lo < hi <= T)
    if (ALIGNED) {
      const int q = 2 * (lane & 31), r0 = lane >> 5, t = t0 + q;     // t % 2 == 0, so t < T => t + 1 < T
      if (t < hi && t + 1 >= lo) {
#pragma unroll 8
        for (int r = r0; r < rows; r += 2) {
          const double2 f = *reinterpret_cast<const double2*>(traj + (size_t)r * T + t);
          tile[r][q] = f.x; tile[r][q + 1] = f.y;
        }
      }
    } else {
      const int t = t0 + lane;
      if (t >= lo && t < hi) {
#pragma unroll 16
        for (int r = 0; r < rows; ++r) tile[r][lane] = traj[(size_t)r * T + t];
      }
    }
    if (t0 + lane >= lo && t0 + lane < hi) obs_tile[lane] = obs[t0 + lane];
    __syncthreads();
    if (n < N) {
      for (int t = lo; t < hi; ++t) {
        const double v = __dadd_rn(__dmul_rn(tile[lane][t - t0], scale), shift);
        const double point = -__dsub_rn(v, obs_tile[t - t0]);
        point_sum = __dadd_rn(point_sum, (point != point) ? 0.0 : point);
        X0[(size_t)(t - first) * N + n] = v;
        X1[(size_t)(t - first) * N + n] = point_sum;
      }
    }
    __syncthreads();                                                 // the next tile overwrites both
  }
}

// The sum of one value per thread of a PATHS_NT workgroup, in the order of the header; every thread
// gets it.
__device__ inline double paths_block_sum(double a, double* part) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) a = __dadd_rn(a, __shfl_down(a, d, 64));
  __syncthreads();                                                   // (part is free again)
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
  __syncthreads();
  return __dadd_rn(__dadd_rn(__dadd_rn(part[0], part[1]), part[2]), part[3]);
}

// The three kernels from here on are no templates: a unit that includes them emits them.  The host
// units (ci_session.h) take the declarations alone.
#ifndef CI_SEASONAL_DECL_ONLY

// grid (2 * the longest window of the chunk, pairs), PATHS_NT threads: blockIdx.x = 2 * step + path.
// mom of a pair: [path][center | spread][count].
__global__ __launch_bounds__(PATHS_NT) void path_moments_kernel(PathsChunk c, const double* __restrict__ X_all,
                                                                double* __restrict__ mom_all) {
  __shared__ double part[PATHS_NT / 64];
  const int p = c.p0 + blockIdx.y, k = blockIdx.x & 1, step = blockIdx.x >> 1, N = c.N;
  const int count = c.count[p];
  if (step >= count) return;                                         // (the whole workgroup)
  const size_t at = (size_t)(c.steps_before[p] - c.steps_before[c.p0]);
  const double* x = X_all + at * 2 * N + ((size_t)k * count + step) * N;
  double a = 0.0;
  for (int n = threadIdx.x; n < N; n += PATHS_NT) a = __dadd_rn(a, x[n]);
  const double center = __ddiv_rn(paths_block_sum(a, part), (double)N);
  a = 0.0;
  for (int n = threadIdx.x; n < N; n += PATHS_NT) {
    const double d = __dsub_rn(x[n], center);
    a = __dadd_rn(a, __dmul_rn(d, d));
  }
  const double spread = __dsqrt_rn(__ddiv_rn(paths_block_sum(a, part), (double)(N - 1)));
  if (threadIdx.x == 0) {
    double* mom = mom_all + at * 4 + (size_t)k * 2 * count;
    mom[step] = center;
    mom[count + step] = spread;
  }
}

// grid (ceil(pairs * 2 / 64)), 64 threads: thread = 2 * (pair of the chunk) + path.
// observed_excursion [pairs, 2], at [pairs, 2].
__global__ __launch_bounds__(64) void path_observed_kernel(PathsChunk c, int pairs, const double* __restrict__ mom_all,
                                                           double* __restrict__ observed_excursion,
                                                           int* __restrict__ at_out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= 2 * pairs) return;
  const int p = c.p0 + (i >> 1), k = i & 1;
  const size_t b = p / c.W;
  const int first = c.first[p], count = c.count[p];
  const double* obs = c.obs + b * c.T + first;
  const double* center = mom_all + (size_t)(c.steps_before[p] - c.steps_before[c.p0]) * 4 + (size_t)k * 2 * count;
  const double* spread = center + count;
  double best = __longlong_as_double(0x7ff8000000000000LL);
  int where = -1;
  for (int s = 0; s < count; ++s) {
    const double o = obs[s], sd = spread[s];
    if (o != o || !(sd > 0.0)) continue;
    const double z = __ddiv_rn(fabs(__dsub_rn(k ? 0.0 : o, center[s])), sd);
    if (where < 0 || z > best) { best = z; where = first + s; }
  }
  observed_excursion[i] = best;
  at_out[i] = where;
}

// grid (2 * ceil(N / PATHS_NT), pairs), PATHS_NT threads: blockIdx.x = 2 * (draw block) + path.
// excursion [pairs, 2, N]; exceed [pairs, 2], zeroed by the caller.
__global__ __launch_bounds__(PATHS_NT) void path_excursion_kernel(PathsChunk c, const double* __restrict__ X_all,
                                                                  const double* __restrict__ mom_all,
                                                                  const double* __restrict__ observed_excursion,
                                                                  double* __restrict__ excursion,
                                                                  int* __restrict__ exceed) {
  const int q = blockIdx.y, p = c.p0 + q, k = blockIdx.x & 1, N = c.N;
  const int n = (blockIdx.x >> 1) * PATHS_NT + threadIdx.x;
  if (n >= N) return;
  const size_t b = p / c.W;
  const int first = c.first[p], count = c.count[p];
  const size_t at = (size_t)(c.steps_before[p] - c.steps_before[c.p0]);
  const double* obs = c.obs + b * c.T + first;
  const double* x = X_all + at * 2 * N + (size_t)k * count * N + n;
  const double* center = mom_all + at * 4 + (size_t)k * 2 * count;
  const double* spread = center + count;
  double best = 0.0;
  for (int s = 0; s < count; ++s) {
    const double o = obs[s], sd = spread[s];
    if (o != o || !(sd > 0.0)) continue;                             // (the same for every lane)
    const double z = __ddiv_rn(fabs(__dsub_rn(x[(size_t)s * N], center[s])), sd);
    best = z > best ? z : best;
  }
  excursion[((size_t)q * 2 + k) * N + n] = best;
  if (best >= observed_excursion[2 * q + k]) atomicAdd(exceed + 2 * q + k, 1);
}

#endif  // CI_SEASONAL_DECL_ONLY

}  // namespace ci
