// ci_pool_event.h -- ci_session_pool_event_trajectories: the weighted sums of ci_pool.h over WINDOWS
// of the members' trajectories, every member shifted to its own start: the draws of a pooled effect
// in event time.  The series of a panel have their own calendars, so column c of group g is step
// first[k] + c of member k; the group's width[g] columns are what all its members have.
//
// The arithmetic is that of ci_pool.h (float64, one rounding per operation, members in order):
//   acc = init (or 0.0);  for the members k of the group, ascending:
//     v = traj[member k][n][first[k] + c] * scale + shift;   acc = acc + w * v
// Columns at or beyond the width are written as 0.0 and never read.
#pragma once
#include "ci_pool.h"

namespace ci {

// CNT consecutive members added to a thread's four accumulators, in order, as pool_chunk does: the
// CNT (or 2 CNT) vector loads first, then the dependent float64 operations.  r: the thread's first
// element relative to a member's `start` (draw * T + column).  A member's window starts anywhere
// in its row and the rows of a session are T floats apart, so unless ALIGNED (every start and T a
// multiple of 4 on an aligned base) the offset of a quad from the 16-byte grid differs from member
// to member and from draw to draw: pool_pick takes it per thread.
template <bool ALIGNED, int CNT>
__device__ __forceinline__ void pool_event_chunk(const float* __restrict__ traj,
                                                 const PoolEntry* __restrict__ en, long long r,
                                                 unsigned base_m, double acc[4]) {
  float4 lo[CNT], hi[CNT];
#pragma unroll
  for (int u = 0; u < CNT; ++u) {
    const long long at = en[u].start + r;
    if (ALIGNED) {
      lo[u] = *reinterpret_cast<const float4*>(traj + at);
    } else {
      const long long a = at - (long long)((base_m + (unsigned)at) & 3u);
      lo[u] = *reinterpret_cast<const float4*>(traj + a);
      hi[u] = *reinterpret_cast<const float4*>(traj + a + 4);
    }
  }
#pragma unroll
  for (int u = 0; u < CNT; ++u) {
    const PoolEntry m = en[u];
    float v[4];
    if (ALIGNED) {
      v[0] = lo[u].x; v[1] = lo[u].y; v[2] = lo[u].z; v[3] = lo[u].w;
    } else {
      pool_pick(lo[u], hi[u], (base_m + (unsigned)(m.start + r)) & 3u, v);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double x = __dadd_rn(__dmul_rn((double)v[j], m.scale), m.shift);
      acc[j] = __dadd_rn(acc[j], __dmul_rn(m.w, x));
    }
  }
}

// grid (ceil(N * ceil(S / 4) / POOL_NT), groups of this launch): a thread owns four consecutive
// columns of one (group, draw) row of the accumulators; the (draw, quad) pairs are flattened over
// grid.x, quads fastest, so a wavefront reads runs of consecutive floats of every member.
// traj: the session's [B, N, T] trajectories, `total` = B*N*T floats; entries offsets[g] ..
// offsets[g + 1] are the members of group g, `start` the element of column 0 of draw 0 (series *
// N*T + first); widths[g] <= S; pooled [groups, N, S] float64 holds the initial accumulator when
// has_init, and the result afterwards.
template <bool ALIGNED>
__global__ __launch_bounds__(POOL_NT) void pool_event_kernel(int N, int T, long long total,
                                                             const float* __restrict__ traj,
                                                             const int* __restrict__ offsets,
                                                             const PoolEntry* __restrict__ entries,
                                                             const int* __restrict__ widths, int S,
                                                             int has_init, double* __restrict__ pooled) {
  const int Q = (S + 3) >> 2;                               // quads per row
  const long long i = (long long)blockIdx.x * POOL_NT + threadIdx.x;
  if (i >= (long long)N * Q) return;
  const int n = (int)(i / Q);
  const int c = (int)(i - (long long)n * Q) * 4;
  const int g = blockIdx.y;
  const int k0 = offsets[g], k1 = offsets[g + 1], W = widths[g];
  double* out = pooled + ((long long)g * N + n) * S + c;
  const int room = S - c < 4 ? S - c : 4;                   // columns of the row this thread writes
  const int left = W - c >= room ? room : (W - c > 0 ? W - c : 0);  // ... of them inside the width
  const bool out16 = room == 4 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0u;
  const unsigned base_m = (unsigned)(reinterpret_cast<uintptr_t>(traj) >> 2) & 3u;
  const long long r = (long long)n * T + c;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};                     // (stays 0.0 at and beyond the width)
  if (has_init) {
    if (out16 && left == 4) {
      const double2 i0 = *reinterpret_cast<const double2*>(out);
      const double2 i1 = *reinterpret_cast<const double2*>(out + 2);
      acc[0] = i0.x; acc[1] = i0.y; acc[2] = i1.x; acc[3] = i1.y;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < left) acc[j] = out[j];
    }
  }
  // A whole quad inside the width reads [at, at + 4) when ALIGNED: inside the member's row.
  // Otherwise it reads [a, a + 8), a = at rounded down to the 16-byte grid: up to 3 floats before the
  // quad and 4 after it.  Both ends are floats of the same buffer (the neighbouring row, draw or
  // series) except in front of the first series and behind the last.  Members ascend, and so do
  // their starts (first < T), so the first member of the group reaches lowest and the last one
  // highest: checked once per thread, and a quad that could leave [0, total) goes element by element.
  bool vec = left == 4 && k0 < k1;
  if (!ALIGNED && vec)
    vec = (entries[k0].start + r >= 4 || base_m == 0u) && entries[k1 - 1].start + r + 8 <= total;
  if (vec) {
    int k = k0;
    for (; k + POOL_AHEAD <= k1; k += POOL_AHEAD) pool_event_chunk<ALIGNED, POOL_AHEAD>(traj, entries + k, r, base_m, acc);
    if (k + 4 <= k1) { pool_event_chunk<ALIGNED, 4>(traj, entries + k, r, base_m, acc); k += 4; }
    if (k + 2 <= k1) { pool_event_chunk<ALIGNED, 2>(traj, entries + k, r, base_m, acc); k += 2; }
    if (k < k1) pool_event_chunk<ALIGNED, 1>(traj, entries + k, r, base_m, acc);
  } else {
    // the last columns of the width, and the quads at the two ends of the buffer
    for (int k = k0; k < k1; ++k) {
      const PoolEntry en = entries[k];
      const float* p = traj + en.start + r;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < left) {
          const double x = __dadd_rn(__dmul_rn((double)p[j], en.scale), en.shift);
          acc[j] = __dadd_rn(acc[j], __dmul_rn(en.w, x));
        }
      }
    }
  }
  if (out16) {
    *reinterpret_cast<double2*>(out) = make_double2(acc[0], acc[1]);
    *reinterpret_cast<double2*>(out + 2) = make_double2(acc[2], acc[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < room) out[j] = acc[j];
  }
}

}  // namespace ci
