// ci_pool.h -- weighted sums over groups of series of a session's resident predictive trajectories:
// the draws of a POOLED effect.  A sum of per-series quantiles is not a quantile of the sum; the band
// of "all geos" or "region north" needs the sum over series draw by draw, and a batch keeps its
// [B, N, T] float32 draws in HBM only.  One streaming pass reads them where they are.
//   pool_kernel        (ci_session_pool_trajectories, ci_ll_session_pool_trajectories): calendar
//                      time, the members' whole [N*T] blocks;
//   pool_event_kernel  (ci_session_pool_event_trajectories): event time, WINDOWS of the members'
//                      rows, every member shifted to its own start.  The series of a panel have their
//                      own calendars, so column c of group g is step first[k] + c of member k; the
//                      group's width[g] columns are what all its members have.
// A calendar sum is the event-time sum in which every member starts at step 0 and the width is T; the
// two kernels differ in how a thread finds its four elements and share everything below that.
//
// Arithmetic is float64 and ordered like the numpy loop it stands for:
//   acc = init (or 0.0);  for the members b of the group, ascending:
//     v = traj[b] * scale[b] + shift[b]      the value ci_session_summarize forms (two roundings;
//                                            under a LINK, ci_link.h, the link of that)
//     acc = acc + w * v                      (two roundings)
// so the result does not depend on the launch geometry, and a batch cut into several sessions
// continues one running sum through `init`, bit for bit.  In event time traj[b] is
// traj[member k][n][first[k] + c]; columns at or beyond the width are written as 0.0 and never read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ci_link.h"

namespace ci {

constexpr int POOL_NT = 256;       // threads per workgroup, four consecutive elements each
constexpr int POOL_AHEAD = 8;      // members whose loads are in flight ahead of the dependent adds

// One (group, member) entry of the sparse weight table.
struct PoolEntry {
  long long start;                 // the member's first element in the trajectories: of its [N*T]
                                   // block, or (event time) of column 0 of draw 0: series * N*T + first
  double w, scale, shift;
};

// float4 loads want 16-byte alignment; series b starts at element b * N*T, which is not a multiple
// of 4 for odd b when N*T is not.  A misaligned member is read as the two aligned float4 that
// cover the thread's four elements (the second is its neighbour's first: an L1 hit), and the four
// are picked by the member's offset m = 1..3.
__device__ __forceinline__ void pool_pick(const float4 a, const float4 b, unsigned m, float v[4]) {
  const float c[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = m == 0u ? c[j] : (m == 1u ? c[j + 1] : (m == 2u ? c[j + 2] : c[j + 3]));
}

// CNT consecutive members of a group added to a thread's four accumulators, in order: the CNT (or
// 2 CNT) vector loads first, then the dependent float64 operations.  `en`: the members' entries;
// r: the thread's first element relative to a member's `start`; base_m: the offset of `traj` from
// the 16-byte grid, in floats.  phase: what a member's `start` is added to for the offset of its
// quad from that grid, (phase + start) & 3.  In calendar time r is a multiple of 4 and phase is
// base_m: the offset is the same for every thread.  In event time a member's window starts anywhere
// in its row and the rows of a session are T floats apart, so unless ALIGNED (every start and T a
// multiple of 4 on an aligned base) the offset differs from member to member and from draw to draw:
// phase is base_m + r, per thread.
template <bool ALIGNED, int CNT, int LINK>
__device__ __forceinline__ void pool_chunk(const float* __restrict__ traj,
                                           const PoolEntry* __restrict__ en, long long r,
                                           unsigned phase, unsigned base_m, double acc[4]) {
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
      pool_pick(lo[u], hi[u], (phase + (unsigned)m.start) & 3u, v);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double x = link_value<LINK>(__dadd_rn(__dmul_rn((double)v[j], m.scale), m.shift));
      acc[j] = __dadd_rn(acc[j], __dmul_rn(m.w, x));
    }
  }
}

// The initial accumulator of a thread: its first `left` elements of `out`; `whole`: all four, and
// `out` 16-byte aligned.
__device__ __forceinline__ void pool_init(const double* out, bool whole, int left, double acc[4]) {
  if (whole) {
    const double2 i0 = *reinterpret_cast<const double2*>(out);
    const double2 i1 = *reinterpret_cast<const double2*>(out + 2);
    acc[0] = i0.x; acc[1] = i0.y; acc[2] = i1.x; acc[3] = i1.y;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < left) acc[j] = out[j];
  }
}

// The members k0 .. k1 - 1 of a group added to a thread's accumulators, in order.  vec: the thread's
// four elements of every member may be read by vector loads (the kernels say when); otherwise its
// first `left` elements are read one by one.
template <bool ALIGNED, int LINK>
__device__ __forceinline__ void pool_members(const float* __restrict__ traj,
                                             const PoolEntry* __restrict__ entries, int k0, int k1,
                                             long long r, unsigned phase, unsigned base_m, bool vec,
                                             int left, double acc[4]) {
  if (vec) {
    // whole chunks of POOL_AHEAD members, then the rest in chunks of 4, 2 and 1: every load is of a
    // member of the group, and the loads of a chunk are issued together, without a branch between
    int k = k0;
    for (; k + POOL_AHEAD <= k1; k += POOL_AHEAD) pool_chunk<ALIGNED, POOL_AHEAD, LINK>(traj, entries + k, r, phase, base_m, acc);
    if (k + 4 <= k1) { pool_chunk<ALIGNED, 4, LINK>(traj, entries + k, r, phase, base_m, acc); k += 4; }
    if (k + 2 <= k1) { pool_chunk<ALIGNED, 2, LINK>(traj, entries + k, r, phase, base_m, acc); k += 2; }
    if (k < k1) pool_chunk<ALIGNED, 1, LINK>(traj, entries + k, r, phase, base_m, acc);
  } else {
    for (int k = k0; k < k1; ++k) {
      const PoolEntry en = entries[k];
      const float* p = traj + en.start + r;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < left) {
          const double x = link_value<LINK>(__dadd_rn(__dmul_rn((double)p[j], en.scale), en.shift));
          acc[j] = __dadd_rn(acc[j], __dmul_rn(en.w, x));
        }
      }
    }
  }
}

// A thread's accumulators written to its `room` elements of `out`; out16: all four, and `out`
// 16-byte aligned.
__device__ __forceinline__ void pool_store(double* out, bool out16, int room, const double acc[4]) {
  if (out16) {
    *reinterpret_cast<double2*>(out) = make_double2(acc[0], acc[1]);
    *reinterpret_cast<double2*>(out + 2) = make_double2(acc[2], acc[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < room) out[j] = acc[j];
  }
}

// grid (ceil(NT / (4 POOL_NT)), groups of this launch): one group and a contiguous slice of the
// flattened N*T axis per workgroup.  traj: the [N*T] blocks of all series of the session; entries
// offsets[g] .. offsets[g + 1] are the members of group g; pooled [groups, NT] float64 holds the
// initial accumulator when has_init, and the result afterwards.
// ALIGNED: every member block starts 16-byte aligned (N*T a multiple of 4 on an aligned base):
// one float4 per member and thread.
template <bool ALIGNED, int LINK = LINK_IDENTITY>
__global__ __launch_bounds__(POOL_NT) void pool_kernel(long long NT,
                                                       const float* __restrict__ traj,
                                                       const int* __restrict__ offsets,
                                                       const PoolEntry* __restrict__ entries,
                                                       int has_init, double* __restrict__ pooled) {
  const long long e = ((long long)blockIdx.x * POOL_NT + threadIdx.x) * 4;
  if (e >= NT) return;
  const int g = blockIdx.y;
  const int k0 = offsets[g], k1 = offsets[g + 1];
  double* out = pooled + (size_t)g * NT + e;
  const int left = NT - e < 4 ? (int)(NT - e) : 4;          // elements of this thread
  const bool out16 = left == 4 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0u;
  const unsigned base_m = (unsigned)(reinterpret_cast<uintptr_t>(traj) >> 2) & 3u;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (has_init) pool_init(out, out16, left, acc);
  // The vector path reads [a, a + 4) (ALIGNED) or [a, a + 8) with a = the member's first element
  // rounded down to a multiple of 4: inside the member's block but for up to 3 elements before it
  // (the end of the series in front; none in front of series 0 on an aligned base) and up to 4 after
  // the thread's own, which stay inside the block while e + 8 <= NT.  The last elements of the slice
  // (and the first four on a misaligned base) go element by element.
  const bool vec = ALIGNED ? left == 4 : (e + 8 <= NT && (e >= 4 || base_m == 0u));
  pool_members<ALIGNED, LINK>(traj, entries, k0, k1, e, base_m, base_m, vec, left, acc);
  pool_store(out, out16, left, acc);
}

// grid (ceil(N * ceil(S / 4) / POOL_NT), groups of this launch): a thread owns four consecutive
// columns of one (group, draw) row of the accumulators; the (draw, quad) pairs are flattened over
// grid.x, quads fastest, so a wavefront reads runs of consecutive floats of every member.
// traj: the session's [B, N, T] trajectories, `total` = B*N*T floats; entries offsets[g] ..
// offsets[g + 1] are the members of group g; widths[g] <= S; pooled [groups, N, S] float64 holds the
// initial accumulator when has_init, and the result afterwards.
template <bool ALIGNED, int LINK = LINK_IDENTITY>
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
  if (has_init) pool_init(out, out16 && left == 4, left, acc);
  // A whole quad inside the width reads [at, at + 4) when ALIGNED: inside the member's row.
  // Otherwise it reads [a, a + 8), a = at rounded down to the 16-byte grid: up to 3 floats before the
  // quad and 4 after it.  Both ends are floats of the same buffer (the neighbouring row, draw or
  // series) except in front of the first series and behind the last.  Members ascend, and so do
  // their starts (first < T), so the first member of the group reaches lowest and the last one
  // highest: checked once per thread, and a quad that could leave [0, total) goes element by element,
  // as do the last columns of the width.
  bool vec = left == 4 && k0 < k1;
  if (!ALIGNED && vec)
    vec = (entries[k0].start + r >= 4 || base_m == 0u) && entries[k1 - 1].start + r + 8 <= total;
  pool_members<ALIGNED, LINK>(traj, entries, k0, k1, r, base_m + (unsigned)r, base_m, vec, left, acc);
  pool_store(out, out16, room, acc);
}

}  // namespace ci
