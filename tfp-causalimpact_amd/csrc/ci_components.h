// ci_components.h -- on-device summarisation of the model's COMPONENTS over the pooled draws of a
// finished session: trend, every seasonal block, the regression term, and the regression weights
// themselves (ci_session_summarize_components; DESIGN.md "Component summaries").
//
// The kernels here only BUILD: each makes the [T, N] float64 matrix of one component of every
// series of the launch (time-major, draws contiguous), the layout the select kernels of
// ci_summary.h read.  Those kernels then take the order statistics, unchanged, and
// comp_row_stats_kernel the mean (and the non-zero count) of every row.
//
//   trend[n,t]      = double(level[n,t]) * scale + shift          (two roundings, as summ_transpose_kernel)
//   seasonal_k[n,t] = double(seasonal[n,t,k]) * scale
//   regression[n,t] = (sum_j double(X[t,j]) * double(w[n,j])) * scale,  j ascending from 0.0; the
//                     products of two float32 values are exact in float64, only the additions round
//   weights[n,j]    = double(w[n,j])                              ("time" axis = the design columns)
//
// Every kernel works on 64 x 64 tiles (steps x draws) with a 64 x 4 workgroup: HBM is read along
// the contiguous axis of the source, staged in LDS (rows padded by one element: the transposed
// read is conflict-free) and written along the draws, the contiguous axis of the result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ci {

// The launches (ci_components.hip) of the three kernels below: block k of K of `in` for B series
// (scales, shifts == nullptr: none), their regression terms, the row statistics of M [rows, N].
hipError_t comp_launch_gather(hipStream_t stream, int B, int N, int T, int K, int k, const float* in,
                              const double* scales, const double* shifts, double* out);
hipError_t comp_launch_regression(hipStream_t stream, int B, int N, int T, int P, const float* Xt,
                                  const float* w, const int* series_T, const double* scales,
                                  double* out);
// ... of float64 designs and weights (a session made from float64 draws): the F = double build.
hipError_t comp_launch_regression_f64(hipStream_t stream, int B, int N, int T, int P, const double* Xt,
                                      const double* w, const int* series_T, const double* scales,
                                      double* out);
hipError_t comp_launch_row_stats(hipStream_t stream, size_t rows, int N, const double* M,
                                 double* mean, int* nonzero);

// One of the kernels is no template: a unit that includes it emits it.  The host units
// (ci_session.h) take the declarations above alone.
#ifndef CI_SEASONAL_DECL_ONLY

// [N, T, K] float32 (one series: draws x steps x interleaved blocks) -> [T, N] float64 of block k.
// K = 1 is the plain transpose (level; the weights with T = P).  A draw's 64 steps of all K blocks
// are 64 K contiguous floats: the lanes sweep them in order (every cache line is used whole) and
// keep the elements of block k.
// grid (ceil(T/64), ceil(N/64), B), block (64, 4); scales == nullptr: no scaling.
template <bool SHIFT>
__global__ __launch_bounds__(256) void comp_gather_kernel(int N, int T, int K, int k,
                                                          const float* __restrict__ in_all,
                                                          const double* __restrict__ scales,
                                                          const double* __restrict__ shifts,
                                                          double* __restrict__ out_all) {
  __shared__ double tile[64][65];
  const size_t b = blockIdx.z;
  const float* in = in_all + b * (size_t)N * T * K;
  double* out = out_all + b * (size_t)N * T;
  const double scale = scales ? scales[b] : 1.0;
  const double shift = SHIFT ? shifts[b] : 0.0;
  const int t0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int span = (T - t0 < 64 ? T - t0 : 64) * K;      // floats of one draw's row segment
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const int n = n0 + ty + 4 * i;
    if (n >= N) continue;                                // uniform over the wavefront
    const float* row = in + ((size_t)n * T + t0) * K;
    for (int e = tx; e < span; e += 64) {
      const int tt = e / K;
      if (e - tt * K != k) continue;
      double v = __dmul_rn((double)row[e], scale);
      if (SHIFT) v = __dadd_rn(v, shift);
      tile[ty + 4 * i][tt] = v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int t = t0 + ty + 4 * i, n = n0 + tx;
    if (n < N && t < T) out[(size_t)t * N + n] = tile[tx][ty + 4 * i];
  }
}

// The regression term: per series a [N, P] x [P, T] product, Xt [P, T] feature-major (rows
// contiguous over time) and w [N, P] (a tile's 64 draws are 64 P contiguous values), both of the
// input type F, widened to double where they are multiplied.  The design
// columns pass through LDS in chunks of COMP_PC: per chunk both sides are read from HBM once per
// tile, the 16 accumulators of a thread (one draw, 16 steps) stay in registers across the chunks, so
// every sum runs over j = 0..P-1 in ascending order.  In the inner loop a wavefront reads one X
// value (broadcast) and 64 weights at a stride of COMP_PC + 1 floats (conflict-free).
// series_T (or nullptr): the own length of every series of a ragged session; the term is 0 from
// there on, like every latent the session reports beyond a series' length.
// grid (ceil(T/64), ceil(N/64), B), block (64, 4).
constexpr int COMP_PC = 32;

template <class F = float>
__global__ __launch_bounds__(256) void comp_regression_kernel(int N, int T, int P,
                                                              const F* __restrict__ Xt_all,
                                                              const F* __restrict__ w_all,
                                                              const int* __restrict__ series_T,
                                                              const double* __restrict__ scales,
                                                              double* __restrict__ out_all) {
  __shared__ F Xs[COMP_PC][64];
  __shared__ F Ws[64][COMP_PC + 1];
  const size_t b = blockIdx.z;
  const F* Xt = Xt_all + b * (size_t)P * T;
  const F* w = w_all + b * (size_t)N * P;
  double* out = out_all + b * (size_t)N * T;
  const int Tb = series_T ? series_T[b] : T;
  const double scale = scales[b];
  const int t0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
  const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * 64 + tx;
  double acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0;
  for (int j0 = 0; j0 < P; j0 += COMP_PC) {
    const int pc = P - j0 < COMP_PC ? P - j0 : COMP_PC;
    for (int e = tid; e < pc * 64; e += 256) {
      const int jj = e >> 6, t = t0 + (e & 63);
      Xs[jj][e & 63] = t < Tb ? Xt[(size_t)(j0 + jj) * T + t] : (F)0;
    }
    for (int e = tid; e < pc * 64; e += 256) {
      const int n = e / pc, jj = e - n * pc;
      Ws[n][jj] = n0 + n < N ? w[(size_t)(n0 + n) * P + j0 + jj] : (F)0;
    }
    __syncthreads();
    for (int jj = 0; jj < pc; ++jj) {
      const double wv = (double)Ws[tx][jj];
#pragma unroll
      for (int i = 0; i < 16; ++i)
        acc[i] = __dadd_rn(acc[i], __dmul_rn((double)Xs[jj][ty + 4 * i], wv));
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int t = t0 + ty + 4 * i, n = n0 + tx;
    if (n < N && t < T) out[(size_t)t * N + n] = __dmul_rn(acc[i], scale);
  }
}

// Mean over the N draws of every row of M [rows, N] and, when `nonzero` is given, how many of
// them are not zero (the inclusion count of a weight).  One wavefront per row, four rows per
// workgroup; the lanes stride over the row (coalesced) and combine in a fixed order.
__global__ __launch_bounds__(256) void comp_row_stats_kernel(size_t rows, int N,
                                                             const double* __restrict__ M,
                                                             double* __restrict__ mean,
                                                             int* __restrict__ nonzero) {
  const int lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const double* x = M + row * N;
  double s = 0.0;
  int c = 0;
  for (int i = lane; i < N; i += 64) {
    const double v = x[i];
    s += v;
    c += v != 0.0 ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    s += __shfl_xor(s, off, 64);
    c += __shfl_xor(c, off, 64);
  }
  if (lane == 0) {
    mean[row] = s / (double)N;
    if (nonzero) nonzero[row] = c;
  }
}

#endif  // CI_SEASONAL_DECL_ONLY

}  // namespace ci
