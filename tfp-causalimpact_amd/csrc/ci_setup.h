// ci_setup.h -- the regression set-up kernel of the Gibbs fits (float32 session, float64 fit).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ci {
// ------------------------------------------------------------------------------------
// setup: X~'X~ (observed rows) and the weights-prior precision (all rows), float64.
// causalimpact_lib.py:451-453; SpikeSlabSampler.__init__ (design rows at missing steps = 0).
// One workgroup per series; thread (i, j) streams over T (coalesced over the
// feature-major copy).
// ------------------------------------------------------------------------------------
template <class XT>
static __global__ void setup_regression_kernel(int TS, int P, const XT* Xt, const uint8_t* mask,
                                        const double* __restrict__ prior_scale, double* xtx,
                                        double* omega, const int* __restrict__ series_T = nullptr) {
  // one wavefront per (series, i, j): lanes stride over time (both rows coalesced), float64 sums.
  // TS is the row stride; a ragged session gives every series its own number of rows T <= TS
  // (series_T) and rows [T, TS) are not read.
  const int e = blockIdx.x % (P * P), series = blockIdx.x / (P * P);
  const int i = e / P, j = e % P, lane = threadIdx.x;
  const int T = series_T ? series_T[series] : TS;
  const XT* xi = Xt + ((size_t)series * P + i) * TS;
  const XT* xj = Xt + ((size_t)series * P + j) * TS;
  const uint8_t* m = mask + (size_t)series * TS;
  double so = 0.0, sa = 0.0;
  for (int t = lane; t < T; t += 64) {
    const double v = (double)xi[t] * (double)xj[t];
    sa += v;
    if (!m[t]) so += v;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    so += __shfl_xor(so, off, 64);
    sa += __shfl_xor(sa, off, 64);
  }
  if (lane == 0) {
    xtx[(size_t)series * P * P + e] = so;
    omega[(size_t)series * P * P + e] =
        0.01 * (i == j ? sa : 0.5 * sa) / (double)T * prior_scale[series];
  }
}

}  // namespace ci
