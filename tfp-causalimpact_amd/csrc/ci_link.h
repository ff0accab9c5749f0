// ci_link.h -- the outcome link of the on-device summaries (ci_session_set_link): the model of a
// multiplicative outcome is fitted to log y (or log1p y), and every summary is wanted on the data
// scale.  E[exp z] != exp E[z], so the link is applied draw by draw where a first-pass kernel forms
//   z = (double)trajectory * scale + shift                  (two roundings, no FMA)
//   value = link(z)
// and everything downstream -- running sums, order statistics, per-draw totals, excursions, pooled
// sums -- reads `value` as before.  LINK is a template parameter of those kernels
// (summ_transpose_kernel, window_totals_kernel, path_values_kernel, pool_kernel, pool_event_kernel):
// the identity instantiation contains no trace of the others.
#pragma once
#include <hip/hip_runtime.h>

namespace ci {

constexpr int LINK_IDENTITY = 0;   // == CI_LINK_IDENTITY
constexpr int LINK_LOG = 1;        // == CI_LINK_LOG:   value = exp(z)
constexpr int LINK_LOG1P = 2;      // == CI_LINK_LOG1P: value = expm1(z)
constexpr int NUM_LINKS = 3;

// The float64 device functions; no clamp: an overflow is +inf, as numpy's.
template <int LINK>
__device__ __forceinline__ double link_value(double z) {
  if constexpr (LINK == LINK_LOG) return exp(z);
  else if constexpr (LINK == LINK_LOG1P) return expm1(z);
  else return z;
}

}  // namespace ci
