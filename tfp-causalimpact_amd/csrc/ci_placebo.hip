// Instantiation unit of the placebo forecasts (ci_placebo.h) and their launch;
// ci_session_summarize_placebo (ci_summary.hip) calls it.
#include "ci_placebo.h"

namespace ci {

using PlaceboFn = void (*)(PlaceboArgs);

template <int HAS_SLOPE, int NS> static PlaceboFn placebo_fn(int out) {
  if (out == PLACEBO_SUM) return placebo_kernel<HAS_SLOPE, NS, PLACEBO_SUM>;
  if (out == PLACEBO_SPREAD) return placebo_kernel<HAS_SLOPE, NS, PLACEBO_SPREAD>;
  return placebo_kernel<HAS_SLOPE, NS, PLACEBO_PIT>;
}

template <int HAS_SLOPE> static PlaceboFn placebo_fn(int ns, int out) {
  switch (ns) {
    case 0: return placebo_fn<HAS_SLOPE, 0>(out);
    case 2: return placebo_fn<HAS_SLOPE, 2>(out);
    case 3: return placebo_fn<HAS_SLOPE, 3>(out);
    case 4: return placebo_fn<HAS_SLOPE, 4>(out);
    case 5: return placebo_fn<HAS_SLOPE, 5>(out);
    case 6: return placebo_fn<HAS_SLOPE, 6>(out);
    case 7: return placebo_fn<HAS_SLOPE, 7>(out);
    default: return nullptr;
  }
}

// One pass over B series: `out` one of PlaceboOut, num_seasons 0 (no block) or 2..7.
hipError_t placebo_launch(hipStream_t stream, int B, int has_slope, int num_seasons, int out,
                          const PlaceboArgs& args) {
  const PlaceboFn fn = has_slope ? placebo_fn<1>(num_seasons, out) : placebo_fn<0>(num_seasons, out);
  if (!fn) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fn, dim3((args.p.N + 63) / 64, B), dim3(64), 0, stream, args);
  return hipGetLastError();
}

}  // namespace ci
