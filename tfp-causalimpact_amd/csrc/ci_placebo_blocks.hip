// Instantiation unit of the block-model placebo forecasts (ci_placebo_blocks.h) and their launch;
// ci_session_summarize_placebo_blocks (ci_summary.hip) calls it.
#include "ci_placebo_blocks.h"

namespace ci {

using PlaceboBlocksFn = void (*)(PlaceboBlocksArgs);

template <int G> static PlaceboBlocksFn placebo_blocks_fn(int out) {
  if (out == PLACEBO_SUM) return placebo_blocks_kernel<G, PLACEBO_SUM>;
  if (out == PLACEBO_SPREAD) return placebo_blocks_kernel<G, PLACEBO_SPREAD>;
  if (out == PLACEBO_VAR) return placebo_blocks_kernel<G, PLACEBO_VAR>;
  return placebo_blocks_kernel<G, PLACEBO_PIT>;
}

int blocks_group_size(int d);      // ci_predict_blocks.hip

// One pass over B series: `out` one of PlaceboOut, args.m.d <= 64.
hipError_t placebo_blocks_launch(hipStream_t stream, int B, int out, const PlaceboBlocksArgs& args) {
  if (args.m.d < 1 || args.m.d > PB_MAX_STATE) return hipErrorInvalidValue;
  const int G = blocks_group_size(args.m.d);
  const PlaceboBlocksFn fn = G == 8 ? placebo_blocks_fn<8>(out) : G == 16 ? placebo_blocks_fn<16>(out)
                           : G == 32 ? placebo_blocks_fn<32>(out) : placebo_blocks_fn<64>(out);
  const int fpw = 64 / G;
  hipLaunchKernelGGL(fn, dim3((args.q.p.N + fpw - 1) / fpw, B), dim3(64), 0, stream, args);
  return hipGetLastError();
}

}  // namespace ci
