// Instantiation unit of the block-model placebo forecasts (ci_placebo_blocks.h) and their launch;
// ci_session_summarize_placebo_blocks, ci_session_pool_placebo[_horizons]_blocks, ci_session_simulate_placebo_blocks and
// ci_session_pool_simulated_placebo_blocks (ci_forecast.hip) call them.  With -DCI_FILTER_F64: the
// float64-input builds and the launches with the suffix _f64.
#include "ci_placebo_blocks.h"

namespace ci {

using PlaceboBlocksFn = void (*)(PlaceboBlocksArgs);

template <int G> static PlaceboBlocksFn placebo_blocks_fn(int out) {
  if (out == PLACEBO_SUM) return placebo_blocks_kernel<G, PLACEBO_SUM, PlaceboBlocksArgs, CI_FILTER_F>;
  if (out == PLACEBO_SPREAD) return placebo_blocks_kernel<G, PLACEBO_SPREAD, PlaceboBlocksArgs, CI_FILTER_F>;
  if (out == PLACEBO_VAR) return placebo_blocks_kernel<G, PLACEBO_VAR, PlaceboBlocksArgs, CI_FILTER_F>;
  return placebo_blocks_kernel<G, PLACEBO_PIT, PlaceboBlocksArgs, CI_FILTER_F>;
}

int blocks_group_size(int d);      // ci_predict_blocks.hip

// One pass over B series: `out` one of PlaceboOut, args.m.d <= 64.
hipError_t CI_FILTER_NAME(placebo_blocks_launch)(hipStream_t stream, int B, int out, const PlaceboBlocksArgs& args) {
  if (args.m.d < 1 || args.m.d > PB_MAX_STATE) return hipErrorInvalidValue;
  const int G = blocks_group_size(args.m.d);
  const PlaceboBlocksFn fn = G == 8 ? placebo_blocks_fn<8>(out) : G == 16 ? placebo_blocks_fn<16>(out)
                           : G == 32 ? placebo_blocks_fn<32>(out) : placebo_blocks_fn<64>(out);
  const int fpw = 64 / G;
  hipLaunchKernelGGL(fn, dim3((args.q.p.N + fpw - 1) / fpw, B), dim3(64), 0, stream, args);
  return hipGetLastError();
}

// One pass over E entries of a group table: SUM into args.q.p.out, VAR into args.var, args.m.d <= 64.
hipError_t CI_FILTER_NAME(placebo_blocks_pool_launch)(hipStream_t stream, int E, const PlaceboBlocksPoolArgs& args) {
  if (args.m.d < 1 || args.m.d > PB_MAX_STATE || !args.q.series_of || !args.var) return hipErrorInvalidValue;
  const int G = blocks_group_size(args.m.d);
  void (*fn)(PlaceboBlocksPoolArgs) = G == 8 ? placebo_blocks_kernel<8, PLACEBO_SUM_VAR, PlaceboBlocksPoolArgs, CI_FILTER_F>
                                    : G == 16 ? placebo_blocks_kernel<16, PLACEBO_SUM_VAR, PlaceboBlocksPoolArgs, CI_FILTER_F>
                                    : G == 32 ? placebo_blocks_kernel<32, PLACEBO_SUM_VAR, PlaceboBlocksPoolArgs, CI_FILTER_F>
                                    : placebo_blocks_kernel<64, PLACEBO_SUM_VAR, PlaceboBlocksPoolArgs, CI_FILTER_F>;
  const int fpw = 64 / G;
  hipLaunchKernelGGL(fn, dim3((args.q.p.N + fpw - 1) / fpw, E), dim3(64), 0, stream, args);
  return hipGetLastError();
}

// One pass over E entries of a group table at the K checkpoints of every entry's horizon row: SUM into
// args.q.p.out, VAR into args.var, [E, O, K, N] each; args.m.d <= 64.
hipError_t CI_FILTER_NAME(placebo_blocks_pool_horizons_launch)(hipStream_t stream, int E,
                                                               const PlaceboBlocksPoolHorizonsArgs& args) {
  if (args.m.d < 1 || args.m.d > PB_MAX_STATE || !args.q.series_of || !args.var || !args.horizons || args.K < 1 ||
      E < 1 || E > 65535)
    return hipErrorInvalidValue;
  const int G = blocks_group_size(args.m.d);
  void (*fn)(PlaceboBlocksPoolHorizonsArgs) =
      G == 8 ? placebo_blocks_kernel<8, PLACEBO_SUM_VAR_HORIZONS, PlaceboBlocksPoolHorizonsArgs, CI_FILTER_F>
      : G == 16 ? placebo_blocks_kernel<16, PLACEBO_SUM_VAR_HORIZONS, PlaceboBlocksPoolHorizonsArgs, CI_FILTER_F>
      : G == 32 ? placebo_blocks_kernel<32, PLACEBO_SUM_VAR_HORIZONS, PlaceboBlocksPoolHorizonsArgs, CI_FILTER_F>
                : placebo_blocks_kernel<64, PLACEBO_SUM_VAR_HORIZONS, PlaceboBlocksPoolHorizonsArgs, CI_FILTER_F>;
  const int fpw = 64 / G;
  hipLaunchKernelGGL(fn, dim3((args.q.p.N + fpw - 1) / fpw, E), dim3(64), 0, stream, args);
  return hipGetLastError();
}

using PlaceboBlocksSimFn = void (*)(PlaceboBlocksSimArgs);

template <int G> static PlaceboBlocksSimFn placebo_blocks_sim_fn(int link) {
  if (link == LINK_LOG) return placebo_blocks_sim_kernel<G, LINK_LOG, false, CI_FILTER_F>;
  if (link == LINK_LOG1P) return placebo_blocks_sim_kernel<G, LINK_LOG1P, false, CI_FILTER_F>;
  return placebo_blocks_sim_kernel<G, LINK_IDENTITY, false, CI_FILTER_F>;
}

// The simulated totals of `nb` series from args.s.b0 on (placebo_sim_launch's for the block models).
hipError_t CI_FILTER_NAME(placebo_blocks_sim_launch)(hipStream_t stream, int nb, int link, const PlaceboBlocksSimArgs& args) {
  if (args.m.d < 1 || args.m.d > PB_MAX_STATE || link < 0 || link >= NUM_LINKS) return hipErrorInvalidValue;
  const int G = blocks_group_size(args.m.d);
  const PlaceboBlocksSimFn fn = G == 8 ? placebo_blocks_sim_fn<8>(link) : G == 16 ? placebo_blocks_sim_fn<16>(link)
                              : G == 32 ? placebo_blocks_sim_fn<32>(link) : placebo_blocks_sim_fn<64>(link);
  const int fpw = 64 / G;
  hipLaunchKernelGGL(fn, dim3((args.s.q.p.N + fpw - 1) / fpw, nb), dim3(64), 0, stream, args);
  return hipGetLastError();
}

template <int G> static PlaceboBlocksSimFn placebo_blocks_sim_entries_fn(int link) {
  if (link == LINK_LOG) return placebo_blocks_sim_kernel<G, LINK_LOG, true, CI_FILTER_F>;
  if (link == LINK_LOG1P) return placebo_blocks_sim_kernel<G, LINK_LOG1P, true, CI_FILTER_F>;
  return placebo_blocks_sim_kernel<G, LINK_IDENTITY, true, CI_FILTER_F>;
}

// The simulated totals of E entries of a group table (placebo_sim_entries_launch's for the block models).
hipError_t CI_FILTER_NAME(placebo_blocks_sim_entries_launch)(hipStream_t stream, int E, int link, const PlaceboBlocksSimArgs& args) {
  if (args.m.d < 1 || args.m.d > PB_MAX_STATE || link < 0 || link >= NUM_LINKS || !args.s.q.series_of)
    return hipErrorInvalidValue;
  const int G = blocks_group_size(args.m.d);
  const PlaceboBlocksSimFn fn = G == 8 ? placebo_blocks_sim_entries_fn<8>(link)
                              : G == 16 ? placebo_blocks_sim_entries_fn<16>(link)
                              : G == 32 ? placebo_blocks_sim_entries_fn<32>(link)
                                        : placebo_blocks_sim_entries_fn<64>(link);
  const int fpw = 64 / G;
  hipLaunchKernelGGL(fn, dim3((args.s.q.p.N + fpw - 1) / fpw, E), dim3(64), 0, stream, args);
  return hipGetLastError();
}

}  // namespace ci
