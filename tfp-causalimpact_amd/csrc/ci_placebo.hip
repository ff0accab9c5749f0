// Instantiation unit of the placebo forecasts (ci_placebo.h) and their launches;
// ci_session_summarize_placebo[_horizons], ci_session_pool_placebo[_horizons], ci_session_simulate_placebo and
// ci_session_pool_simulated_placebo (ci_forecast.hip) call them.  With -DCI_FILTER_F64: the float64-input
// builds of the two filters and their launches with the suffix _f64; the kernels over accumulators and
// totals read no input of a session and belong to the float32 build alone.
#include "ci_placebo.h"

namespace ci {

using PlaceboFn = void (*)(PlaceboArgs);

template <int HAS_SLOPE, int NS> static PlaceboFn placebo_fn(int out) {
  if (out == PLACEBO_SUM) return placebo_kernel<HAS_SLOPE, NS, PLACEBO_SUM, CI_FILTER_F>;
  if (out == PLACEBO_SPREAD) return placebo_kernel<HAS_SLOPE, NS, PLACEBO_SPREAD, CI_FILTER_F>;
  if (out == PLACEBO_VAR) return placebo_kernel<HAS_SLOPE, NS, PLACEBO_VAR, CI_FILTER_F>;
  return placebo_kernel<HAS_SLOPE, NS, PLACEBO_PIT, CI_FILTER_F>;
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

// One pass over B series (with args.series_of: B entries): `out` one of PlaceboOut, num_seasons 0
// (no block) or 2..7.
hipError_t CI_FILTER_NAME(placebo_launch)(hipStream_t stream, int B, int has_slope, int num_seasons, int out,
                          const PlaceboArgs& args) {
  const PlaceboFn fn = has_slope ? placebo_fn<1>(num_seasons, out) : placebo_fn<0>(num_seasons, out);
  if (!fn) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fn, dim3((args.p.N + 63) / 64, B), dim3(64), 0, stream, args);
  return hipGetLastError();
}

using PlaceboSimFn = void (*)(PlaceboSimArgs);

template <int HAS_SLOPE, int NS> static PlaceboSimFn placebo_sim_fn(int link) {
  if (link == LINK_LOG) return placebo_sim_kernel<HAS_SLOPE, NS, LINK_LOG, false, CI_FILTER_F>;
  if (link == LINK_LOG1P) return placebo_sim_kernel<HAS_SLOPE, NS, LINK_LOG1P, false, CI_FILTER_F>;
  return placebo_sim_kernel<HAS_SLOPE, NS, LINK_IDENTITY, false, CI_FILTER_F>;
}

template <int HAS_SLOPE> static PlaceboSimFn placebo_sim_fn(int ns, int link) {
  switch (ns) {
    case 0: return placebo_sim_fn<HAS_SLOPE, 0>(link);
    case 2: return placebo_sim_fn<HAS_SLOPE, 2>(link);
    case 3: return placebo_sim_fn<HAS_SLOPE, 3>(link);
    case 4: return placebo_sim_fn<HAS_SLOPE, 4>(link);
    case 5: return placebo_sim_fn<HAS_SLOPE, 5>(link);
    case 6: return placebo_sim_fn<HAS_SLOPE, 6>(link);
    case 7: return placebo_sim_fn<HAS_SLOPE, 7>(link);
    default: return nullptr;
  }
}

// The simulated totals of `nb` series from args.b0 on: rows [nb * O, N] in args.q.p.out, cnt per row
// in args.counted; link one of ci_link.h, num_seasons 0 (no block) or 2..7.
hipError_t CI_FILTER_NAME(placebo_sim_launch)(hipStream_t stream, int nb, int has_slope, int num_seasons, int link,
                              const PlaceboSimArgs& args) {
  const PlaceboSimFn fn = has_slope ? placebo_sim_fn<1>(num_seasons, link) : placebo_sim_fn<0>(num_seasons, link);
  if (!fn || link < 0 || link >= NUM_LINKS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fn, dim3((args.q.p.N + 63) / 64, nb), dim3(64), 0, stream, args);
  return hipGetLastError();
}

template <int HAS_SLOPE, int NS> static PlaceboSimFn placebo_sim_entries_fn(int link) {
  if (link == LINK_LOG) return placebo_sim_kernel<HAS_SLOPE, NS, LINK_LOG, true, CI_FILTER_F>;
  if (link == LINK_LOG1P) return placebo_sim_kernel<HAS_SLOPE, NS, LINK_LOG1P, true, CI_FILTER_F>;
  return placebo_sim_kernel<HAS_SLOPE, NS, LINK_IDENTITY, true, CI_FILTER_F>;
}

template <int HAS_SLOPE> static PlaceboSimFn placebo_sim_entries_fn(int ns, int link) {
  switch (ns) {
    case 0: return placebo_sim_entries_fn<HAS_SLOPE, 0>(link);
    case 2: return placebo_sim_entries_fn<HAS_SLOPE, 2>(link);
    case 3: return placebo_sim_entries_fn<HAS_SLOPE, 3>(link);
    case 4: return placebo_sim_entries_fn<HAS_SLOPE, 4>(link);
    case 5: return placebo_sim_entries_fn<HAS_SLOPE, 5>(link);
    case 6: return placebo_sim_entries_fn<HAS_SLOPE, 6>(link);
    case 7: return placebo_sim_entries_fn<HAS_SLOPE, 7>(link);
    default: return nullptr;
  }
}

// The simulated totals of E entries of a group table (args.q.series_of, origins and horizon from the
// launch's first entry on): rows [E * O, N] in args.q.p.out, cnt per row in args.counted.
hipError_t CI_FILTER_NAME(placebo_sim_entries_launch)(hipStream_t stream, int E, int has_slope, int num_seasons, int link,
                                      const PlaceboSimArgs& args) {
  const PlaceboSimFn fn = has_slope ? placebo_sim_entries_fn<1>(num_seasons, link)
                                    : placebo_sim_entries_fn<0>(num_seasons, link);
  if (!fn || link < 0 || link >= NUM_LINKS || !args.q.series_of) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fn, dim3((args.q.p.N + 63) / 64, E), dim3(64), 0, stream, args);
  return hipGetLastError();
}

using PlaceboHorizonsFn = void (*)(PlaceboHorizonsArgs);

template <int HAS_SLOPE> static PlaceboHorizonsFn placebo_horizons_fn(int ns) {
  switch (ns) {
    case 0: return placebo_horizons_kernel<HAS_SLOPE, 0, CI_FILTER_F>;
    case 2: return placebo_horizons_kernel<HAS_SLOPE, 2, CI_FILTER_F>;
    case 3: return placebo_horizons_kernel<HAS_SLOPE, 3, CI_FILTER_F>;
    case 4: return placebo_horizons_kernel<HAS_SLOPE, 4, CI_FILTER_F>;
    case 5: return placebo_horizons_kernel<HAS_SLOPE, 5, CI_FILTER_F>;
    case 6: return placebo_horizons_kernel<HAS_SLOPE, 6, CI_FILTER_F>;
    case 7: return placebo_horizons_kernel<HAS_SLOPE, 7, CI_FILTER_F>;
    default: return nullptr;
  }
}

// The three planes [nb * O * K, N] each of `nb` series from args.b0 on in args.p.out, one filter pass;
// num_seasons 0 (no block) or 2..7.
hipError_t CI_FILTER_NAME(placebo_horizons_launch)(hipStream_t stream, int nb, int has_slope, int num_seasons,
                                   const PlaceboHorizonsArgs& args) {
  const PlaceboHorizonsFn fn = has_slope ? placebo_horizons_fn<1>(num_seasons) : placebo_horizons_fn<0>(num_seasons);
  if (!fn || nb < 1 || nb > 65535 || args.O < 1 || args.K < 1 || args.rows != (size_t)nb * args.O * args.K)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(fn, dim3((args.p.N + 63) / 64, nb), dim3(64), 0, stream, args);
  return hipGetLastError();
}

using PlaceboPoolHorizonsFn = void (*)(PlaceboPoolHorizonsArgs);

template <int HAS_SLOPE> static PlaceboPoolHorizonsFn placebo_pool_horizons_fn(int ns) {
  switch (ns) {
    case 0: return placebo_pool_horizons_kernel<HAS_SLOPE, 0, CI_FILTER_F>;
    case 2: return placebo_pool_horizons_kernel<HAS_SLOPE, 2, CI_FILTER_F>;
    case 3: return placebo_pool_horizons_kernel<HAS_SLOPE, 3, CI_FILTER_F>;
    case 4: return placebo_pool_horizons_kernel<HAS_SLOPE, 4, CI_FILTER_F>;
    case 5: return placebo_pool_horizons_kernel<HAS_SLOPE, 5, CI_FILTER_F>;
    case 6: return placebo_pool_horizons_kernel<HAS_SLOPE, 6, CI_FILTER_F>;
    case 7: return placebo_pool_horizons_kernel<HAS_SLOPE, 7, CI_FILTER_F>;
    default: return nullptr;
  }
}

// The two planes [E * O * K, N] each of E entries of a group table (args.series_of, origins and
// horizons from the launch's first entry on) in args.p.out, one filter pass; num_seasons 0 or 2..7.
hipError_t CI_FILTER_NAME(placebo_pool_horizons_launch)(hipStream_t stream, int E, int has_slope, int num_seasons,
                                        const PlaceboPoolHorizonsArgs& args) {
  const PlaceboPoolHorizonsFn fn = has_slope ? placebo_pool_horizons_fn<1>(num_seasons)
                                             : placebo_pool_horizons_fn<0>(num_seasons);
  if (!fn || E < 1 || E > 65535 || args.O < 1 || args.K < 1 || !args.series_of ||
      args.rows != (size_t)E * args.O * args.K)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(fn, dim3((args.p.N + 63) / 64, E), dim3(64), 0, stream, args);
  return hipGetLastError();
}

#ifndef CI_FILTER_F64
// The rows [(c1 - c0) * O, N] of one pass of simulated totals added to acc [G, O, N].
hipError_t placebo_pool_totals_launch(hipStream_t stream, int N, int O, int G, int c0, int c1,
                                      const int* offsets, const double* weights, const double* M, double* acc) {
  const size_t rows = (size_t)G * O;
  const dim3 grid((N + 63) / 64, (unsigned)(rows < 65535 ? rows : 65535)), block(64);
  hipLaunchKernelGGL((placebo_pool_kernel<0, 1>), grid, block, 0, stream, N, O, rows, c0, c1, offsets, weights, M, acc);
  return hipGetLastError();
}

// below[row] and, with `rewrite`, the rows of M [rows, N] as (x - seen)^2 in place.
hipError_t placebo_sim_seen_launch(hipStream_t stream, size_t rows, int N, double* M, const double* seen,
                                   const int* counted, double* below, int rewrite) {
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  if (rewrite) hipLaunchKernelGGL(placebo_sim_seen_kernel<1>, grid, block, 0, stream, rows, N, M, seen, counted, below);
  else hipLaunchKernelGGL(placebo_sim_seen_kernel<0>, grid, block, 0, stream, rows, N, M, seen, counted, below);
  return hipGetLastError();
}

// The rows [(c1 - c0) * O, N] of one pass (which: 0 SUM, 1 VAR) added to acc [G, O, 2, N].
hipError_t placebo_pool_launch(hipStream_t stream, int N, int O, int G, int which, int c0, int c1,
                               const int* offsets, const double* weights, const double* M, double* acc) {
  const size_t rows = (size_t)G * O;
  const dim3 grid((N + 63) / 64, (unsigned)(rows < 65535 ? rows : 65535)), block(64);
  if (which)
    hipLaunchKernelGGL(placebo_pool_kernel<1>, grid, block, 0, stream, N, O, rows, c0, c1, offsets, weights, M, acc);
  else
    hipLaunchKernelGGL(placebo_pool_kernel<0>, grid, block, 0, stream, N, O, rows, c0, c1, offsets, weights, M, acc);
  return hipGetLastError();
}

// The matrix `out` (PLACEBO_SUM, PLACEBO_SPREAD, PLACEBO_PIT) of the rows r0 .. r0 + rows - 1 of acc.
hipError_t placebo_finish_launch(hipStream_t stream, int N, size_t r0, size_t rows, int out,
                                 const double* acc, const double* seen, double* M) {
  const dim3 grid((N + 63) / 64, (unsigned)(rows < 65535 ? rows : 65535)), block(64);
  if (out == PLACEBO_SUM)
    hipLaunchKernelGGL(placebo_finish_kernel<PLACEBO_SUM>, grid, block, 0, stream, N, r0, rows, acc, seen, M);
  else if (out == PLACEBO_SPREAD)
    hipLaunchKernelGGL(placebo_finish_kernel<PLACEBO_SPREAD>, grid, block, 0, stream, N, r0, rows, acc, seen, M);
  else if (out == PLACEBO_PIT)
    hipLaunchKernelGGL(placebo_finish_kernel<PLACEBO_PIT>, grid, block, 0, stream, N, r0, rows, acc, seen, M);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}
#endif  // CI_FILTER_F64

}  // namespace ci
