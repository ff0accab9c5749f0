"""The route table of tests/test_gpu_float64_routes.py, checked without a GPU: every case still
takes the (global_ws, reg_lds, kernel) route written next to it, the table still covers every route
of `ci_fit_gibbs_f64`, and the query refuses what the fit refuses.  A moved LDS threshold shows
here, before any GPU time is spent on a case that silently changed its route."""
import ctypes as C

import pytest

from causalimpact import _native
import test_gpu_float64_routes as routes


@pytest.mark.parametrize("T,p,has_slope,seasons,pattern,W,S,route,trend", routes.ROUTE_CASES)
def test_route_case_takes_the_route_it_names(T, p, has_slope, seasons, pattern, W, S, route, trend):
  routes.assert_route(routes.route_problem(T, p, has_slope, seasons, W, S, num_chains=routes.CHAINS,
                                           chain_offset=routes.CHAIN_OFFSET), route, trend)


@pytest.mark.parametrize("T,p,has_slope,seasons,W,S,route,trend", routes.BATCH_CASES)
def test_batch_case_takes_the_route_it_names(T, p, has_slope, seasons, W, S, route, trend):
  pb = routes.route_problem(T, p, has_slope, seasons, W, S, num_chains=routes.CHAINS, num_series=3,
                            chain_offset=routes.CHAIN_OFFSET, series_offset=routes.SERIES_OFFSET)
  routes.assert_route(pb, route, trend)


def test_route_table_covers_every_route_of_both_kernels_and_every_gap_pattern():
  seen = {(c[7], c[8]) for c in routes.ROUTE_CASES}
  assert seen == {((g, r), k) for g in (0, 1) for r in (0, 1) for k in (0, 1)}
  assert {c[4] for c in routes.ROUTE_CASES} == {"tail", "lead", "run", "scatter", "longpost", "all"}
  assert len(routes.ROUTE_CASES) >= 21 and len(routes.BATCH_CASES) >= 3
  for T, p, has_slope, seasons, pattern, W, S, _, _ in routes.ROUTE_CASES:
    assert W + S <= 30
    mask = routes.make_mask(T, pattern)
    assert mask[int(0.7 * T):].all() and not mask.all(), (T, pattern)


def test_route_windows_named_in_the_table_end_where_it_says():
  """The two narrow (0, 0) windows of the register draw: one step outside them is another route."""
  def route(T, p, slope):
    r = _native.fit_gibbs_f64_route(routes.route_problem(T, p, slope, ()))
    return (r["global_ws"], r["reg_lds"])
  assert [route(T, 4, 0) for T in (2052, 2053, 2064, 2065)] == [(0, 1), (0, 0), (0, 0), (1, 1)]
  assert [route(T, 4, 1) for T in (1432, 1433, 1440, 1441)] == [(0, 1), (0, 0), (0, 0), (1, 1)]


def test_route_query_validates_as_the_fit_does():
  L = _native.load()
  out = (C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64())
  refs = [C.byref(v) for v in out]
  with pytest.raises(_native.NativeError, match="T must be >= 3"):
    _native.fit_gibbs_f64_route(routes.route_problem(2, 0, 0, ()))
  with pytest.raises(_native.NativeError, match="too wide for one wavefront: 65 > 64"):
    _native.fit_gibbs_f64_route(routes.route_problem(200, 0, 0, ((64, 1),)))
  # (the LDS limit behind it is a backstop no accepted shape reaches: the widest state beside the
  # widest design stays under it, with the launch size the query reports)
  r = _native.fit_gibbs_f64_route(routes.route_problem(200, 511, 0, ((63, 1),)))
  assert (r["global_ws"], r["reg_lds"], r["trend_kernel"]) == (1, 0, 0) and r["lds_bytes"] < 160 * 1024
  pb = routes.route_problem(200, 2, 0, ())
  pb.abi_version = 999
  with pytest.raises(_native.NativeError, match="ABI mismatch"):
    _native.fit_gibbs_f64_route(pb)
  pb = routes.route_problem(200, 2, 0, ())
  assert L.ci_fit_gibbs_f64_route(C.byref(pb), None, refs[1], refs[2], refs[3]) != 0
  assert b"NULL argument" in L.ci_last_error()
  assert L.ci_fit_gibbs_f64_route(None, *refs) != 0
  assert b"problem is NULL" in L.ci_last_error()
  assert L.ci_fit_gibbs_f64_route(C.byref(pb), *refs) == 0
  assert (out[0].value, out[1].value, out[2].value) == (0, 1, 1) and out[3].value > 0
