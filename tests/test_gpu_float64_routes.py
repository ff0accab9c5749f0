"""Every route, batch layout and gap pattern of the float64 Gibbs kernels (csrc/ci_gibbs64.h)
against the float64 oracle, draw for draw at the tolerances of tests/test_gpu_float64.py.

`ci_fit_gibbs_f64` picks (global_ws, reg_lds) from the LDS footprint and one of two kernels from the
number of seasonal blocks: four kernel builds, each with the regression block in LDS or in the
workspace, each with a register (P <= 16), a dense (P <= 32) or a workspace (P > 32) regression
draw.  ROUTE_CASES names one shape per combination, with the missing-data pattern that stresses it,
and every case first asserts through `_native.fit_gibbs_f64_route` that it still takes the route
written next to it (tests/test_float64_route_table.py checks the same table without a GPU).
BATCH_CASES run three series with their own data, gaps and priors in ONE launch: every per-series
offset of the kernels with series != 0."""
import functools

import numpy as np
import pytest

from causalimpact import _model, _native
from causalimpact import _synthetic as syn
from oracle import ci_oracle as orc

pytestmark = pytest.mark.gpu

SEED = (7, 1)
CHAINS = 2
CHAIN_OFFSET = 3
SERIES_OFFSET = 5
WEEK = ((7, 1),)

# (T, covariates p (P = p + 1), has_slope, seasons, mask pattern, W, S, (global_ws, reg_lds), trend kernel)
ROUTE_CASES = [
    # -- trend kernel (eight wavefronts, time-parallel: thread j owns Lc = ceil(T/256)|1 steps)
    # P <= 16 register draw with X'X / Omega read from global memory; window T 2053-2064
    (2056, 4, 0, (), "run", 1, 7, (0, 0), 1),
    (1436, 4, 1, (), "scatter", 1, 7, (0, 0), 1),      # the same with a slope; window 1433-1440
    (2070, 4, 0, (), "run", 1, 7, (1, 1), 1),          # workspace, register draw; 40 wholly masked lanes at Lc = 9
    (2100, 24, 0, (), "all", 2, 6, (1, 1), 1),         # workspace, dense draw in LDS
    (1800, 31, 0, (), "all", 2, 6, (0, 0), 1),         # P = 32 dense draw in the workspace, arrays in LDS
    (1445, 36, 1, (), "scatter", 1, 7, (1, 0), 1),     # both in the workspace
    (256, 2, 1, (), "lead", 3, 17, (0, 1), 1),         # Lc = 1, all 256 pass threads
    (257, 2, 1, (), "run", 3, 17, (0, 1), 1),          # Lc = 3, 86 threads, the last one short
    (768, 0, 1, (), "longpost", 2, 10, (0, 1), 1),     # Lc = 3 exactly full, P = 0
    (769, 1, 0, (), "all", 2, 10, (0, 1), 1),          # Lc = 5
    (3, 0, 0, (), "tail", 3, 20, (0, 1), 1),           # the shortest series the ABI accepts
    (5, 1, 1, (), "tail", 3, 20, (0, 1), 1),
    # -- sequential kernel (one wavefront, any seasonal blocks)
    (750, 2, 0, WEEK, "all", 2, 8, (1, 1), 0),         # gibbs64_kernel<true>: arrays in the workspace
    (600, 31, 0, WEEK, "run", 1, 7, (0, 0), 0),        # P = 32, regression block out of LDS
    (730, 40, 1, WEEK, "scatter", 1, 7, (1, 0), 0),    # P = 41 with a slope, everything in the workspace
    (200, 40, 0, WEEK, "lead", 2, 10, (0, 0), 0),      # P > 32 with the arrays in LDS
    (140, 0, 1, WEEK, "run", 3, 17, (0, 1), 0),        # P = 0 with a block
    (520, 0, 0, ((4, 3), (7, 1)), "all", 2, 8, (1, 1), 0),   # two blocks, P = 0, workspace
    (30, 1, 0, ((63, 1),), "tail", 2, 8, (0, 1), 0),   # D = 64 in LDS (150,144 B of the 153,600 allowed)
    (40, 2, 0, ((63, 1),), "lead", 2, 8, (1, 1), 0),   # D = 64 in the workspace: kf / rs rows of T*D doubles
    (9, 0, 0, WEEK, "tail", 3, 20, (0, 1), 0),         # a series shorter than two cycles
]

# (T, p, has_slope, seasons, W, S, (global_ws, reg_lds), trend kernel): three series per launch
BATCH_CASES = [
    (120, 3, 0, (), 3, 12, (0, 1), 1),                 # trend, LDS
    (2070, 4, 1, (), 1, 5, (1, 1), 1),                 # trend, workspace: the per-chain workspace stride
    (750, 2, 0, WEEK, 1, 5, (1, 1), 0),                # seasonal, workspace
]
BATCH_MASKS = ("lead", "run", "scatter")


def route_problem(T, p, has_slope, seasons, W=0, S=1, **kw):
  """The ci_problem of a shape: p covariates and the intercept make P = p + 1 columns (none: P = 0)."""
  counts, _ = _model.expand_seasons(seasons, T)
  return _native.make_problem(T=T, P=p + 1 if p else 0, has_slope=has_slope, num_seasons=counts, num_warmup=W,
                              num_results=S, **kw)


def make_mask(T, pattern):
  """The missing-data patterns: the tail [pre, T) is always masked (the post-period)."""
  pre = int(0.7 * T)
  rng = np.random.default_rng(T)
  mask = np.zeros(T, bool)
  mask[pre:] = True
  run = slice(pre // 3, pre // 3 + max(4, pre // 4))
  if pattern == "lead":                       # init_level_loc comes from the first OBSERVED value
    mask[0:3] = True
  elif pattern == "run":                      # whole lanes of the time-parallel kernel unobserved
    mask[run] = True
  elif pattern == "scatter":
    mask[:pre] |= rng.random(pre) < 0.15
  elif pattern == "longpost":                 # only the first steps observed
    mask[max(6, T // 3):] = True
  elif pattern == "all":
    mask[0:2] = True
    mask[run] = True
    mask[:pre] |= rng.random(pre) < 0.10
  else:
    assert pattern == "tail", pattern
  return mask


def make_series(T, p, has_slope, seasons, pattern, data_seed=31, y_scale=1.0, **spec_extra):
  """(y, mask, X or None, spec): the inputs of tests/test_gpu_float64.py with a gap pattern."""
  y, _, X, _ = syn.make_sampler_inputs(T, max(p, 1), data_seed)
  X = X if p > 0 else None
  y = y_scale * (y + 0.5 * np.sin(2 * np.pi * np.arange(T) / 7.0))
  mask = make_mask(T, pattern)
  spec = orc.default_spec(y, mask, X, has_slope=bool(has_slope), seasons=seasons)
  spec.update(spec_extra)
  return y, mask, X, spec


def assert_route(pb, route, trend):
  r = _native.fit_gibbs_f64_route(pb)
  assert ((r["global_ws"], r["reg_lds"]), r["trend_kernel"]) == (tuple(route), trend), r
  assert 0 < r["lds_bytes"] <= 160 * 1024


def assert_equals_oracle(got, b, c, w, has_slope, P, K):
  """Series b, chain c of a device fit against the oracle's chain `w`: every output, every draw."""
  tol = dict(rtol=1e-8, atol=1e-9)
  path = dict(rtol=1e-8, atol=1e-8)
  np.testing.assert_allclose(got["observation_noise_scale"][b, c], w["obs_scale"], **tol)
  np.testing.assert_allclose(got["level_scale"][b, c], w["level_scale"], **tol)
  if has_slope:
    np.testing.assert_allclose(got["slope_scale"][b, c], w["slope_scale"], **tol)
    np.testing.assert_allclose(got["slope"][b, c], w["slope"], **path)
  if P:
    np.testing.assert_array_equal(got["weights"][b, c] != 0, w["weights"] != 0)
    np.testing.assert_allclose(got["weights"][b, c], w["weights"], **tol)
  if K:
    np.testing.assert_allclose(got["seasonal_drift_scales"][b, c], w["drift_scales"], **tol)
    np.testing.assert_allclose(got["seasonal_levels"][b, c], w["seasonal"], **path)
  np.testing.assert_allclose(got["level"][b, c], w["level"], **path)
  np.testing.assert_allclose(got["posterior_trajectories"][b, c], w["trajectories"], **path)
  np.testing.assert_allclose(got["posterior_means"][b, c], w["pred_mean"], **path)


@pytest.mark.parametrize("T,p,has_slope,seasons,pattern,W,S,route,trend", ROUTE_CASES)
def test_float64_route_equals_the_oracle_draw_for_draw(T, p, has_slope, seasons, pattern, W, S,
                                                       route, trend):
  y, mask, X, spec = make_series(T, p, has_slope, seasons, pattern)
  _, flg = _model.expand_seasons(seasons, T)
  pb = route_problem(T, p, has_slope, seasons, W, S, num_chains=CHAINS,
                     chain_offset=CHAIN_OFFSET, seed=SEED)
  assert pb.P == spec["P"]
  assert_route(pb, route, trend)
  got = _native.fit_gibbs_f64(pb, y[None], mask[None], None if X is None else X[None], flg,
                              _native.make_params([spec]))
  assert all(v.dtype == np.float64 for v in got.values())
  for c in range(CHAINS):
    w = orc.fit_gibbs(y, mask, X, spec, num_results=S, num_warmup=W, seed=SEED, chain=CHAIN_OFFSET + c)
    assert_equals_oracle(got, 0, c, w, has_slope, spec["P"], len(seasons))


# ---- batches: num_series = 3 in one launch
def batch_series(T, p, has_slope, seasons):
  """Three series with their own data seed, gap pattern and priors: series 1's outcome is three
  times as large (every prior of default_spec scales with it), series 2 has its own weights-prior
  multiplier."""
  out = []
  for b, pattern in enumerate(BATCH_MASKS):
    extra = dict(weights_prior_scale=2.0) if b == 2 else {}
    out.append(make_series(T, p, has_slope, seasons, pattern, data_seed=31 + b,
                           y_scale=3.0 if b == 1 else 1.0, **extra))
  return out


@functools.lru_cache(maxsize=None)
def batch_fit(case, flags=0):
  """(series, full device fit of the batch) -- computed once per shape, read by several tests."""
  T, p, has_slope, seasons, W, S, route, trend = BATCH_CASES[case]
  series = batch_series(T, p, has_slope, seasons)
  pb = route_problem(T, p, has_slope, seasons, W, S, num_chains=CHAINS, chain_offset=CHAIN_OFFSET,
                     num_series=len(series), series_offset=SERIES_OFFSET, seed=SEED, flags=flags)
  assert_route(pb, route, trend)
  got = _native.fit_gibbs_f64(pb, *batch_inputs(series, seasons, T))
  for v in got.values():
    v.setflags(write=False)
  return series, got


def batch_inputs(series, seasons, T):
  _, flg = _model.expand_seasons(seasons, T)
  X = None if series[0][2] is None else np.stack([s[2] for s in series])
  return (np.stack([s[0] for s in series]), np.stack([s[1] for s in series]), X, flg,
          _native.make_params([s[3] for s in series]))


@pytest.mark.parametrize("case", range(len(BATCH_CASES)))
def test_float64_batch_series_equal_the_oracle_on_their_own_streams(case):
  """Series b of a batch = the oracle on series b alone with the Philox key of series id 5 + b."""
  T, p, has_slope, seasons, W, S, _, _ = BATCH_CASES[case]
  series, got = batch_fit(case)
  for b, (y, mask, X, spec) in enumerate(series):
    key = _native.series_stream_key(SEED, SERIES_OFFSET + b)
    for c in range(CHAINS):
      w = orc.fit_gibbs(y, mask, X, spec, num_results=S, num_warmup=W, seed=key, chain=CHAIN_OFFSET + c)
      assert_equals_oracle(got, b, c, w, has_slope, spec["P"], len(seasons))
  for name in ("observation_noise_scale", "level", "posterior_trajectories", "weights"):
    for b in range(1, len(series)):
      assert not np.array_equal(got[name][b], got[name][0]), (name, b)
      assert not np.allclose(got[name][b], got[name][b - 1]), (name, b)


def test_float64_batch_with_shared_streams_equals_the_oracle_on_the_plain_seed():
  T, p, has_slope, seasons, W, S, _, _ = BATCH_CASES[0]
  series, got = batch_fit(0, _native.FLAG_SHARED_SERIES_STREAMS)
  for b, (y, mask, X, spec) in enumerate(series):
    for c in range(CHAINS):
      w = orc.fit_gibbs(y, mask, X, spec, num_results=S, num_warmup=W, seed=SEED, chain=CHAIN_OFFSET + c)
      assert_equals_oracle(got, b, c, w, has_slope, spec["P"], len(seasons))


@pytest.mark.parametrize("case", range(len(BATCH_CASES)))
def test_float64_batch_equals_single_series_launches_bit_for_bit(case):
  """Same kernel, same arithmetic: series b of the batch and a launch of series b alone with
  series_offset = 5 + b give the same bits."""
  T, p, has_slope, seasons, W, S, _, _ = BATCH_CASES[case]
  series, got = batch_fit(case)
  for b, one in enumerate(series):
    pb = route_problem(T, p, has_slope, seasons, W, S, num_chains=CHAINS, chain_offset=CHAIN_OFFSET,
                       series_offset=SERIES_OFFSET + b, seed=SEED)
    alone = _native.fit_gibbs_f64(pb, *batch_inputs([one], seasons, T))
    assert sorted(alone) == sorted(got)
    for name, v in alone.items():
      np.testing.assert_array_equal(v[0], got[name][b], err_msg=f"{name}, series {b}")


def test_float64_batch_want_selects_outputs_and_leaves_the_rest_out():
  T, p, has_slope, seasons, W, S, _, _ = BATCH_CASES[0]
  series, full = batch_fit(0)
  want = ("posterior_trajectories", "observation_noise_scale")
  pb = route_problem(T, p, has_slope, seasons, W, S, num_chains=CHAINS, chain_offset=CHAIN_OFFSET,
                     num_series=len(series), series_offset=SERIES_OFFSET, seed=SEED)
  got = _native.fit_gibbs_f64(pb, *batch_inputs(series, seasons, T), want=want)
  assert sorted(got) == sorted(want)
  for name in want:
    assert got[name].shape == full[name].shape
    assert np.any(got[name] != 0)
    np.testing.assert_array_equal(got[name], full[name])
