"""Aggregates of a batch on the device: ci_session_pool_trajectories / ci_ll_session_pool_trajectories
(csrc/ci_pool.h) against the numpy loop of their definition, the running sum chained over sessions,
and `fit_causalimpact_batch(aggregates=...)` against the host arithmetic on numpy-pooled draws.

Shapes: 5 series, 47 model steps (32 pre-period, 11 in the window, 4 after it), one covariate,
3 chains x 27 draws -- N*T = 81 * 47 is odd, so every odd series starts off the 16-byte grid of the
vector loads and the slice ends in a partial quad -- and one NaN in one series' post-period."""
import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _native
from causalimpact import batch
from causalimpact import causalimpact_lib as lib
from causalimpact import data as cid

pytestmark = pytest.mark.gpu

B, T, CHAINS, DRAWS = 5, 47, 3, 27
N = CHAINS * DRAWS
PRE, POST = (0, 31), (32, 42)
ALPHA, SEED = 0.05, (5, 11)
NAN_SERIES, NAN_STEP = 3, 38
NAMES = ["north", "south", "east", "west", "centre"]
AGGREGATES = {"total": "all", "mix": {"north": 0.5, "west": -2.0}, "one": ["east"],
              "left": {"south": 1.0, "east": 0.25, "west": 1.0},
              "right": {"east": 1.0, "west": 3.0, "centre": 1.0}}
# the same groups by position in the batch
GROUPS = [{0: 1.0, 1: 1.0, 2: 1.0, 3: 1.0, 4: 1.0}, {0: 0.5, 3: -2.0}, {2: 1.0},
          {1: 1.0, 2: 0.25, 3: 1.0}, {2: 1.0, 3: 3.0, 4: 1.0}]


def _values(num_series=B, seed=0):
  rng = np.random.default_rng(seed)
  x = rng.normal(size=(num_series, T, 1))
  y = (1.5 * x[:, :, 0] + 10.0 + 3.0 * np.arange(num_series)[:, None]
       + np.cumsum(0.1 * rng.normal(size=(num_series, T)), axis=1) + 0.3 * rng.normal(size=(num_series, T)))
  y[:, 32:43] += 1.0
  v = np.concatenate([y[:, :, None], x], axis=2)
  if num_series > NAN_SERIES:
    v[NAN_SERIES, NAN_STEP, 0] = np.nan
  return v


def _options(**kw):
  return ci.InferenceOptions(num_results=DRAWS, num_chains=CHAINS, num_warmup_steps=10, **kw)


def _pool_loop(traj, scale, shift, groups, init=None):
  """The definition: per group, over the members ascending, acc = acc + w * (traj * scale + shift),
  every operation rounded on its own in float64."""
  out = np.zeros((len(groups),) + traj.shape[1:]) if init is None else init.copy()
  for g, group in enumerate(groups):
    for b in sorted(group):
      value = traj[b].astype(np.float64) * np.float64(scale[b]) + np.float64(shift[b])
      out[g] = out[g] + np.float64(group[b]) * value
  return out


def _assert_frames_equal(a: pd.DataFrame, b: pd.DataFrame, rtol=1e-10):
  """The comparison of tests/test_gpu_summary.py for device against host frames."""
  assert list(a.columns) == list(b.columns) and list(a.index) == list(b.index)
  for c in a.columns:
    if a[c].dtype.kind in "fc":
      np.testing.assert_allclose(a[c].to_numpy(float), b[c].to_numpy(float), rtol=rtol,
                                 atol=1e-12, equal_nan=True, err_msg=str(c))
    else:
      assert (a[c] == b[c]).all(), c


def _assert_frames_identical(a: pd.DataFrame, b: pd.DataFrame):
  """Every numeric column array_equal (NaN == NaN, -0.0 == 0.0), every other column equal."""
  assert list(a.columns) == list(b.columns) and list(a.index) == list(b.index)
  for c in a.columns:
    if a[c].dtype.kind in "fc":
      np.testing.assert_array_equal(a[c].to_numpy(float), b[c].to_numpy(float), err_msg=str(c))
    else:
      assert (a[c] == b[c]).all(), c


class _Fitted:
  """The batch as `fit_causalimpact_batch` prepares it, and sessions over runs of its positions."""

  def __init__(self):
    self.values = _values()
    self.prep = batch.prepare_batch(self.values, pd.RangeIndex(T), PRE, POST)
    y = batch._sampler_outcome(self.prep, ci.DataOptions())
    pre_sd = np.nanstd(y[:, :self.prep.num_pre], axis=1, ddof=1)
    self.fit = batch._new_fit(self.prep, y, np.full(B, T), pre_sd, ALPHA, SEED, ci.ModelOptions(),
                              _options(), False)

  def session(self, ids):
    """The ordinary session of `batch._run_launch` over consecutive positions, not yet run."""
    f, ids = self.fit, np.asarray(ids)
    pb = _native.make_problem(T=T, P=f.design.shape[2], has_slope=False, num_warmup=10, num_results=DRAWS,
                              num_chains=CHAINS, num_series=len(ids), seed=f.seed, device=0,
                              series_offset=int(ids[0]))
    return _native.Session(pb, f.y[ids], f.mask[ids], f.design[ids], None,
                           _native.make_params([f.params[b] for b in ids]))


@pytest.fixture(scope="module")
def fitted():
  return _Fitted()


@pytest.fixture(scope="module")
def whole(fitted):
  """One session of all five series: (trajectories [B, N, T] float32, pooled without init, pooled with
  a non-zero init, the init, the session's summary)."""
  f = fitted.fit
  sess = fitted.session(range(B))
  try:
    sess.run()
    traj = sess.fetch(["posterior_trajectories"])["posterior_trajectories"].reshape(B, N, T)
    init = np.random.default_rng(7).normal(size=(len(GROUPS), N, T)) * 50.0
    plain = sess.pool_trajectories(f.scale, f.shift, GROUPS)
    continued = sess.pool_trajectories(f.scale, f.shift, GROUPS, init)
    dsum = sess.summarize(f.scale, f.shift, f.observed, f.flags, f.ranks)
  finally:
    sess.close()
  return traj, plain, continued, init, dsum


def test_pool_equals_the_numpy_loop_of_its_definition(fitted, whole):
  traj, plain, continued, init, _ = whole
  f = fitted.fit
  assert plain.shape == (len(GROUPS), N, T) and plain.dtype == np.float64
  assert (N * T) % 4 != 0                                   # misaligned series, a tail quad
  np.testing.assert_array_equal(plain, _pool_loop(traj, f.scale, f.shift, GROUPS))
  np.testing.assert_array_equal(continued, _pool_loop(traj, f.scale, f.shift, GROUPS, init))
  assert not np.array_equal(plain, continued)


def test_running_sum_chained_over_two_sessions_equals_one_session(fitted, whole):
  """Series 0-2, then series 3-4 (series_offset = 3) fed the first part's output: bit-equal to the
  session of all five.  The group of series 2 alone has no member in the second part and passes
  through it.  The argument checks that need a session are made on the second one."""
  _, plain, _, _, _ = whole
  f = fitted.fit
  first_ids, second_ids = np.arange(0, 3), np.arange(3, 5)
  _, csr = batch.aggregate_groups(AGGREGATES, NAMES)
  sess = fitted.session(first_ids)
  try:
    sess.run()
    first = sess.pool_trajectories(f.scale[first_ids], f.shift[first_ids],
                                   batch._PoolChain([], csr).groups_of(first_ids))
  finally:
    sess.close()
  sess = fitted.session(second_ids)
  try:
    groups = batch._PoolChain([], csr).groups_of(second_ids)
    assert groups[2] == {}
    with pytest.raises(_native.NativeError, match="needs a finished ci_session_run"):
      sess.pool_trajectories(f.scale[second_ids], f.shift[second_ids], groups, first)
    sess.run()
    second = sess.pool_trajectories(f.scale[second_ids], f.shift[second_ids], groups, first)
    # ---- refusals, straight through ctypes (the binding would not build these tables)
    L = _native.load()
    two, out = np.ones(2), np.zeros((1, N, T))

    def call(num_groups, offsets, members, weights):
      o, m = np.asarray(offsets, np.int32), np.asarray(members, np.int32)
      w = np.asarray(weights, np.float64)
      rc = L.ci_session_pool_trajectories(sess._h, two.ctypes.data, two.ctypes.data, num_groups,
                                          o.ctypes.data, m.ctypes.data, w.ctypes.data, None,
                                          out.ctypes.data)
      return rc, L.ci_last_error()

    for args, message in [((0, [0], [0], [1.0]), b"num_groups must be >= 1"),
                          ((1, [1, 2], [0, 1], [1.0, 1.0]), b"offsets[0] must be 0"),
                          ((2, [0, 2, 1], [0, 1], [1.0, 1.0]), b"offsets must not decrease"),
                          ((1, [0, 1], [2], [1.0]), b"out of range"),
                          ((1, [0, 1], [-1], [1.0]), b"out of range"),
                          ((1, [0, 2], [1, 0], [1.0, 1.0]), b"strictly ascending"),
                          ((1, [0, 2], [1, 1], [1.0, 1.0]), b"strictly ascending"),
                          ((1, [0, 2], [0, 1], [1.0, np.nan]), b"not finite"),
                          ((1, [0, 1], [0], [np.inf]), b"not finite")]:
      rc, error = call(*args)
      assert rc != 0 and message in error, (args, error)
    rc = L.ci_session_pool_trajectories(sess._h, None, two.ctypes.data, 1, None, None, None, None,
                                        out.ctypes.data)
    assert rc != 0 and b"NULL argument" in L.ci_last_error()
  finally:
    sess.close()
  np.testing.assert_array_equal(second, plain)


# ---- groups of more members than one chunk of loads ---------------------------------------------------
# 15 series, 17 steps, 3 chains x 3 draws: N*T = 153 is odd again.  The kernel adds the members of a
# group in chunks of 8, 4, 2 and 1: 15 = 8 + 4 + 2 + 1, 8, 9 = 8 + 1, 7 = 4 + 2 + 1, and 1.
MANY_B, MANY_T, MANY_DRAWS = 15, 17, 3
MANY_N = CHAINS * MANY_DRAWS
MANY_GROUPS = [{b: (-1.0) ** b * (0.25 + 0.5 * b) for b in range(15)},
               {b: 1.0 for b in range(0, 15, 2)},
               {b: 3.0 - b for b in (1, 2, 4, 5, 6, 7, 8, 9, 10)},
               {b: 0.125 * b for b in range(1, 15, 2)},
               {14: -2.5}]


@pytest.fixture(scope="module")
def many():
  """(trajectories [15, 9, 17] float32, scale, shift, pooled without init, pooled with init, init) of
  one ordinary session of 15 series."""
  rng = np.random.default_rng(3)
  x = rng.normal(size=(MANY_B, MANY_T, 1))
  y = 1.5 * x[:, :, 0] + 10.0 + 3.0 * np.arange(MANY_B)[:, None] + 0.3 * rng.normal(size=(MANY_B, MANY_T))
  prep = batch.prepare_batch(np.concatenate([y[:, :, None], x], axis=2), pd.RangeIndex(MANY_T), (0, 10), (11, 16))
  ys = batch._sampler_outcome(prep, ci.DataOptions())
  options = ci.InferenceOptions(num_results=MANY_DRAWS, num_chains=CHAINS, num_warmup_steps=5)
  f = batch._new_fit(prep, ys, np.full(MANY_B, MANY_T), np.nanstd(ys[:, :prep.num_pre], axis=1, ddof=1),
                     ALPHA, SEED, ci.ModelOptions(), options, False)
  pb = _native.make_problem(T=MANY_T, P=f.design.shape[2], has_slope=False, num_warmup=5,
                            num_results=MANY_DRAWS, num_chains=CHAINS, num_series=MANY_B, seed=f.seed, device=0)
  sess = _native.Session(pb, f.y, f.mask, f.design, None, _native.make_params(f.params))
  try:
    sess.run()
    traj = sess.fetch(["posterior_trajectories"])["posterior_trajectories"].reshape(MANY_B, MANY_N, MANY_T)
    init = np.random.default_rng(9).normal(size=(len(MANY_GROUPS), MANY_N, MANY_T)) * 50.0
    plain = sess.pool_trajectories(f.scale, f.shift, MANY_GROUPS)
    continued = sess.pool_trajectories(f.scale, f.shift, MANY_GROUPS, init)
  finally:
    sess.close()
  return traj, f.scale, f.shift, plain, continued, init


@pytest.mark.parametrize("with_init", [False, True])
def test_groups_of_up_to_15_members_equal_the_numpy_loop(many, with_init):
  traj, scale, shift, plain, continued, init = many
  assert [len(g) for g in MANY_GROUPS] == [15, 8, 9, 7, 1]
  assert any(w < 0 for w in MANY_GROUPS[0].values()) and (MANY_N * MANY_T) % 2 == 1
  assert np.isfinite(traj).all() and traj.std() > 0
  if with_init:
    np.testing.assert_array_equal(continued, _pool_loop(traj, scale, shift, MANY_GROUPS, init))
  else:
    np.testing.assert_array_equal(plain, _pool_loop(traj, scale, shift, MANY_GROUPS))


@pytest.fixture(scope="module")
def api(fitted):
  kw = dict(pre_period=PRE, post_period=POST, alpha=ALPHA, seed=SEED, names=NAMES)
  one = ci.fit_causalimpact_batch(fitted.values, inference_options=_options(devices=[0]),
                                  aggregates=AGGREGATES, **kw)
  return one, kw


def test_api_aggregates_do_not_depend_on_the_split_into_launches(fitted, api):
  one, kw = api
  two = ci.fit_causalimpact_batch(fitted.values, inference_options=_options(devices=[0, 0]),
                                  aggregates=AGGREGATES, **kw)
  assert list(one.aggregates) == list(AGGREGATES) == list(two.aggregates)
  for name in AGGREGATES:
    pd.testing.assert_frame_equal(one.aggregates[name].series, two.aggregates[name].series, check_exact=True)
    pd.testing.assert_frame_equal(one.aggregates[name].summary, two.aggregates[name].summary, check_exact=True)
  pd.testing.assert_frame_equal(one.aggregate_summary, two.aggregate_summary, check_exact=True)
  pd.testing.assert_frame_equal(one.summary, two.summary, check_exact=True)
  assert list(one.aggregate_summary.index) == [(a, r) for a in AGGREGATES for r in ("average", "cumulative")]
  assert list(one.aggregate_summary.columns) == list(one.summary.columns) and one.aggregate_summary.shape[1] == 15


def test_group_of_one_series_is_that_series(api):
  one, _ = api
  _assert_frames_identical(one.aggregates["one"].series, one[2].series)
  _assert_frames_identical(one.aggregates["one"].summary, one[2].summary)
  got = one.aggregate_summary.loc["one"]
  _assert_frames_identical(got, one[2].summary)


def test_aggregate_frames_equal_the_host_arithmetic_on_numpy_pooled_draws(fitted, whole, api):
  traj, _, _, _, dsum = whole
  one, _ = api
  f = fitted.fit
  # the API call drew what the session of the fixture drew
  np.testing.assert_array_equal(one._dsum["value_order"], dsum["value_order"])
  pooled = _pool_loop(traj, f.scale, f.shift, GROUPS)
  # every series' posterior mean on the data scale, with its own scaler's statistics
  means = []
  for b in range(B):
    d = cid.CausalImpactData(pd.DataFrame(fitted.values[b], columns=["y", "x0"]), PRE, POST)
    means.append(d.outcome_scaler.inverse_transform(one._means[b].astype(np.float64)))
  means = np.stack(means).reshape(B, T)
  for g, name in enumerate(AGGREGATES):
    group = GROUPS[g]
    outcome, mean = np.zeros(T), np.zeros(T)
    for b in sorted(group):
      outcome = outcome + group[b] * fitted.values[b, :, 0]
      mean = mean + group[b] * means[b]
    ci_data = cid.CausalImpactData(pd.DataFrame({"y": outcome}), PRE, POST, standardize_data=False)
    series, summary = lib._compute_impact(mean, pooled[g], ci_data, ALPHA)
    got = one.aggregates[name]
    _assert_frames_equal(got.series, series)
    _assert_frames_equal(got.summary, summary)
    _assert_frames_equal(one.aggregate_summary.loc[name], summary)
    nan_at = np.flatnonzero(np.isnan(got.series["observed"].to_numpy()))
    assert list(nan_at) == ([NAN_STEP] if NAN_SERIES in group else []), name
    assert got.posterior_samples is None
    assert np.isfinite(got.series["posterior_mean"].to_numpy()).all()      # gap / tail: predictions stay


def test_without_aggregates_nothing_changes(fitted, api):
  one, kw = api
  none = ci.fit_causalimpact_batch(fitted.values, inference_options=_options(devices=[0]),
                                   aggregates=None, **kw)
  plain = ci.fit_causalimpact_batch(fitted.values, inference_options=_options(devices=[0]), **kw)
  assert none.aggregates is None and none.aggregate_summary is None
  assert plain.aggregates is None and plain.aggregate_summary is None
  pd.testing.assert_frame_equal(none.summary, plain.summary, check_exact=True)
  pd.testing.assert_frame_equal(one.summary, plain.summary, check_exact=True)   # ... nor with them
  pd.testing.assert_frame_equal(one[1].series, plain[1].series, check_exact=True)


def test_hmc_batch_in_one_launch_pools_on_the_device(fitted):
  """The one-launch HMC route (trend model, short run): ci_ll_session_pool_trajectories against the
  numpy loop on the trajectories of the same session, and the API's frames against the host
  arithmetic on them."""
  f = fitted.fit
  chains, draws, warm = 2, 24, 30
  pb = _native.make_problem(T=T, P=f.design.shape[2], has_slope=False, num_warmup=0, num_results=1,
                            num_series=B, seed=f.seed, device=0, series_offset=0)
  sess = _native.BatchLogLikSession(pb, _native.make_params(list(f.params)), f.y, f.mask, f.design)
  try:
    with pytest.raises(_native.NativeError, match="needs a finished ci_ll_session_hmc_run"):
      sess._hmc_shape = (chains, draws)
      sess.pool_trajectories(f.scale, f.shift, GROUPS)
    sess.hmc_run(num_chains=chains, num_warmup=warm, num_results=draws, seed=f.seed)
    # the refusals of the shared checks through this entry point too
    L = _native.load()
    ones, room = np.ones(B), np.zeros((1, chains * draws, T))
    for offsets, members, weights, message in [([0, 1], [B], [1.0], b"out of range"),
                                               ([0, 2], [1, 1], [1.0, 1.0], b"strictly ascending"),
                                               ([0, 1], [0], [np.nan], b"not finite")]:
      o, m, w = np.asarray(offsets, np.int32), np.asarray(members, np.int32), np.asarray(weights, np.float64)
      rc = L.ci_ll_session_pool_trajectories(sess._h, ones.ctypes.data, ones.ctypes.data, 1, o.ctypes.data,
                                             m.ctypes.data, w.ctypes.data, None, room.ctypes.data)
      assert rc != 0 and message in L.ci_last_error(), (offsets, L.ci_last_error())
    _, _, _, out = sess.hmc_fetch(["posterior_trajectories", "posterior_means"], with_draws=False)
    init = np.random.default_rng(8).normal(size=(len(GROUPS), chains * draws, T))
    got = sess.pool_trajectories(f.scale, f.shift, GROUPS)
    continued = sess.pool_trajectories(f.scale, f.shift, GROUPS, init)
  finally:
    sess.close()
  traj = out["posterior_trajectories"].reshape(B, chains * draws, T)
  pooled = _pool_loop(traj, f.scale, f.shift, GROUPS)
  np.testing.assert_array_equal(got, pooled)
  np.testing.assert_array_equal(continued, _pool_loop(traj, f.scale, f.shift, GROUPS, init))

  io = ci.InferenceOptions(sampler="hmc", num_results=draws, num_chains=chains, num_warmup_steps=warm)
  assert batch.hmc_batch_route(float64=False, standardize_data=True, num_seasonal_blocks=0, T=T, P=2,
                               hmc_init="gibbs") == "one_launch"
  res = ci.fit_causalimpact_batch(fitted.values, PRE, POST, alpha=ALPHA, seed=SEED, names=NAMES,
                                  inference_options=io, aggregates=AGGREGATES)
  assert isinstance(res, batch.CausalImpactBatchAnalysis) and not isinstance(res, batch.PerSeriesBatchAnalysis)
  np.testing.assert_array_equal(res._means, out["posterior_means"].mean(axis=1))   # the same fit
  _assert_frames_identical(res.aggregates["one"].series, res[2].series)
  _assert_frames_identical(res.aggregates["one"].summary, res[2].summary)
  mu, sd = batch.scaler_stats(fitted.values[:, :32, 0])
  means = res._means.astype(np.float64) * sd[:, None] + mu[:, None]
  for g, name in enumerate(AGGREGATES):
    group = GROUPS[g]
    outcome, mean = np.zeros(T), np.zeros(T)
    for b in sorted(group):
      outcome = outcome + group[b] * fitted.values[b, :, 0]
      mean = mean + group[b] * means[b]
    ci_data = cid.CausalImpactData(pd.DataFrame({"y": outcome}), PRE, POST, standardize_data=False)
    series, summary = lib._compute_impact(mean, pooled[g], ci_data, ALPHA)
    _assert_frames_equal(res.aggregates[name].series, series)
    _assert_frames_equal(res.aggregates[name].summary, summary)


def test_float64_batch_pools_on_the_per_series_route():
  """Three series, float64: fitted series by series, the same sum accumulated in numpy.  The group of
  one series gives that series' analysis; the total equals the host arithmetic on the sum of the
  three fits' own data-scale trajectories."""
  v = _values(3, seed=4)
  names = NAMES[:3]
  aggregates = {"total": "all", "one": ["south"], "mix": {"north": 0.5, "east": -2.0}}
  kw = dict(alpha=ALPHA, seed=SEED, data_options=ci.DataOptions(dtype=np.float64),
            inference_options=_options())
  res = ci.fit_causalimpact_batch(v, PRE, POST, names=names, aggregates=aggregates, **kw)
  assert isinstance(res, batch.PerSeriesBatchAnalysis)
  assert list(res.aggregates) == list(aggregates)
  _assert_frames_equal(res.aggregates["one"].series, res[1].series)
  _assert_frames_equal(res.aggregates["one"].summary, res[1].summary)
  _assert_frames_equal(res.aggregate_summary.loc["one"], res[1].summary)
  plain = ci.fit_causalimpact_batch(v, PRE, POST, names=names, **kw)
  assert plain.aggregates is None
  _assert_frames_equal(res.summary, plain.summary)
  # the total against the host arithmetic on the three single fits' trajectories
  sunk = []
  for b in range(3):
    lib.fit_causalimpact(pd.DataFrame(v[b], columns=["y", "x0"]), PRE, POST,
                         seed=_native.series_stream_key(SEED, b), alpha=ALPHA,
                         data_options=ci.DataOptions(dtype=np.float64), inference_options=_options(),
                         _trajectory_sink=lambda *a: sunk.append(a))
  total_draws, total_mean, outcome = 0.0, 0.0, 0.0
  for b, (pm, tr, scale, shift) in enumerate(sunk):
    assert tr.dtype == np.float64
    total_draws = total_draws + 1.0 * (tr * scale + shift)
    total_mean = total_mean + 1.0 * (pm * scale + shift)
    outcome = outcome + 1.0 * v[b, :, 0]
  ci_data = cid.CausalImpactData(pd.DataFrame({"y": outcome}), PRE, POST, standardize_data=False)
  series, summary = lib._compute_impact(total_mean, total_draws, ci_data, ALPHA)
  _assert_frames_equal(res.aggregates["total"].series, series)
  _assert_frames_equal(res.aggregates["total"].summary, summary)


def test_raw_scale_float32_series_do_not_change_with_aggregates():
  """`standardize_data=False` in float32: fitted series by series.  With aggregates the fits keep
  their trajectories on the host and summarise them there with the same kernels on the same values:
  every series' frames and the summary table are the ones without aggregates, exactly; the group of
  one series gives that series' analysis at the tolerance of device against host frames."""
  v = _values(3, seed=6)
  names = NAMES[:3]
  kw = dict(alpha=ALPHA, seed=SEED, names=names, data_options=ci.DataOptions(standardize_data=False),
            inference_options=_options())
  with_ = ci.fit_causalimpact_batch(v, PRE, POST, aggregates={"total": "all", "one": ["south"]}, **kw)
  without = ci.fit_causalimpact_batch(v, PRE, POST, **kw)
  assert isinstance(with_, batch.PerSeriesBatchAnalysis) and without.aggregates is None
  pd.testing.assert_frame_equal(with_.summary, without.summary, check_exact=True)
  for b in range(3):
    _assert_frames_identical(with_[b].series, without[b].series)
    _assert_frames_identical(with_[b].summary, without[b].summary)
  _assert_frames_equal(with_.aggregates["one"].series, with_[1].series)
  _assert_frames_equal(with_.aggregates["one"].summary, with_[1].summary)
  nan_free = with_.aggregates["total"].series["observed"].to_numpy()
  np.testing.assert_array_equal(nan_free, (0.0 + v[0, :, 0]) + v[1, :, 0] + v[2, :, 0])
