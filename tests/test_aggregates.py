"""Aggregates of a batch (`fit_causalimpact_batch(aggregates=...)`), the parts that need no GPU: the
group specification and its refusals, the pooled observed / posterior-mean arithmetic, the numpy
accumulator of the routes that fit series by series, and the two C-ABI entry points
(ci_session_pool_trajectories, ci_ll_session_pool_trajectories): declared, bound and exported with
one signature, argument errors before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _native
from causalimpact import batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["north", "south", "east", "west", "centre"]


# ---- the group specification ---------------------------------------------------------------------
def test_names_weights_and_all_become_csr():
  names, (offsets, members, weights) = batch.aggregate_groups(
      {"total": "all", "mix": {"west": -2.0, "north": 0.5}, "one": ["east"],
       "pair": ("south", "north"), "dropped": {"south": 0.0, "centre": 3.0}}, NAMES)
  assert names == ["total", "mix", "one", "pair", "dropped"]
  assert offsets.dtype == np.int32 and members.dtype == np.int32 and weights.dtype == np.float64
  np.testing.assert_array_equal(offsets, [0, 5, 7, 8, 10, 11])
  np.testing.assert_array_equal(members, [0, 1, 2, 3, 4, 0, 3, 2, 0, 1, 4])       # ascending per group
  np.testing.assert_array_equal(weights, [1, 1, 1, 1, 1, 0.5, -2.0, 1, 1, 1, 3.0])  # zero weight left out


@pytest.mark.parametrize("spec, message", [
    ({"g": ["north", "nowhere"]}, "unknown series 'nowhere'"),
    ({"g": {"nowhere": 1.0}}, "unknown series 'nowhere'"),
    ({"g": []}, "is empty"),
    ({"g": {}}, "is empty"),
    ({"g": {"north": 0.0}}, "is empty"),
    ({"g": {"north": np.nan}}, "not finite"),
    ({"g": {"north": 1.0, "south": np.inf}}, "not finite"),
    ({"g": ["north", "south", "north"]}, "listed twice"),
    ({"g": "north"}, "the string 'all'"),
    ({}, "`aggregates` is empty"),
    (["north"], "must be a mapping"),
])
def test_group_specification_refusals(spec, message):
  with pytest.raises(ValueError, match=message):
    batch.aggregate_groups(spec, NAMES)


def test_series_names_must_be_unique_for_aggregates():
  with pytest.raises(ValueError, match="unique series names"):
    batch.aggregate_groups({"g": "all"}, ["a", "b", "a"])


def _values(B=5, T=47, seed=0):
  rng = np.random.default_rng(seed)
  x = rng.normal(size=(B, T, 1))
  y = 1.5 * x[:, :, 0] + 10.0 + np.arange(B)[:, None] + 0.3 * rng.normal(size=(B, T))
  return np.concatenate([y[:, :, None], x], axis=2)


def test_fit_refuses_bad_aggregates_before_any_device_work():
  """Through the public call: every refusal is raised ahead of data preparation and launches."""
  v = _values()
  kw = dict(pre_period=(0, 31), post_period=(32, 42), names=NAMES)
  with pytest.raises(ValueError, match="shared_streams=True.*perfectly correlated.*joint posterior"):
    ci.fit_causalimpact_batch(v, aggregates={"total": "all"}, shared_streams=True, **kw)
  with pytest.raises(ValueError, match="unknown series 'nowhere'"):
    ci.fit_causalimpact_batch(v, aggregates={"g": ["nowhere"]}, **kw)
  with pytest.raises(ValueError, match="is empty"):
    ci.fit_causalimpact_batch(v, aggregates={"g": []}, **kw)
  with pytest.raises(ValueError, match="not finite"):
    ci.fit_causalimpact_batch(v, aggregates={"g": {"north": np.inf}}, **kw)
  with pytest.raises(ValueError, match="listed twice"):
    ci.fit_causalimpact_batch(v, aggregates={"g": ["east", "east"]}, **kw)
  with pytest.raises(TypeError):
    ci.fit_causalimpact_panel([pd.DataFrame(v[0])], [((0, 31), (32, 42))], aggregates={"g": "all"})


def test_groups_are_cut_to_the_positions_of_a_launch():
  _, csr = batch.aggregate_groups({"total": "all", "mix": {"north": 0.5, "west": -2.0}, "one": ["east"]},
                                  NAMES)
  assert batch._PoolChain([], csr).groups_of(np.array([0, 1, 2])) == [{0: 1.0, 1: 1.0, 2: 1.0}, {0: 0.5}, {2: 1.0}]
  assert batch._PoolChain([], csr).groups_of(np.array([3, 4])) == [{0: 1.0, 1: 1.0}, {0: -2.0}, {}]


# ---- pooled observed and posterior mean ----------------------------------------------------------
def test_pooled_rows_are_the_ordered_float64_sum_and_propagate_nan():
  rng = np.random.default_rng(1)
  rows = rng.normal(size=(5, 47)) * 1e3
  rows[1, 40] = np.nan
  _, csr = batch.aggregate_groups({"total": "all", "mix": {"north": 0.5, "west": -2.0}, "one": ["east"]},
                                  NAMES)
  got = batch.pool_weighted(rows, csr)
  want = np.zeros((3, 47))
  for g, group in enumerate([{0: 1.0, 1: 1.0, 2: 1.0, 3: 1.0, 4: 1.0}, {0: 0.5, 3: -2.0}, {2: 1.0}]):
    for t in range(47):
      acc = 0.0
      for b in sorted(group):
        acc = acc + group[b] * float(rows[b, t])
      want[g, t] = acc
  np.testing.assert_array_equal(got, want)
  assert np.isnan(got[0, 40]) and not np.isnan(got[1:, 40]).any()       # NaN where a MEMBER is NaN
  assert np.isnan(got).sum() == 1
  # an initial accumulator is continued, not overwritten
  init = rng.normal(size=(1, 47))
  _, last_two = batch.aggregate_groups({"a": "all"}, [0, 1])
  np.testing.assert_array_equal(batch.pool_weighted(rows[3:], last_two, init),
                                (init + 1.0 * rows[3]) + 1.0 * rows[4])


def test_pooled_observed_has_the_gap_and_tail_of_the_calendar():
  """32 pre-period steps, a gap of 2, a window of 11, a tail of 2: the pooled observed outcome is NaN
  in gap and tail like every member's, and equals the request built from the pooled raw outcome."""
  from causalimpact import causalimpact_lib as lib
  from causalimpact import data as cid
  v = _values()
  v[3, 38, 0] = np.nan
  prep = batch.prepare_batch(v, pd.RangeIndex(47), (0, 31), (34, 44))
  _, csr = batch.aggregate_groups({"total": "all", "mix": {"north": 0.5, "west": -2.0}}, NAMES)
  observed = batch.pool_weighted(prep.observed, csr)
  outcome = batch.pool_weighted(prep.values[:, :, 0], csr)
  gap_tail = np.r_[32, 33, 45, 46]
  assert np.isnan(observed[:, gap_tail]).all()
  assert np.isnan(observed[:, 38]).all() and np.isnan(observed).sum() == 2 * 5
  for g in range(2):
    ci_data = cid.CausalImpactData(pd.DataFrame({"y": outcome[g]}), (0, 31), (34, 44),
                                   standardize_data=False)
    rq = lib._device_summary_request(ci_data, 0.05)
    np.testing.assert_array_equal(rq["observed"], observed[g])
    np.testing.assert_array_equal(rq["flags"], prep.flags)
    assert (rq["scale"], rq["shift"]) == (1.0, 0.0)


def test_scaler_stats_are_the_single_series_scaler():
  from causalimpact import data as cid
  v = _values(seed=3) * 37.0
  v[2, 5, 0] = np.nan
  mu, sd = batch.scaler_stats(v[:, :32, 0])
  for b in range(5):
    d = cid.CausalImpactData(pd.DataFrame(v[b], columns=["y", "x"]), (0, 31), (32, 42))
    assert float(np.ravel(d.outcome_scaler.mean_)[0]) == mu[b]
    assert float(np.ravel(d.outcome_scaler.stddev_)[0]) == sd[b]


# ---- the accumulator of the per-series routes ------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_pool_equals_an_explicit_loop_bit_for_bit(dtype):
  rng = np.random.default_rng(2)
  B, N, T = 4, 7, 9
  traj = rng.normal(size=(B, N, T)).astype(dtype)
  pm = rng.normal(size=(B, T)).astype(dtype)
  scale = rng.uniform(0.5, 30.0, B)
  shift = rng.normal(size=B) * 100.0
  groups = [{0: 1.0, 1: 1.0, 2: 1.0, 3: 1.0}, {0: 0.5, 3: -2.0}, {2: 1.0}, {1: 0.3, 2: 0.7}, {2: 1.0, 3: 1.0}]
  csr = _native.groups_csr(groups, B)
  pool = batch.HostPool(csr)
  for b in range(B):
    pool.add(b, pm[b], traj[b], scale[b], shift[b])
  want = np.zeros((len(groups), N, T))
  for g, group in enumerate(groups):
    for n in range(N):
      for t in range(T):
        acc = 0.0
        for b in sorted(group):
          value = float(traj[b, n, t]) * float(scale[b]) + float(shift[b])
          acc = acc + group[b] * value
        want[g, n, t] = acc
  np.testing.assert_array_equal(pool.pooled, want)
  np.testing.assert_array_equal(_native.pool_host(traj, scale, shift, groups), want)
  np.testing.assert_array_equal(np.stack(pool.means), pm.astype(np.float64) * scale[:, None] + shift[:, None])
  # a sum continued through `init` equals the sum in one piece
  first = _native.pool_host(traj[:2], scale[:2], shift[:2], [{b: w for b, w in g.items() if b < 2} for g in groups])
  rest = _native.pool_host(traj[2:], scale[2:], shift[2:],
                           [{b - 2: w for b, w in g.items() if b >= 2} for g in groups], init=first)
  np.testing.assert_array_equal(rest, want)


def test_groups_csr_refusals():
  for groups, message in [([{5: 1.0}], "outside"), ([{-1: 1.0}], "outside"), ([[1, 1]], "listed twice"),
                          ([{0: np.nan}], "not finite")]:
    with pytest.raises(ValueError, match=message):
      _native.groups_csr(groups, 5)
  offsets, members, weights = _native.groups_csr([[3, 1], {}, {2: 0.0, 0: 2.0}], 5)
  np.testing.assert_array_equal(offsets, [0, 2, 2, 3])
  np.testing.assert_array_equal(members, [1, 3, 0])
  np.testing.assert_array_equal(weights, [1.0, 1.0, 2.0])


# ---- the C-ABI ------------------------------------------------------------------------------------
POOL_SYMBOLS = ("ci_session_pool_trajectories", "ci_ll_session_pool_trajectories")
_CTYPE_OF = {"int32_t": C.c_int32}


def _header_parameters(symbol):
  hdr = open(os.path.join(ROOT, "include", "causalimpact_amd.h")).read()
  hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
  m = re.search(r"\bint\s+" + symbol + r"\s*\(([^)]*)\)\s*;", hdr)
  assert m, f"{symbol} is not declared"
  return [" ".join(p.split()) for p in m.group(1).split(",")]


@pytest.mark.parametrize("symbol", POOL_SYMBOLS)
def test_header_binding_and_library_agree_on_the_signature(symbol):
  params = _header_parameters(symbol)
  session = "ci_session*" if symbol == "ci_session_pool_trajectories" else "ci_ll_session*"
  assert params == [f"{session} session", "const double* scale", "const double* shift",
                    "int32_t num_groups", "const int32_t* offsets", "const int32_t* members",
                    "const double* weights", "const double* init", "double* out"]
  assert symbol in _native.exported_symbols()
  lib = C.CDLL(_native.LIB_PATH)
  assert hasattr(lib, symbol)
  bound = getattr(_native.load(), symbol).argtypes
  want = [C.c_void_p if "*" in p else _CTYPE_OF[p.split()[0]] for p in params]
  assert list(bound) == want


@pytest.mark.parametrize("symbol", POOL_SYMBOLS)
def test_null_arguments_are_refused_before_any_device_call(symbol):
  """No session can exist without a GPU, so what is reachable here is the first check: a NULL
  session, with every other argument valid, is an error and not a crash.  (The checks behind it --
  finished run, groups, members, weights -- need a session: tests/test_gpu_aggregates.py.)"""
  fn = getattr(_native.load(), symbol)
  one = np.ones(1)
  off, mem = np.array([0, 1], np.int32), np.zeros(1, np.int32)
  out = np.zeros(4)
  rc = fn(None, one.ctypes.data, one.ctypes.data, 1, off.ctypes.data, mem.ctypes.data, one.ctypes.data,
          None, out.ctypes.data)
  assert rc != 0 and b"NULL argument" in _native.load().ci_last_error()
  assert _native.load().ci_abi_version() == 5 == _native.ABI_VERSION        # additive: no version bump


# ---- the chain of pool steps over the launches of a batch ------------------------------------------
def _fake_launch_pool(traj, scale, shift, ids):
  """What a session over the positions `ids` would compute, in numpy."""
  return lambda groups, init: _native.pool_host(traj[ids], scale[ids], shift[ids], groups, init)


def test_pool_chain_hands_the_accumulator_from_launch_to_launch():
  rng = np.random.default_rng(5)
  B, N, T = 5, 3, 4
  traj = rng.normal(size=(B, N, T)).astype(np.float32)
  scale, shift = rng.uniform(1, 2, B), rng.normal(size=B)
  _, csr = batch.aggregate_groups({"total": "all", "mix": {"north": 0.5, "west": -2.0}, "one": ["east"]},
                                  NAMES)
  groups = [{0: 1.0, 1: 1.0, 2: 1.0, 3: 1.0, 4: 1.0}, {0: 0.5, 3: -2.0}, {2: 1.0}]
  want = _native.pool_host(traj, scale, shift, groups)
  for cut in ([[0, 1, 2, 3, 4]], [[0, 1, 2], [3, 4]], [[0], [1], [2, 3], [4]]):
    launches = [(0, T, ids) for ids in cut]
    chain = batch._PoolChain(launches, csr)
    for launch in launches:
      chain.step(launch, _fake_launch_pool(traj, scale, shift, np.asarray(launch[2])))
    np.testing.assert_array_equal(chain.result(), want)
  # launches of two devices run side by side: the second waits for the first
  from causalimpact import causalimpact_lib as lib
  launches = [(0, T, [0, 1, 2]), (1, T, [3, 4])]
  chain = batch._PoolChain(launches, csr)
  lib.map_by_device(chain.guarded(lambda launch: chain.step(
      launch, _fake_launch_pool(traj, scale, shift, np.asarray(launch[2])))), launches)
  np.testing.assert_array_equal(chain.result(), want)


def test_chain_with_full_width_axes_from_step_zero_is_the_chain_without_axes():
  """A calendar aggregate is the event-time aggregate whose members all start at step 0 with the width
  T: one chain built without axes and one built with such axes, driven by the same fake session, end
  in the same accumulator."""
  rng = np.random.default_rng(6)
  B, N, T = 5, 3, 4
  traj = (rng.normal(size=(B, N, T)) * 10.0 ** rng.integers(-3, 4, size=(B, 1, 1))).astype(np.float32)
  scale, shift = rng.uniform(1, 2, B), rng.normal(size=B)
  _, csr = batch.aggregate_groups({"total": "all", "mix": {"north": 0.5, "west": -2.0}, "one": ["east"]},
                                  NAMES)
  offsets = csr[0]
  axes = [batch.EventAxis(L=1, gap=0, Hwin=1, H=T - 1, first=np.zeros(offsets[g + 1] - offsets[g], np.int32))
          for g in range(3)]
  seen = []

  def fake_pool(ids):
    def pool(groups, init):
      seen.append(type(groups[0]))
      if isinstance(groups[0], tuple):
        return _native.pool_event_host(traj[ids], scale[ids], shift[ids], groups, init)
      return _native.pool_host(traj[ids], scale[ids], shift[ids], groups, init)
    return pool

  # (positions that interleave: what a batch never has and a panel does)
  for cut in ([[0, 1, 2, 3, 4]], [[0, 1, 2], [3, 4]], [[0, 2, 4], [1, 3]]):
    launches = [(0, T, ids) for ids in cut]
    plain, event = batch._PoolChain(launches, csr), batch._PoolChain(launches, csr, axes)
    assert plain.stride is None and event.stride == T
    for launch in launches:
      plain.step(launch, fake_pool(np.asarray(launch[2])))
      event.step(launch, fake_pool(np.asarray(launch[2])))
    assert plain.result().shape == (3, N, T)
    np.testing.assert_array_equal(event.result(), plain.result())
  assert set(seen) == {dict, tuple}


def test_pool_chain_passes_a_failure_on_instead_of_blocking():
  from causalimpact import causalimpact_lib as lib
  _, csr = batch.aggregate_groups({"total": "all"}, NAMES)
  launches = [(0, 4, [0, 1, 2]), (1, 4, [3, 4])]

  def failing(chain):
    def run(launch):
      if launch[0] == 0:
        raise RuntimeError("the fit of the first launch failed")
      chain.step(launch, lambda groups, init: np.zeros((1, 2, 4)))
    return chain.guarded(run)

  # the launch that waits gets its predecessor's exception, and so does whoever asks for the result
  chain = batch._PoolChain(launches, csr)
  run = failing(chain)
  with pytest.raises(RuntimeError, match="first launch failed"):
    run(launches[0])
  with pytest.raises(RuntimeError, match="first launch failed"):
    run(launches[1])
  with pytest.raises(RuntimeError, match="first launch failed"):
    chain.result()
  # side by side on two devices: the call ends with the exception, nothing stays blocked
  with pytest.raises(RuntimeError, match="first launch failed"):
    lib.map_by_device(failing(batch._PoolChain(launches, csr)), launches)


def test_pool_chain_failure_reaches_a_waiter_behind_a_launch_that_never_runs():
  """Two launches on the first device and one on a second.  The first launch fails; its device stops
  there, so the second launch never runs -- and the third, on the other device, waits for the
  second.  It must get the error instead of blocking with its session open."""
  import threading
  from causalimpact import causalimpact_lib as lib
  _, csr = batch.aggregate_groups({"total": "all"}, NAMES)
  launches = [(0, 4, [0, 1]), (0, 4, [2]), (1, 4, [3, 4])]
  chain = batch._PoolChain(launches, csr)
  ran = []

  def run(launch):
    ran.append(tuple(launch[2]))
    if launch[2] == [0, 1]:
      raise RuntimeError("the fit of the first launch failed")
    chain.step(launch, lambda groups, init: np.zeros((1, 2, 4)))

  outcome = []

  def call():
    try:
      lib.map_by_device(chain.guarded(run), launches)
      outcome.append(None)
    except BaseException as e:   # pylint: disable=broad-except
      outcome.append(e)

  worker = threading.Thread(target=call, daemon=True)
  worker.start()
  worker.join(timeout=20)
  assert not worker.is_alive(), "a launch is blocked on an accumulator that never comes"
  assert isinstance(outcome[0], RuntimeError) and "first launch failed" in str(outcome[0])
  assert (2,) not in ran
  with pytest.raises(RuntimeError, match="first launch failed"):
    chain.result()
  # the same without threads: every future behind the failed launch carries its error
  chain = batch._PoolChain(launches, csr)
  chain.fail(launches[0], RuntimeError("gone"))
  with pytest.raises(RuntimeError, match="gone"):
    chain.step(launches[2], lambda groups, init: np.zeros((1, 2, 4)))
