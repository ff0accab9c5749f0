"""Joint bands and the whole-path test of POOLED effects on the device.

ci_summarize_draw_paths_f64 (first pass: path_values_f64_kernel of csrc/ci_paths.h) on synthetic
float64 draws against `_native.path_excursions_host` on the same arrays, by the method of
tests/test_gpu_joint_bands.py: center within 1e-10 * max_n |x[n, t]| and spread within 1e-10 relative
(the device adds the draws in its own order: at most N * 2^-53), and GIVEN the device's center and
spread, excursion, excursion_order, observed_excursion, at and exceed are the host loop's bit for bit.

G = 3 groups of N = 300 draws: one full stripe of 256 threads plus 44 draws, whose last 64-draw tile
holds 44 rows.  T = 67 is one 64-step tile and a remainder, rows off the 16-byte grid; T = 72 takes the
16-byte loads.

Then `fit_causalimpact_batch(aggregates=..., joint_bands=True)` and
`fit_causalimpact_panel(event_aggregates=..., joint_bands=True)` against `lib._joint_frames` on
`path_excursions_host` of numpy-pooled draws."""
import functools
import warnings

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _model
from causalimpact import _native
from causalimpact import batch
from causalimpact import causalimpact_lib as lib
from causalimpact import _synthetic as syn

pytestmark = pytest.mark.gpu

G, N = 3, 300
RANKS = [0, 150, 284, 285, 299]
SCALE, SHIFT = (3.7, -0.5, 1.0), (-12.25, 4.0, 0.0)
# (first, count): the post-period, across the tile edge, the last step, an empty window, two that
# overlap; the observations of steps 52 and 62 are missing
WINDOWS = ((40, 27), (60, 7), (66, 1), (55, 0), (45, 10), (50, 12))
# group 2, windows 0 and 4: no observation inside
GROUP_WINDOWS = (WINDOWS, ((45, 20), (64, 3), (0, 67), (50, 0), (60, 5), (66, 1)),
                 ((50, 4), (40, 27), (63, 2), (41, 1), (50, 4), (44, 0)))
HOLES = ((52, 62), (52, 62, 45), (52, 62, 50, 51, 53, 60))
BITWISE = ("excursion", "excursion_order", "observed_excursion", "at", "exceed")


def _tables(windows):
  return (np.array([[f for f, _ in ws] for ws in windows], np.int32),
          np.array([[c for _, c in ws] for ws in windows], np.int32))


@functools.lru_cache(maxsize=None)
def _inputs(T):
  """(draws [G, N, T] float64, observed [G, T], first, count [G, W]); T = 72: window 0 of group 0 is
  stretched to the last step."""
  rng = np.random.default_rng(100 + T)
  draws = rng.normal(size=(G, N, T)) * 2.5 + np.cumsum(rng.normal(size=(G, N, T)) * 0.2, axis=2) + 7.0
  obs = rng.normal(size=(G, T)) * 3.0 + 10.0
  for g, steps in enumerate(HOLES):
    obs[g, list(steps)] = np.nan
  windows = GROUP_WINDOWS if T == 67 else (((40, T - 40),) + WINDOWS[1:],) + GROUP_WINDOWS[1:]
  first, count = _tables(windows)
  for a in (draws, obs, first, count):
    a.setflags(write=False)
  return draws, obs, first, count


@functools.lru_cache(maxsize=None)
def _host(T):
  """The host loop on `_inputs(T)`, computed once."""
  draws, obs, first, count = _inputs(T)
  return _native.path_excursions_host(draws, SCALE, SHIFT, obs, first, count, RANKS)


def _check(got, draws, obs, first, count, own, scale=SCALE, shift=SHIFT, ranks=RANKS):
  """The method of tests/test_gpu_joint_bands.py::_check."""
  B, N_, T = draws.shape
  W = first.shape[1]
  assert set(got) == set(_native.PATH_OUTPUTS)
  assert got["center"].shape == got["spread"].shape == (B, W, 2, T)
  assert got["excursion"].shape == (B, W, 2, N_) and got["excursion_order"].shape == (B, W, 2, len(ranks))
  assert got["at"].dtype == got["exceed"].dtype == np.int32
  # 1. the moments, to the summation error of N draws
  for k in ("center", "spread"):
    np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(own[k]), err_msg=k)
  with np.errstate(all="ignore"), warnings.catch_warnings():
    warnings.simplefilter("ignore", RuntimeWarning)                     # (steps outside a window: all NaN)
    big = np.nanmax(np.abs(own["x"]), axis=3)                           # [B, W, 2, T]
  there = ~np.isnan(own["center"])
  err = np.abs(got["center"] - own["center"])[there]
  print(f"  T = {T}: center: max error {err.max():.3e}, the smallest bound {(1e-10 * big[there]).min():.3e}")
  assert (err <= 1e-10 * big[there]).all()
  rel = (np.abs(got["spread"] - own["spread"]) / own["spread"])[there]
  print(f"  T = {T}: spread: max relative error {rel.max():.3e}")
  assert (rel <= 1e-10).all()
  # 2. everything else from the device's own moments, bit for bit
  want = _native.path_excursions_host(draws, scale, shift, obs, first, count, ranks,
                                      center=got["center"], spread=got["spread"])
  for k in BITWISE:
    np.testing.assert_array_equal(got[k], want[k], err_msg=k)
  # 3. the conventions
  empty = count == 0
  assert empty.any()
  assert (got["excursion"][empty] == 0.0).all() and (got["excursion_order"][empty] == 0.0).all()
  assert np.isnan(got["observed_excursion"][empty]).all()
  assert (got["at"][empty] == -1).all() and (got["exceed"][empty] == 0).all()
  assert np.isnan(got["center"][empty]).all() and np.isnan(got["spread"][empty]).all()
  assert not np.isnan(got["excursion"]).any()
  for b in range(B):
    for w in range(W):
      f, c = first[b, w], count[b, w]
      has = ~np.isnan(obs[b, f:f + c])
      outside = np.ones(T, bool)
      outside[f:f + c] = False
      assert np.isnan(got["center"][b, w][:, outside]).all()
      assert not np.isnan(got["center"][b, w, 0, f:f + c]).any()
      np.testing.assert_array_equal(np.isnan(got["center"][b, w, 1, f:f + c]), ~has)
      if has.any():
        assert (got["at"][b, w] >= f).all() and (got["at"][b, w] < f + c).all()
        assert (got["excursion"][b, w] > 0.0).all()
      else:
        assert (got["at"][b, w] == -1).all() and (got["excursion"][b, w] == 0.0).all()
        assert np.isnan(got["observed_excursion"][b, w]).all()


@pytest.mark.parametrize("T", [67, 72])
def test_entry_equals_the_host_loop(T):
  draws, obs, first, count = _inputs(T)
  assert (T % 2 == 0) == (T == 72) and N % 64 == 44 and N > 256
  got = _native.summarize_draw_paths(draws, SCALE, SHIFT, obs, first, count, RANKS)
  _check(got, draws, obs, first, count, _host(T))
  # group 2 has no observation inside its windows 0 and 4
  assert (got["at"][2, 0] == -1).all() and (got["at"][2, 4] == -1).all()
  assert (got["at"][0, 0] >= 0).all()
  # ... and some of the outputs alone
  part = _native.summarize_draw_paths(draws, SCALE, SHIFT, obs, first, count, RANKS, want=("spread", "exceed"))
  assert list(part) == ["spread", "exceed"]
  np.testing.assert_array_equal(part["spread"], got["spread"])
  np.testing.assert_array_equal(part["exceed"], got["exceed"])


def _table_bytes(T, W):
  """The tables of a call (include/causalimpact_amd.h)."""
  return (G * T + 2 * G) * 8 + 2 * G * W * 4 + (G * W + 1) * 8 + 8 * 4


def _pair_bytes(c):
  return (c * (2 * N + 4) + 2 * N + 20) * 8


def test_chunks_equal_one_call():
  """The limit of the call's device memory so small that (a) every group is a chunk of its own, (b) a
  chunk ends inside a group, whose draws travel again."""
  T = 67
  draws, obs, first, count = _inputs(T)
  W = first.shape[1]
  tables, group = _table_bytes(T, W), N * T * 8
  whole = _native.summarize_draw_paths(draws, SCALE, SHIFT, obs, first, count, RANKS, max_bytes=1 << 30)
  plain = _native.summarize_draw_paths(draws, SCALE, SHIFT, obs, first, count, RANKS)
  assert whole.pop("num_chunks") == 1
  per_group = max(sum(_pair_bytes(c) for c in count[g]) for g in range(G))
  by_group = _native.summarize_draw_paths(draws, SCALE, SHIFT, obs, first, count, RANKS,
                                          max_bytes=tables + group + per_group + 64)
  largest = max(_pair_bytes(c) for c in count.ravel())
  by_pair = _native.summarize_draw_paths(draws, SCALE, SHIFT, obs, first, count, RANKS,
                                         max_bytes=tables + group + largest + 64)
  print(f"  chunks: {by_group['num_chunks']} by group, {by_pair['num_chunks']} inside groups")
  assert by_group.pop("num_chunks") == 3
  assert by_pair.pop("num_chunks") > 3
  for k in _native.PATH_OUTPUTS:
    np.testing.assert_array_equal(plain[k], whole[k], err_msg=k)
    np.testing.assert_array_equal(by_group[k], whole[k], err_msg=k)
    np.testing.assert_array_equal(by_pair[k], whole[k], err_msg=k)
  with pytest.raises(_native.NativeError, match=r"window 0 of group 0: .* the limit is"):
    _native.summarize_draw_paths(draws, SCALE, SHIFT, obs, first, count, RANKS,
                                 max_bytes=tables + group + 1000)
  with pytest.raises(_native.NativeError, match=r"the tables alone take"):
    _native.summarize_draw_paths(draws, SCALE, SHIFT, obs, first, count, RANKS, max_bytes=100)


def test_float32_session_trajectories_give_the_session_routes_bits():
  """B = 3 series of a finished float32 session: its trajectories as float64 through the new entry are,
  output by output, what `Session.summarize_paths` computes from them where they are."""
  B, T, C_, S = 3, 67, 2, 35
  series = []
  for b in range(B):
    y, mask, X, _ = syn.standardize_for_sampler(*syn.make_raw_series(T, 1, 40 + 7 * b), int(0.7 * T))
    series.append((y, mask, X, _model.series_params(np.where(mask, np.nan, y), mask, X)))
  pb = _native.make_problem(T=T, P=2, has_slope=False, num_warmup=3, num_results=S, num_chains=C_,
                            num_series=B, seed=(5, 9))
  sess = _native.Session(pb, np.stack([s[0] for s in series]), np.stack([s[1] for s in series]),
                         np.stack([s[2] for s in series]), None, _native.make_params([s[3] for s in series]))
  _, obs, first, count = _inputs(T)
  ranks = [0, 34, 65, 66, 69]
  try:
    sess.run()
    traj = sess.fetch(["posterior_trajectories"])["posterior_trajectories"].reshape(B, C_ * S, T)
    want = sess.summarize_paths(SCALE, SHIFT, obs, first, count, ranks)
  finally:
    sess.close()
  assert traj.dtype == np.float32 and np.isfinite(traj).all() and traj.std() > 0
  got = _native.summarize_draw_paths(traj.astype(np.float64), SCALE, SHIFT, obs, first, count, ranks)
  for k in _native.PATH_OUTPUTS:
    np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_every_refusal_is_an_error_and_disturbs_no_later_call():
  T = 67
  draws, obs, first, count = _inputs(T)
  L = _native.load()
  fn = L.ci_summarize_draw_paths_f64
  ranks = np.asarray([0, N - 1], np.int32)
  out = np.zeros((G, 65, 2, 2))

  def raw(first_, count_, num_windows=None, num_ranks=2, num_groups=G, num_draws=N, scale=SCALE, shift=SHIFT,
          null=None, rk=ranks):
    fi = np.asarray(first_, np.int32)
    fi = np.ascontiguousarray(np.broadcast_to(fi, (G, fi.shape[-1])))
    co = np.ascontiguousarray(np.broadcast_to(np.asarray(count_, np.int32), fi.shape))
    sc, sh = np.asarray(scale, np.float64), np.asarray(shift, np.float64)
    args = dict(draws=draws.ctypes.data, scale=sc.ctypes.data, shift=sh.ctypes.data, observed=obs.ctypes.data,
                first=fi.ctypes.data, count=co.ctypes.data, ranks=rk.ctypes.data)
    if null:
      args[null] = None
    rc = fn(0, num_groups, num_draws, T, args["draws"], args["scale"], args["shift"], args["observed"],
            fi.shape[1] if num_windows is None else num_windows, args["first"], args["count"], num_ranks,
            args["ranks"], None, None, None, out.ctypes.data, None, None, None)
    return rc, L.ci_last_error().decode()

  for null in ("draws", "scale", "shift", "observed", "first", "count", "ranks"):
    rc, msg = raw([40], [27], null=null)
    assert rc != 0 and "NULL argument" in msg, null
  rc, msg = raw([40], [27], num_groups=0)
  assert rc != 0 and "num_groups must be >= 1, got 0" in msg
  rc, msg = raw([40], [27], num_draws=1)
  assert rc != 0 and "num_draws must be >= 2, got 1" in msg
  for num_windows in (0, 65):
    rc, msg = raw(np.zeros(65), np.zeros(65), num_windows=num_windows)
    assert rc != 0 and f"num_windows must be in [1, 64], got {num_windows}" in msg
  rc, msg = raw([[40, 3], [40, 3], [40, -1]], [[27, 3]] * 3)
  assert rc != 0 and "window 1 of group 2" in msg and "negative" in msg
  rc, msg = raw([[40, 3]] * 3, [[27, 3], [27, -2], [27, 3]])
  assert rc != 0 and "window 1 of group 1" in msg and "negative" in msg
  rc, msg = raw([[40, 50]] * 3, [[27, 18]] * 3)
  assert rc != 0 and "window 1 of group 0" in msg and "beyond the draws' 67 steps" in msg
  for num_ranks in (0, 9):
    rc, msg = raw([40], [27], num_ranks=num_ranks)
    assert rc != 0 and f"num_ranks must be in [1, 8], got {num_ranks}" in msg
  for bad in (N, -1):
    rc, msg = raw([40], [27], rk=np.asarray([0, bad], np.int32))
    assert rc != 0 and f"rank {bad} out of range [0, {N})" in msg
  rc, msg = raw([40], [27], scale=(1.0, np.inf, 1.0))
  assert rc != 0 and "the scale of group 1 is not finite" in msg
  rc, msg = raw([40], [27], shift=(1.0, 1.0, np.nan))
  assert rc != 0 and "the shift of group 2 is not finite" in msg
  with pytest.raises(ValueError, match="unknown path outputs"):
    _native.summarize_draw_paths(draws, SCALE, SHIFT, obs, first, count, RANKS, want=("centre",))
  with pytest.raises(ValueError, match=r"must be \[G, N, T\]"):
    _native.summarize_draw_paths(draws[0], 1.0, 0.0, obs[0], [40], [27], RANKS)
  # ... and the next call is the call it always was
  got = _native.summarize_draw_paths(draws, SCALE, SHIFT, obs, first, count, RANKS)
  _check(got, draws, obs, first, count, _host(T))


# ---- the public calls ---------------------------------------------------------------------------------
ALPHA, SEED = 0.05, (5, 11)
NUMERIC = ("critical_value", "max_excursion", "p")


def _assert_joint_equal(a: pd.DataFrame, b: pd.DataFrame, exact: bool, label=lambda x: x):
  """Two frames of joint bands or joint tables: the float columns within rtol 1e-10 / atol 1e-12 (the
  comparison of tests/test_gpu_aggregates.py for device against host frames) or bit for bit, every other
  column equal, missing where the other is; label: maps the labels of `b` (at, first_outside)."""
  assert list(a.columns) == list(b.columns) and len(a) == len(b)
  for c in a.columns:
    if a[c].dtype == np.float64:
      x, y = a[c].to_numpy(float), b[c].to_numpy(float)
      if exact:
        np.testing.assert_array_equal(x, y, err_msg=str(c))
      else:
        np.testing.assert_allclose(x, y, rtol=1e-10, atol=1e-12, equal_nan=True, err_msg=str(c))
    else:
      assert a[c].dtype == b[c].dtype, c
      x, y = list(a[c]), list(b[c])
      for u, v in zip(x, y):
        if pd.isna(u) or pd.isna(v):
          assert pd.isna(u) and pd.isna(v), (c, x, y)
        else:
          assert u == (label(v) if c in ("at", "first_outside") else v), (c, x, y)


class _Spy:
  """Records the one pool call of a one-launch fit with the trajectories of its session."""

  def __init__(self, patch, method):
    self.calls = []
    real = getattr(_native.Session, method)

    def spy(sess, scale, shift, groups, *rest):
      pb = sess.pb
      traj = sess.fetch(["posterior_trajectories"])["posterior_trajectories"]
      self.calls.append(dict(traj=traj.reshape(pb.num_series, -1, pb.T), scale=np.array(scale, np.float64),
                             shift=np.array(shift, np.float64), groups=groups))
      return real(sess, scale, shift, groups, *rest)

    patch.setattr(_native.Session, method, spy)


B, T_B, DRAWS = 6, 60, 70
PRE, POST = (0, 39), (40, 55)
NAMES = ["a", "b", "c", "d", "e", "f"]
AGGREGATES = {"all": "all", "west": {"a": 0.5, "c": -2.0, "d": 1.5}, "one": ["b"]}
GROUPS = [{b: 1.0 for b in range(B)}, {0: 0.5, 2: -2.0, 3: 1.5}, {1: 1.0}]
EFFECT_WINDOWS = {"early": (40, 46), "late": (47, 55)}
WINDOW_STEPS = ((40, 7), (47, 9))


def _values(seed=0):
  rng = np.random.default_rng(seed)
  x = rng.normal(size=(B, T_B, 2))
  y = (1.5 * x[:, :, 0] - 0.7 * x[:, :, 1] + 10.0 + 3.0 * np.arange(B)[:, None]
       + np.cumsum(0.1 * rng.normal(size=(B, T_B)), axis=1) + 0.3 * rng.normal(size=(B, T_B)))
  y[:, 40:48] += 1.5                                     # rises ...
  y[:, 48:56] -= 1.0                                     # ... and reverses
  v = np.concatenate([y[:, :, None], x], axis=2)
  v[3, 44, 0] = np.nan                                   # a missing outcome inside the post-period
  return v


def _fit_batch(joint_bands=True, devices=(0,), **kw):
  options = dict(num_results=DRAWS, num_chains=1, num_warmup_steps=10, devices=list(devices))
  options.update(kw.pop("options", {}))
  return ci.fit_causalimpact_batch(_values(), PRE, POST, alpha=ALPHA, seed=SEED, names=NAMES,
                                   inference_options=ci.InferenceOptions(**options), aggregates=AGGREGATES,
                                   effect_windows=EFFECT_WINDOWS, joint_bands=joint_bands, **kw)


@pytest.fixture(scope="module")
def fitted():
  with pytest.MonkeyPatch.context() as patch:
    spy = _Spy(patch, "pool_trajectories")
    res = _fit_batch()
  return res, spy


def _check_tables(res, aggregates, window_names):
  """Indices and dtypes of the two tables and of every group's frames."""
  paths = list(lib.JOINT_PATHS)
  table, by_window = res.aggregate_joint_summary, res.aggregate_window_joint_summary
  assert list(table.columns) == list(lib.JOINT_SUMMARY_COLUMNS) == list(by_window.columns)
  assert table.index.names == ["aggregate", None] and by_window.index.names == ["aggregate", "window", None]
  assert list(table.index) == [(a, p) for a in aggregates for p in paths]
  assert list(by_window.index) == [(a, w, p) for a in aggregates for w in window_names for p in paths]
  for name in aggregates:
    one = res.aggregates[name]
    assert list(one.joint_bands.columns) == list(lib.JOINT_BAND_COLUMNS)
    assert list(one.joint_bands.index) == list(one.series.index)
    _assert_joint_equal(table.loc[name], one.joint_summary, exact=True)
    _assert_joint_equal(by_window.loc[name], one.window_joint_summary, exact=True)
  for frame in (table, by_window):
    assert str(frame["n_outside"].dtype) == "Int64" and str(frame["significant"].dtype) == "boolean"
    assert frame["p"].dtype == np.float64


def test_batch_aggregate_frames_equal_the_host_arithmetic_on_numpy_pooled_draws(fitted):
  res, spy = fitted
  assert type(res) is ci.CausalImpactBatchAnalysis and len(spy.calls) == 1
  call = spy.calls[0]
  traj = call["traj"]
  assert traj.shape == (B, DRAWS, T_B) and call["groups"] == GROUPS
  pooled, observed = np.zeros((len(GROUPS), DRAWS, T_B)), np.zeros((len(GROUPS), T_B))
  prep = res._prep
  for g, group in enumerate(GROUPS):
    for b in sorted(group):
      pooled[g] = pooled[g] + group[b] * (traj[b].astype(np.float64) * call["scale"][b] + call["shift"][b])
      observed[g] = observed[g] + group[b] * prep.observed[b]
  assert np.isnan(observed[0, 44]) and np.isnan(observed[1, 44]) and not np.isnan(observed[2, :POST[1] + 1]).any()
  first = np.array([POST[0]] + [f for f, _ in WINDOW_STEPS], np.int32)
  count = np.array([POST[1] - POST[0] + 1] + [c for _, c in WINDOW_STEPS], np.int32)
  ranks = lib._path_ranks(DRAWS, ALPHA)
  host = lib._paths_record(_native.path_excursions_host(pooled, 1.0, 0.0, observed, first, count, ranks))
  _check_tables(res, AGGREGATES, list(EFFECT_WINDOWS))
  for g, name in enumerate(AGGREGATES):
    bands, summary, by_window = lib._joint_frames(
        {k: v[g] for k, v in host.items()}, ranks, DRAWS, ALPHA, observed[g], prep.index[prep.model_rows],
        prep.index, list(EFFECT_WINDOWS))
    got = res.aggregates[name]
    _assert_joint_equal(got.joint_bands, bands, exact=False)
    _assert_joint_equal(got.joint_summary, summary, exact=False)
    _assert_joint_equal(got.window_joint_summary, by_window, exact=False)
    assert got.joint_summary["critical_value"].notna().all()
    inside = got.joint_bands["posterior_lower"].notna()
    assert list(np.flatnonzero(inside)) == list(range(POST[0], POST[1] + 1))


def test_batch_group_of_one_series_is_that_series_bit_for_bit(fitted):
  res, _ = fitted
  own, got = res[1], res.aggregates["one"]
  assert own.joint_bands is not None and own.window_joint_summary is not None
  _assert_joint_equal(got.joint_bands, own.joint_bands, exact=True)
  _assert_joint_equal(got.joint_summary, own.joint_summary, exact=True)
  _assert_joint_equal(got.window_joint_summary, own.window_joint_summary, exact=True)
  _assert_joint_equal(res.aggregate_joint_summary.loc["one"], res.joint_summary.loc["b"], exact=True)


def test_batch_tables_do_not_depend_on_the_split_into_launches(fitted):
  res, _ = fitted
  two = _fit_batch(devices=(0, 0))
  pd.testing.assert_frame_equal(res.aggregate_joint_summary, two.aggregate_joint_summary, check_exact=True)
  pd.testing.assert_frame_equal(res.aggregate_window_joint_summary, two.aggregate_window_joint_summary,
                                check_exact=True)
  for name in AGGREGATES:
    pd.testing.assert_frame_equal(res.aggregates[name].joint_bands, two.aggregates[name].joint_bands,
                                  check_exact=True)


def test_batch_without_joint_bands_nothing_new_runs_and_no_frame_differs(fitted, monkeypatch):
  res, _ = fitted

  def refuse(*a, **k):
    raise AssertionError("summarize_draw_paths without joint_bands")

  monkeypatch.setattr(_native, "summarize_draw_paths", refuse)
  off = _fit_batch(joint_bands=False)
  assert off.aggregate_joint_summary is None and off.aggregate_window_joint_summary is None
  assert off.joint_summary is None and off.window_joint_summary is None
  for name in AGGREGATES:
    a, b = off.aggregates[name], res.aggregates[name]
    assert a.joint_bands is None and a.joint_summary is None and a.window_joint_summary is None
    pd.testing.assert_frame_equal(a.series, b.series, check_exact=True)
    pd.testing.assert_frame_equal(a.summary, b.summary, check_exact=True)
    pd.testing.assert_frame_equal(a.window_summary, b.window_summary, check_exact=True)
  for attr in ("summary", "window_summary", "aggregate_summary", "aggregate_window_summary"):
    pd.testing.assert_frame_equal(getattr(off, attr), getattr(res, attr), check_exact=True)
  for b in range(B):
    pd.testing.assert_frame_equal(off[b].series, res[b].series, check_exact=True)
    pd.testing.assert_frame_equal(off[b].summary, res[b].summary, check_exact=True)
  # ... and without aggregates the attributes stay None with joint_bands
  monkeypatch.undo()
  none = ci.fit_causalimpact_batch(_values(), PRE, POST, alpha=ALPHA, seed=SEED, names=NAMES, joint_bands=True,
                                   inference_options=ci.InferenceOptions(num_results=DRAWS, num_chains=1,
                                                                         num_warmup_steps=10))
  assert none.aggregates is None and none.aggregate_joint_summary is None
  assert none.aggregate_window_joint_summary is None and none.joint_summary is not None


def test_one_launch_hmc_batch_produces_the_tables():
  res = _fit_batch(options=dict(sampler="hmc", num_chains=2, num_results=25, num_warmup_steps=15))
  assert type(res) is ci.CausalImpactBatchAnalysis
  _check_tables(res, AGGREGATES, list(EFFECT_WINDOWS))
  assert res.aggregate_joint_summary["p"].notna().all()
  _assert_joint_equal(res.aggregates["one"].joint_bands, res[1].joint_bands, exact=True)
  _assert_joint_equal(res.aggregates["one"].joint_summary, res[1].joint_summary, exact=True)
  _assert_joint_equal(res.aggregates["one"].window_joint_summary, res[1].window_joint_summary, exact=True)


def test_float64_batch_on_the_per_series_route_produces_the_tables():
  """Fitted series by series and pooled in numpy; the member's own tables come from the host loop, the
  group's from the device: the tolerance of device against host frames."""
  v = _values()[:3]
  aggregates = {"all": "all", "one": ["b"]}
  res = ci.fit_causalimpact_batch(v, PRE, POST, alpha=ALPHA, seed=SEED, names=NAMES[:3], aggregates=aggregates,
                                  effect_windows=EFFECT_WINDOWS, joint_bands=True,
                                  data_options=ci.DataOptions(dtype=np.float64),
                                  inference_options=ci.InferenceOptions(num_results=DRAWS, num_chains=1,
                                                                        num_warmup_steps=10))
  assert isinstance(res, batch.PerSeriesBatchAnalysis)
  _check_tables(res, aggregates, list(EFFECT_WINDOWS))
  assert res.aggregate_joint_summary["p"].notna().all()
  _assert_joint_equal(res.aggregates["one"].joint_bands, res[1].joint_bands, exact=False)
  _assert_joint_equal(res.aggregates["one"].joint_summary, res[1].joint_summary, exact=False)
  _assert_joint_equal(res.aggregates["one"].window_joint_summary, res[1].window_joint_summary, exact=False)


# ---- a panel in event time ----------------------------------------------------------------------------
def _frame(num_rows, seed, start):
  """One covariate; the outcome steps up by 1 from row `start` on."""
  rng = np.random.default_rng(seed)
  x = rng.normal(size=num_rows)
  y = (1.5 * x + 10.0 + 3.0 * seed + np.cumsum(0.1 * rng.normal(size=num_rows))
       + 0.3 * rng.normal(size=num_rows))
  y[start:] += 1.0
  return pd.DataFrame({"y": y, "x0": x})


# four series of one steps-per-thread class, every one with its own length and periods: position 1
# drops 4 rows in front, leaves a gap of 3 and has a post-period of 18 rows, the others of 12 to 14;
# position 2 misses an outcome value inside its window
P_NAMES = ["n", "s", "e", "w"]
P_FRAMES = [_frame(48, 0, 36), _frame(66, 1, 45), _frame(55, 4, 40), _frame(52, 5, 38)]
P_FRAMES[2].iloc[44, 0] = np.nan
P_PERIODS = [((0, 35), (36, 47)), ((4, 41), (45, 62)), ((0, 39), (40, 51)), ((0, 37), (38, 51))]
P_AGGREGATES = {"all": "all", "pair": {"n": 0.5, "w": 1.5}, "one": ["s"]}
P_MEMBERS = [{b: 1.0 for b in range(4)}, {0: 0.5, 3: 1.5}, {1: 1.0}]
# in event time; only "one" (18 rows from its start on) reaches "far"
P_WINDOWS = {"early": (0, 5), "late": (6, 11), "far": (12, 17)}
P_DRAWS, P_CHAINS = 35, 2


def _fit_panel(joint_bands=True):
  return ci.fit_causalimpact_panel(
      P_FRAMES, P_PERIODS, alpha=ALPHA, seed=SEED, names=P_NAMES, event_aggregates=P_AGGREGATES,
      effect_windows=P_WINDOWS, joint_bands=joint_bands,
      inference_options=ci.InferenceOptions(num_results=P_DRAWS, num_chains=P_CHAINS, num_warmup_steps=10,
                                            devices=[0]))


@pytest.fixture(scope="module")
def panel():
  with pytest.MonkeyPatch.context() as patch:
    spy = _Spy(patch, "pool_event_trajectories")
    res = _fit_panel()
  return res, spy


def test_panel_aggregate_frames_equal_the_host_arithmetic_on_the_event_axis(panel):
  res, spy = panel
  assert len(spy.calls) == 1                                      # one class, one launch
  call, prep = spy.calls[0], res._prep
  N_ = P_DRAWS * P_CHAINS
  axes = batch.event_axes(prep, _native.groups_csr(P_MEMBERS, 4))
  ranks = lib._path_ranks(N_, ALPHA)
  _check_tables(res, P_AGGREGATES, list(P_WINDOWS))
  for g, (name, members, axis) in enumerate(zip(P_AGGREGATES, P_MEMBERS, axes)):
    width = axis.width
    pooled, observed = np.zeros((N_, width)), np.zeros(width)
    for b, f in zip(sorted(members), axis.first):
      value = call["traj"][b, :, f:f + width].astype(np.float64) * call["scale"][b] + call["shift"][b]
      pooled = pooled + members[b] * value
      observed = observed + members[b] * prep.observed[b, f:f + width]
    windows = [(axis.L, axis.Hwin)] + [(axis.L + lo, hi - lo + 1) if hi < axis.Hwin else (0, 0)
                                       for lo, hi in P_WINDOWS.values()]
    first, count = _tables([windows])
    host = lib._paths_record(_native.path_excursions_host(pooled[None], 1.0, 0.0, observed, first, count, ranks))
    index = pd.Index(np.arange(-axis.L, axis.H), name="event_time")
    bands, summary, by_window = lib._joint_frames({k: v[0] for k, v in host.items()}, ranks, N_, ALPHA,
                                                  observed, index, index, list(P_WINDOWS))
    got = res.aggregates[name]
    assert got.joint_bands.index.name == "event_time" and list(got.joint_bands.index) == list(index)
    _assert_joint_equal(got.joint_bands, bands, exact=False)
    _assert_joint_equal(got.joint_summary, summary, exact=False)
    _assert_joint_equal(got.window_joint_summary, by_window, exact=False)
    # a window beyond the group's axis: blank rows
    far = res.aggregate_window_joint_summary.loc[name].loc["far"]
    assert far.isna().all().all() == (name != "one"), name
    assert res.aggregate_window_joint_summary.loc[name].loc["early"]["p"].notna().all()
    labels = [x for x in got.joint_summary["at"] if x is not None]
    assert labels and all(0 <= x < axis.Hwin for x in labels)


def test_panel_group_of_one_series_is_that_series_with_labels_in_event_time(panel):
  res, _ = panel
  own, got = res[1], res.aggregates["one"]
  steps, start = 66 - 4, 45                               # the rows from its pre-period on; its treatment start
  assert len(got.joint_bands) == steps and list(got.joint_bands.index) == list(range(-41, 21))
  _assert_joint_equal(got.joint_bands, own.joint_bands.iloc[-steps:], exact=True)
  to_event_time = lambda row: row - start                 # pylint: disable=unnecessary-lambda-assignment
  _assert_joint_equal(got.joint_summary, own.joint_summary, exact=True, label=to_event_time)
  _assert_joint_equal(got.window_joint_summary, own.window_joint_summary, exact=True, label=to_event_time)
  assert got.window_joint_summary.loc["far"]["p"].notna().all()


def test_panel_without_joint_bands_no_frame_differs(panel):
  res, _ = panel
  off = _fit_panel(joint_bands=False)
  assert off.aggregate_joint_summary is None and off.aggregate_window_joint_summary is None
  for name in P_AGGREGATES:
    assert off.aggregates[name].joint_bands is None and off.aggregates[name].joint_summary is None
    pd.testing.assert_frame_equal(off.aggregates[name].series, res.aggregates[name].series, check_exact=True)
    pd.testing.assert_frame_equal(off.aggregates[name].summary, res.aggregates[name].summary, check_exact=True)
  for attr in ("summary", "window_summary", "aggregate_summary", "aggregate_window_summary"):
    pd.testing.assert_frame_equal(getattr(off, attr), getattr(res, attr), check_exact=True)
