"""ci_session_summarize_windows / ci_ll_session_summarize_windows on the device -- every draw's
totals over sub-windows of the steps -- at session level against `_native.window_totals_host` on the
trajectories fetched from the same session and against `Session.summarize` on the post-period, bit for
bit, and at package level (`effect_windows=`) across the routes.

T = 70 is one 64-step tile and a remainder, with rows that are not 16-byte aligned; C = 2, S = 37
gives N = 74 draws: one full wavefront of lanes and a remainder."""
import functools

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _model
from causalimpact import _native
from causalimpact import _synthetic as syn

pytestmark = pytest.mark.gpu

RANKS = [1, 2, 36, 71, 72]          # the ranks of a 95 % band over 74 draws, and the median
SCALE, SHIFT = (3.7, -0.5, 2.0), (-12.25, 4.0, 0.0)
# (first, count): the whole post-period, across the tile edge, single steps at the edge and at the
# end, an empty window, an overlapping one
WINDOWS = [(49, 21), (60, 9), (63, 1), (64, 1), (69, 1), (55, 0), (50, 15)]


def _series(T, P, seed, seasons):
  y, mask, X, _ = syn.standardize_for_sampler(*syn.make_raw_series(T, P - 1, seed), int(0.7 * T))
  if seasons:
    y = y + 0.8 * np.sin(2 * np.pi * np.arange(T) / 7.0)
  spec = _model.series_params(np.where(mask, np.nan, y), mask, X, num_seasonal_blocks=len(seasons))
  return y, mask, X, spec


def _pad(arrs, T, fill):
  out = np.full((len(arrs), T) + arrs[0].shape[1:], fill, arrs[0].dtype)
  for b, a in enumerate(arrs):
    out[b, :a.shape[0]] = a
  return out


def _open(lengths, seasons=(), ragged=False, C_=2, S=37, P=3):
  series = [_series(T, P, 40 + 7 * b, seasons) for b, T in enumerate(lengths)]
  T = max(lengths)
  if ragged and seasons:
    T = (T + 3) & ~3
  pb = _native.make_problem(T=T, P=P, has_slope=False, num_warmup=3, num_results=S, num_chains=C_,
                            num_series=len(lengths), seed=(5, 9),
                            num_seasons=_model.expand_seasons(seasons, 1)[0])
  y, mask = _pad([s[0] for s in series], T, np.nan), _pad([s[1] for s in series], T, True)
  X = _pad([s[2] for s in series], T, 7.5)                  # (padding rows are never read)
  par = _native.make_params([s[3] for s in series])
  sc = _model.expand_seasons(seasons, T)[1]
  if ragged:
    return _native.Session.ragged(pb, list(lengths), y, mask, X, par, season_change=sc if seasons else None), T
  return _native.Session(pb, y, mask, X, sc, par), T


def _observed(B, T, holes):
  obs = np.random.default_rng(17).normal(size=(B, T)) * 3.0 + 10.0
  for b, steps in enumerate(holes):
    obs[b, list(steps)] = np.nan
  return obs


@functools.lru_cache(maxsize=None)
def _run(lengths, windows, post, holes, seasons=(), ragged=False, C_=2, S=37):
  """One session: its fetched trajectories [B, N, T], `summarize_windows` of the per-series
  `windows`, `summarize` with the post-period `post` = per series (first, count), and the inputs."""
  sess, T = _open(lengths, seasons, ragged, C_, S)
  B = len(lengths)
  try:
    sess.run()
    traj = sess.fetch(["posterior_trajectories"])["posterior_trajectories"].reshape(B, C_ * S, T)
    obs = _observed(B, T, holes)
    first = np.array([[f for f, _ in ws] for ws in windows], np.int32)
    count = np.array([[c for _, c in ws] for ws in windows], np.int32)
    flags = np.zeros((B, T), np.uint8)
    for b, (f, c) in enumerate(post):
      flags[b, f:f + c] = 3
    got = sess.summarize_windows(SCALE[:B], SHIFT[:B], obs, first, count, RANKS)
    whole = sess.summarize(SCALE[:B], SHIFT[:B], obs, flags, RANKS)
    return traj, got, whole, obs, first, count, sess.kernel_name()
  finally:
    sess.close()


def _check(run, what):
  """Checks 1-3: the totals against the host loop on the fetched float32 trajectories, the order
  statistics against a sort, and window 0 (every series' whole post-period) against `summarize`."""
  traj, got, whole, obs, first, count, name = run
  B, N = traj.shape[:2]
  print(f"{what}: kernel {name}, trajectories {traj.shape}, windows {first.shape[1]}")
  assert traj.dtype == np.float32
  assert got["per_draw"].shape == (B, first.shape[1], 2, N)
  assert got["per_draw_order"].shape == (B, first.shape[1], 2, len(RANKS))
  want = _native.window_totals_host(traj, SCALE[:B], SHIFT[:B], obs, first, count)
  np.testing.assert_array_equal(got["per_draw"], want)
  np.testing.assert_array_equal(got["per_draw_order"], np.sort(got["per_draw"], axis=-1)[..., RANKS])
  np.testing.assert_array_equal(got["per_draw"][:, 0], whole["per_draw"])
  np.testing.assert_array_equal(got["per_draw_order"][:, 0], whole["per_draw_order"])
  empty = count == 0
  assert (got["per_draw"][empty] == 0.0).all() and (got["per_draw_order"][empty] == 0.0).all()
  assert not np.isnan(got["per_draw"]).any()


HOLES = ((52, 64),) * 3


def test_windows_equal_the_host_loop_and_the_post_period_equals_summarize():
  _check(_run((70, 70, 70), (tuple(WINDOWS),) * 3, ((49, 21),) * 3, HOLES), "N = 74")


def test_two_draw_tiles_and_a_remainder():
  _check(_run((70, 70, 70), (tuple(WINDOWS),) * 3, ((49, 21),) * 3, HOLES, C_=3, S=50), "N = 150")


def test_a_window_over_four_tiles():
  windows = ((49, 151), (3, 190), (60, 9), (199, 1), (55, 0), (128, 64))
  _check(_run((200, 200, 200), (windows,) * 3, ((49, 151),) * 3, HOLES), "T = 200")


def test_ragged_trend_session_takes_every_series_own_windows():
  windows = (((49, 21), (60, 9), (63, 1), (64, 1)), ((20, 13), (25, 5), (32, 1), (20, 0)),
             ((40, 24), (50, 14), (63, 1), (40, 1)))
  run = _run((70, 33, 64), windows, ((49, 21), (20, 13), (40, 24)), ((52, 64), (22, 32), (41, 63)), ragged=True)
  assert "ragged" in run[-1] and run[0].shape[2] == 70
  _check(run, "ragged trend")


def test_ragged_seasonal_session_reads_aligned_rows():
  """Stride 72: every row starts on a 16-byte boundary, the loads are four steps wide."""
  windows = (((49, 21), (60, 9), (63, 1), (64, 1), (61, 6)), ((20, 15), (25, 5), (34, 1), (20, 0), (21, 3)),
             ((40, 26), (50, 14), (63, 1), (64, 2), (47, 18)))
  run = _run((70, 35, 66), windows, ((49, 21), (20, 15), (40, 26)), ((52, 64), (22, 34), (41, 64)),
             seasons=((7, 1),), ragged=True)
  assert "ragged" in run[-1] and run[0].shape[2] == 72
  _check(run, "ragged seasonal")


def test_every_refusal_is_an_error_before_any_device_work():
  fn = _native.load().ci_session_summarize_windows
  sess, T = _open((70,))
  one, obs = np.ones(1), np.zeros((1, T))
  ranks = np.asarray([0, 73], np.int32)
  out = np.zeros((1, 1025, 2, 2))

  def raw(first, count, num_windows=None, num_ranks=2, scale=one, rk=ranks):
    first, count = np.asarray(first, np.int32), np.asarray(count, np.int32)
    rc = fn(sess._h, None if scale is None else scale.ctypes.data, one.ctypes.data, obs.ctypes.data,   # pylint: disable=protected-access
            first.size if num_windows is None else num_windows, first.ctypes.data, count.ctypes.data,
            num_ranks, rk.ctypes.data, None, out.ctypes.data)
    return rc, _native.load().ci_last_error().decode()

  try:
    with pytest.raises(_native.NativeError, match="needs a finished ci_session_run"):
      sess.summarize_windows(1.0, 0.0, obs, [49], [21], [0, 73])
    sess.run()
    rc, msg = raw([49], [21], scale=None)
    assert rc != 0 and "NULL argument" in msg
    for num_windows in (0, 1025):
      rc, msg = raw(np.zeros(1025), np.zeros(1025), num_windows=num_windows)
      assert rc != 0 and f"num_windows must be in [1, 1024], got {num_windows}" in msg
    rc, msg = raw([49, -1], [21, 3])
    assert rc != 0 and "window 1 of series 0" in msg and "negative" in msg
    rc, msg = raw([49, 50, 3], [21, 3, -2])
    assert rc != 0 and "window 2 of series 0" in msg and "negative" in msg
    rc, msg = raw([49, 50], [21, 21])
    assert rc != 0 and "window 1 of series 0" in msg and "beyond the session's 70 steps" in msg
    rc, msg = raw([2147483647], [2147483647])
    assert rc != 0 and "window 0 of series 0" in msg
    for num_ranks in (0, 9):
      rc, msg = raw([49], [21], num_ranks=num_ranks)
      assert rc != 0 and f"num_ranks must be in [1, 8], got {num_ranks}" in msg
    with pytest.raises(_native.NativeError, match=r"rank 74 out of range \[0, 74\)"):
      sess.summarize_windows(1.0, 0.0, obs, [49], [21], [0, 74])
    with pytest.raises(ValueError, match="`count` must have the shape of `first`"):
      sess.summarize_windows(1.0, 0.0, obs, [49, 50], [21], [0, 73])
    # ... and the session is as usable as before: the full width, the order statistics alone
    got = sess.summarize_windows(1.0, 0.0, obs, [0], [70], [0, 73], want_draws=False)
    assert list(got) == ["per_draw_order"] and got["per_draw_order"].shape == (1, 1, 2, 2)
  finally:
    sess.close()


# ---- package level: effect_windows= -------------------------------------------------------------------

ALPHA, SEED = 0.1, 11
OPTS = dict(num_chains=2, num_results=37)
HMC = dict(sampler="hmc", num_chains=2, num_results=25, num_warmup_steps=15)
NAMES = ["g0", "g1", "g2", "g3"]


def _frames(lengths, hole=True):
  idx = pd.date_range("2022-03-01", periods=max(lengths), freq="D")
  frames = []
  for b, Tb in enumerate(lengths):
    y, X = syn.make_raw_series(max(lengths), 1, 70 + b, effect=4.0 + b)
    frame = pd.DataFrame(np.column_stack([y, X]), index=idx, columns=["y", "x0"]).iloc[:Tb].copy()
    if hole:
      frame.iloc[9 + b, 0] = np.nan                     # a missing value inside the pre-period
    frames.append(frame)
  return frames


def _batch_setup():
  """Four series of 70 rows: a row before the pre-period, a gap of two, 24 post rows, a tail of one;
  series 1 misses an observation inside the post-period.  w1, w2 and rest partition the post-period."""
  frames = _frames((70,) * 4)
  frames[1].iloc[50, 0] = np.nan
  idx = frames[0].index
  windows = {"all": (idx[45], idx[68]), "w1": (idx[45], idx[52]), "w2": (idx[53], idx[60]),
             "rest": (idx[61], idx[68])}
  return frames, ((idx[1], idx[42]), (idx[45], idx[68])), windows


@functools.lru_cache(maxsize=None)
def _batch(**options):
  frames, periods, windows = _batch_setup()
  return ci.fit_causalimpact_batch(frames, *periods, alpha=ALPHA, seed=SEED, names=NAMES,
                                   inference_options=ci.InferenceOptions(**(options or OPTS)),
                                   aggregates={"all": "all"}, effect_windows=windows)


def _assert_all_window_is_the_summary(window_summary, summary):
  got = window_summary.xs("all", level="window")
  assert list(window_summary.columns) == list(summary.columns)
  pd.testing.assert_frame_equal(got, summary, check_exact=True, check_names=False)


def test_batch_windows_reproduce_the_summary_and_add_up():
  frames, _, windows = _batch_setup()
  got = _batch()
  assert type(got) is ci.CausalImpactBatchAnalysis             # (the one-launch route)
  table = got.window_summary
  assert table.index.names == ["series", "window", None] and len(table) == 4 * 4 * 2
  assert list(table.index.get_level_values("window").unique()) == list(windows)
  assert not table.isna().any().any()
  _assert_all_window_is_the_summary(table, got.summary)
  for b, name in enumerate(NAMES):
    pd.testing.assert_frame_equal(got[b].window_summary, table.xs(name, level="series"), check_exact=True)
    assert got[b].window_summary.index.names == ["window", None]
    # the cumulative rows of a partition add up, to the bound of re-associating a float64 sum of n
    # terms: n * 2^-52 * sum |terms| (abs_effect: the observations and the posterior means)
    post = got[b].series.loc[windows["all"][0]:windows["all"][1]]
    assert len(post) == 24
    obs_terms = np.nansum(np.abs(post["observed"].to_numpy()))
    all_terms = obs_terms + np.sum(np.abs(post["posterior_mean"].to_numpy()))
    parts = sum(table.loc[(name, w, "cumulative")] for w in ("w1", "w2", "rest"))
    whole = got.summary.loc[(name, "cumulative")]
    for col, terms in (("actual", obs_terms), ("abs_effect", all_terms)):
      bound = len(post) * 2.0 ** -52 * terms
      print(f"{name} {col}: parts - whole = {parts[col] - whole[col]:.3e}, bound {bound:.3e}")
      assert abs(parts[col] - whole[col]) <= bound, (name, col)
  # series 1 misses an observation in w1: one step fewer behind its average
  w1 = table.loc[("g1", "w1")]
  np.testing.assert_allclose(w1.loc["cumulative", "actual"], 7 * w1.loc["average", "actual"], rtol=1e-14)


def test_aggregate_windows_reproduce_the_aggregate_summary():
  got = _batch()
  table = got.aggregate_window_summary
  assert table.index.names == ["aggregate", "window", None] and len(table) == 4 * 2
  pd.testing.assert_frame_equal(table.xs("all", level="window"), got.aggregate_summary, check_exact=True,
                                check_names=False)
  pd.testing.assert_frame_equal(got.aggregates["all"].window_summary, table.loc["all"], check_exact=True)
  assert not table.isna().any().any()


PANEL_LENGTHS = (80, 55, 72)
PANEL_WINDOWS = {"w1": (0, 6), "w2": (7, 13), "all": (0, 29)}


def _panel_setup():
  """Own lengths and periods; 30 post rows, but 10 for series 1; b rows of tail, a gap of two, rows
  before the pre-period.

  The comparisons with `fit_causalimpact` below are exact, so the two routes must put the draws on
  the data scale with the same (sd, mean) of the pre-period outcome.  `prepare_panel` reduces a
  padded block along a strided axis and a series' own `Scaler` a column: in general their sums round
  in different orders and the statistics may differ in the last bit (`batch.scaler_stats`) -- with
  the data of an earlier version of this set-up the means of two of the three series did, by one unit
  in the last place, and so did `summary`.  Here no summation order can matter: the outcome lies on a
  grid of 1/64 below 2^10 and the pre-period has 33 rows of which 32 are observed, so the sum (21
  bits), the mean (a multiple of 2^-11), the deviations and the sum of their squares (47 bits) are
  all exact in float64."""
  frames = _frames(PANEL_LENGTHS, hole=False)
  periods, starts = [], []
  for b, frame in enumerate(frames):
    n_post = 10 if b == 1 else 30
    start = len(frame) - n_post - b
    idx = frame.index
    frame["y"] = np.round(frame["y"].to_numpy() * 64.0) / 64.0
    assert np.abs(frame["y"]).max() < 1024.0
    frame.iloc[start - 3 - 32 + 5 + b, 0] = np.nan       # a missing value inside the pre-period
    periods.append(((idx[start - 3 - 32], idx[start - 3]), (idx[start], idx[start + n_post - 1])))
    starts.append(start)
  return frames, periods, starts


@functools.lru_cache(maxsize=None)
def _panel(shared_streams=False):
  frames, periods, _ = _panel_setup()
  return ci.fit_causalimpact_panel(frames, periods, alpha=ALPHA, seed=SEED, shared_streams=shared_streams,
                                   inference_options=ci.InferenceOptions(**OPTS), effect_windows=PANEL_WINDOWS)


def test_panel_windows_in_event_time():
  got = _panel()
  assert type(got) is ci.CausalImpactPanelAnalysis
  table = got.window_summary
  assert len(table) == 3 * 3 * 2
  for b in (0, 2):
    pd.testing.assert_frame_equal(table.loc[(b, "all")], got.summary.loc[b], check_exact=True)
    assert not table.loc[b].isna().any().any()
  assert table.loc[(1, "w2")].isna().all().all() and table.loc[(1, "all")].isna().all().all()
  assert not table.loc[(1, "w1")].isna().any().any()
  assert got[1].window_summary.loc["w2"].isna().all().all()


def test_panel_with_shared_streams_equals_the_single_fits():
  frames, periods, starts = _panel_setup()
  got = _panel(shared_streams=True)
  for b, frame in enumerate(frames):
    covered = [w for w, (_, hi) in PANEL_WINDOWS.items() if hi < (10 if b == 1 else 30)]
    labels = {w: (frame.index[starts[b] + PANEL_WINDOWS[w][0]], frame.index[starts[b] + PANEL_WINDOWS[w][1]])
              for w in covered}
    one = ci.fit_causalimpact(frame, *periods[b], alpha=ALPHA, seed=SEED,
                              inference_options=ci.InferenceOptions(**OPTS), effect_windows=labels)
    pd.testing.assert_frame_equal(got[b].summary, one.summary, check_exact=True)   # (the README's promise)
    assert list(one.window_summary.index.get_level_values("window").unique()) == covered
    pd.testing.assert_frame_equal(got[b].window_summary.loc[covered], one.window_summary, check_exact=True)


def _single(windows=True, **options):
  frames, periods, all_windows = _batch_setup()
  data_options = ci.DataOptions(dtype=options.pop("dtype", np.float32))
  return ci.fit_causalimpact(frames[1], *periods, alpha=ALPHA, seed=SEED, data_options=data_options,
                             inference_options=ci.InferenceOptions(**options),
                             effect_windows=all_windows if windows else None)


def test_single_fit_on_the_device_agrees_with_the_host_postprocessing():
  dev, host = _single(**OPTS), _single(summarize_on_device=False, **OPTS)
  assert dev.window_summary.index.names == ["window", None] and len(dev.window_summary) == 4 * 2
  pd.testing.assert_frame_equal(dev.window_summary.loc["all"], dev.summary, check_exact=True)
  pd.testing.assert_frame_equal(host.window_summary.loc["all"], host.summary, check_exact=True)
  assert list(dev.window_summary.index) == list(host.window_summary.index)
  # the tolerance of tests/test_gpu_summary.py for `summary` between these two routes
  for c in dev.window_summary.columns:
    np.testing.assert_allclose(dev.window_summary[c].to_numpy(float), host.window_summary[c].to_numpy(float),
                               rtol=1e-10, atol=1e-12, err_msg=str(c))


@pytest.mark.parametrize("route", ["float64", "hmc"])
def test_single_fits_pooled_on_the_host_reproduce_their_summary(route):
  one = _single(dtype=np.float64, **OPTS) if route == "float64" else _single(**HMC)
  assert len(one.window_summary) == 4 * 2 and not one.window_summary.isna().any().any()
  pd.testing.assert_frame_equal(one.window_summary.loc["all"], one.summary, check_exact=True)


def test_one_launch_hmc_batch_reproduces_its_summary():
  got = _batch(**HMC)
  assert type(got) is ci.CausalImpactBatchAnalysis             # (ci_ll_session_summarize_windows)
  _assert_all_window_is_the_summary(got.window_summary, got.summary)
  pd.testing.assert_frame_equal(got.aggregate_window_summary.xs("all", level="window"), got.aggregate_summary,
                                check_exact=True, check_names=False)


def test_event_time_groups_take_the_windows_on_their_own_axis():
  """`event_aggregates`: the group of all three series has the short series' post-period of 10 rows,
  so w2 and all are not covered (NaN rows); the group of the two long ones covers everything."""
  frames, periods, _ = _panel_setup()
  got = ci.fit_causalimpact_panel(frames, periods, alpha=ALPHA, seed=SEED,
                                  inference_options=ci.InferenceOptions(**OPTS), effect_windows=PANEL_WINDOWS,
                                  event_aggregates={"every": "all", "long": [0, 2]})
  table = got.aggregate_window_summary
  assert table.index.names == ["aggregate", "window", None] and len(table) == 2 * 3 * 2
  pd.testing.assert_frame_equal(table.loc["long"].loc["all"], got.aggregate_summary.loc["long"], check_exact=True)
  assert not table.loc["long"].isna().any().any()
  assert table.loc["every"].loc["w2"].isna().all().all() and table.loc["every"].loc["all"].isna().all().all()
  assert not table.loc["every"].loc["w1"].isna().any().any()
  pd.testing.assert_frame_equal(got.window_summary, _panel().window_summary, check_exact=True)


def test_routes_fitted_series_by_series_stack_the_fits_own_tables():
  """A raw-scale panel (every window handed to the series' own fit as positions into its index) and
  a float64 batch with an aggregate: the host routes of `window_totals_host`."""
  frames, periods, _ = _panel_setup()
  got = ci.fit_causalimpact_panel(frames, periods, alpha=ALPHA, seed=SEED,
                                  data_options=ci.DataOptions(standardize_data=False),
                                  inference_options=ci.InferenceOptions(**OPTS), effect_windows=PANEL_WINDOWS)
  assert type(got).__name__ == "PerSeriesBatchAnalysis"
  table = got.window_summary
  assert table.index.names == ["series", "window", None] and len(table) == 3 * 3 * 2
  for b in (0, 2):
    pd.testing.assert_frame_equal(table.loc[b].loc["all"], got.summary.loc[b], check_exact=True)
    assert not table.loc[b].isna().any().any()
  assert table.loc[1].loc["w2"].isna().all().all() and table.loc[1].loc["all"].isna().all().all()
  assert not table.loc[1].loc["w1"].isna().any().any()
  pd.testing.assert_frame_equal(got[1].window_summary, table.loc[1], check_exact=True)
  frames, periods, windows = _batch_setup()
  got = ci.fit_causalimpact_batch(frames[:2], *periods, alpha=ALPHA, seed=SEED, names=NAMES[:2],
                                  data_options=ci.DataOptions(dtype=np.float64),
                                  inference_options=ci.InferenceOptions(**OPTS),
                                  aggregates={"all": "all"}, effect_windows=windows)
  assert type(got).__name__ == "PerSeriesBatchAnalysis"
  _assert_all_window_is_the_summary(got.window_summary, got.summary)
  pd.testing.assert_frame_equal(got.aggregate_window_summary.xs("all", level="window"), got.aggregate_summary,
                                check_exact=True, check_names=False)


def test_the_default_call_computes_nothing():
  frames, periods, _ = _batch_setup()
  got = ci.fit_causalimpact_batch(frames[:2], *periods, alpha=ALPHA, seed=SEED,
                                  inference_options=ci.InferenceOptions(**OPTS), aggregates={"all": "all"})
  assert got.window_summary is None and got.aggregate_window_summary is None
  assert got[0].window_summary is None and got.aggregates["all"].window_summary is None
  assert _single(windows=False, **OPTS).window_summary is None
