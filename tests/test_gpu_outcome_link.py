"""The outcome link on the device (ci_session_set_link, ci_session_value_mean; csrc/ci_link.h) and
`outcome_link=` at package level.

The element-wise exp / expm1 is the only place where device and numpy may differ: it is compared
with `_native.link_values_host` to 4 ulp (the OpenCL full-profile bound for double exp / expm1 is
3 ulp, plus 1 ulp for numpy's).  Everything downstream is compared bit for bit GIVEN the device's own
values v: a group of one member with weight 1 and no `init` makes `pool_trajectories` return
value[b, n, t] itself (0.0 + 1 * v), and the existing numpy definitions are applied to that.

Shapes as in tests/test_gpu_windows.py: T = 70 is one 64-step tile and a remainder, C = 2, S = 37
gives N = 74 draws, B = 3; an ordinary session, a ragged trend session of lengths (41, 70, 66) and a
ragged weekly-seasonal one (stride 72).  scale ~ (0.35, 0.2, 0.5) and shift ~ (4.0, 6.5, 0.1): the
trajectories are O(1), so nothing overflows."""
import functools
import json
import warnings

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _native

import test_gpu_joint_bands as joint
import test_gpu_windows as win

pytestmark = pytest.mark.gpu

RANKS = win.RANKS                   # the ranks of a 95 % band over 74 draws, and the median
SCALE, SHIFT = (0.35, 0.2, 0.5), (4.0, 6.5, 0.1)
LINKS = {"identity": _native.LINK_IDENTITY, "log": _native.LINK_LOG, "log1p": _native.LINK_LOG1P}
C_, S_ = 2, 37
N = C_ * S_
# per kind: lengths, seasons, ragged, per series the (first, count) windows -- window 0 the
# post-period, then test_gpu_windows.py's list on every series' own steps: across the tile edge, single
# steps at the edge and at the end, an empty window, an overlapping one -- and the steps without an
# observation, inside and outside the post-period
LONG = tuple(win.WINDOWS)
SHORT = ((28, 13), (30, 9), (31, 1), (32, 1), (40, 1), (35, 0), (29, 10))
MID = ((45, 21), (60, 6), (63, 1), (64, 1), (65, 1), (55, 0), (50, 15))
KINDS = {
    "ordinary": ((70, 70, 70), (), False, (LONG, LONG, LONG), ((5, 52, 64),) * 3),
    "ragged": ((41, 70, 66), (), True, (SHORT, LONG, MID), ((5, 30, 39), (5, 52, 64), (7, 47, 64))),
    "ragged_seasonal": ((41, 70, 66), ((7, 1),), True, (SHORT, LONG, MID),
                        ((5, 30, 39), (5, 52, 64), (7, 47, 64))),
}
SINGLE = [{0: 1.0}, {1: 1.0}, {2: 1.0}]
GROUPS = [{0: 1.5, 2: -0.25}, {0: 1.0, 1: 2.0, 2: 0.5}, {1: 1.0}]


def _observed(B, T, holes):
  obs = np.exp(np.random.default_rng(17).normal(size=(B, T)) * 0.4 + 4.0)      # positive
  for b, steps in enumerate(holes):
    obs[b, list(steps)] = np.nan
  return obs


def _event_groups(windows, weights):
  """Every group: its members from the first step of their own post-period on, 9 columns."""
  return [({b: (w, windows[b][0][0]) for b, w in group.items()}, 9) for group in weights]


def _calls(sess, obs, flags, first, count, windows):
  """Everything a session forms `value` for, under the link it has now."""
  out = dict(
      summarize=sess.summarize(SCALE, SHIFT, obs, flags, RANKS),
      windows=sess.summarize_windows(SCALE, SHIFT, obs, first, count, RANKS),
      paths=sess.summarize_paths(SCALE, SHIFT, obs, first, count, joint.RANKS),
      pool=sess.pool_trajectories(SCALE, SHIFT, GROUPS),
      event=sess.pool_event_trajectories(SCALE, SHIFT, _event_groups(windows, GROUPS)))
  return out


@functools.lru_cache(maxsize=None)
def _run(kind):
  """One session of `kind`: the fetched float32 trajectories [B, N, T], the inputs, and per link the
  device's own values v (singleton pools), `value_mean` and every call of `_calls`; under the identity
  three times: before any set_link, after set_link(identity), after set_link(log), set_link(identity)."""
  lengths, seasons, ragged, windows, holes = KINDS[kind]
  sess, T = win._open(lengths, seasons, ragged, C_, S_)          # pylint: disable=protected-access
  B = len(lengths)
  try:
    sess.run()
    traj = sess.fetch(["posterior_trajectories"])["posterior_trajectories"].reshape(B, N, T)
    obs = _observed(B, T, holes)
    first = np.array([[f for f, _ in ws] for ws in windows], np.int32)
    count = np.array([[c for _, c in ws] for ws in windows], np.int32)
    flags = np.zeros((B, T), np.uint8)
    for b, ws in enumerate(windows):
      flags[b, ws[0][0]:] = 1
      flags[b, ws[0][0]:ws[0][0] + ws[0][1]] = 3
    args = (obs, flags, first, count, windows)
    out = dict(traj=traj, obs=obs, flags=flags, first=first, count=count, windows=windows, T=T,
               name=sess.kernel_name(), before=_calls(sess, *args))
    sess.set_link(_native.LINK_IDENTITY)
    out["set_identity"] = _calls(sess, *args)
    sess.set_link(_native.LINK_LOG)
    sess.set_link(_native.LINK_IDENTITY)
    out["back_to_identity"] = _calls(sess, *args)
    for name, link in LINKS.items():
      sess.set_link(link)
      out[name] = dict(_calls(sess, *args), v=sess.pool_trajectories(SCALE, SHIFT, SINGLE),
                       value_mean=sess.value_mean(SCALE, SHIFT))
    return out
  finally:
    sess.close()


def _assert_same(a, b, what):
  if isinstance(a, dict):
    assert list(a) == list(b), what
    for k in a:
      _assert_same(a[k], b[k], f"{what}.{k}")
  else:
    np.testing.assert_array_equal(a, b, err_msg=what)


# ---- 1. the identity changes nothing ----------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(KINDS))
def test_identity_link_changes_no_bit(kind):
  run = _run(kind)
  for again in ("set_identity", "back_to_identity"):
    _assert_same(run["before"], run[again], again)
  # ... and it is the map of today: the singleton pool is the two-rounding z of the fetched trajectories
  z = run["traj"].astype(np.float64) * np.asarray(SCALE)[:, None, None] + np.asarray(SHIFT)[:, None, None]
  np.testing.assert_array_equal(run["identity"]["v"], 0.0 + 1.0 * z)


# ---- 2. the link itself ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("link", ["log", "log1p"])
def test_device_link_is_within_4_ulp_of_numpy(kind, link):
  run = _run(kind)
  z = run["traj"].astype(np.float64) * np.asarray(SCALE)[:, None, None] + np.asarray(SHIFT)[:, None, None]
  want = _native.link_values_host(z, LINKS[link])
  got = run[link]["v"]
  assert got.shape == want.shape == (3, N, run["T"]) and np.isfinite(want).all()
  ulps = np.abs(got - want) / np.spacing(np.abs(want))
  print("outcome_link ulp:", json.dumps(dict(test="link_ulp", kind=kind, link=link, values=int(want.size),
                                             max_ulp=float(ulps.max()), differing=int((ulps > 0).sum()))))
  assert ulps.max() <= 4.0
  if link == "log":
    assert (got > 0.0).all()


# ---- 3. everything downstream, bit for bit, given the device's own values ----------------------------------

def _summary_host(v, obs, flags, ranks):
  """`Session.summarize` in numpy on data-scale values v [B, N, T]: the sort at the ranks, the sequential
  running sums with the NaN steps skipped and reported NaN, the per-draw totals over the window."""
  B, n, T = v.shape
  point = -(v - obs[:, None, :])
  base = np.where((flags & 1)[:, None, :] != 0, point, 0.0)
  hole = np.isnan(base)
  cum = np.cumsum(np.where(hole, 0.0, base), axis=2)             # (sequential along t)
  cum[hole] = np.nan
  per_draw = np.zeros((B, 2, n))
  for b in range(B):
    for t in np.flatnonzero(flags[b] & 2):
      per_draw[b, 0] = per_draw[b, 0] + v[b, :, t]
      p = point[b, :, t]
      per_draw[b, 1] = np.where(p == p, per_draw[b, 1] + p, per_draw[b, 1])
  return dict(value_order=np.sort(v, axis=1)[:, ranks, :], cum_order=np.sort(cum, axis=1)[:, ranks, :],
              per_draw=per_draw, per_draw_order=np.sort(per_draw, axis=2)[:, :, ranks])


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("link", list(LINKS))
def test_summarize_and_value_mean_from_the_device_values(kind, link):
  run = _run(kind)
  got, v = run[link], run[link]["v"]
  want = _summary_host(v, run["obs"], run["flags"], RANKS)
  for k, a in want.items():
    np.testing.assert_array_equal(got["summarize"][k], a, err_msg=k)
  # the header's bound for means: N * 2^-52 * max |v| of the row
  err = np.abs(got["value_mean"] - v.mean(axis=1))
  bound = N * 2.0 ** -52 * np.abs(v).max(axis=1)
  print(f"{kind} {link}: value_mean max error {err.max():.3e}, bound {bound.min():.3e} ..")
  assert got["value_mean"].shape == (3, run["T"]) and (err <= bound).all()


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("link", list(LINKS))
def test_windows_from_the_device_values(kind, link):
  run = _run(kind)
  got, v = run[link]["windows"], run[link]["v"]
  want = _native.window_totals_host(v, 1.0, 0.0, run["obs"], run["first"], run["count"])
  np.testing.assert_array_equal(got["per_draw"], want)
  np.testing.assert_array_equal(got["per_draw_order"], np.sort(got["per_draw"], axis=-1)[..., RANKS])
  # window 0 is every series' post-period: `summarize`'s totals, bit for bit
  np.testing.assert_array_equal(got["per_draw"][:, 0], run[link]["summarize"]["per_draw"])
  np.testing.assert_array_equal(got["per_draw_order"][:, 0], run[link]["summarize"]["per_draw_order"])
  assert (got["per_draw"][run["count"] == 0] == 0.0).all()


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("link", list(LINKS))
def test_paths_from_the_device_values(kind, link):
  """As tests/test_gpu_joint_bands.py compares the identity route: the moments to the summation error
  of N draws, everything else bit for bit given the device's moments."""
  run = _run(kind)
  got, v = run[link]["paths"], run[link]["v"]
  own = _native.path_excursions_host(v, 1.0, 0.0, run["obs"], run["first"], run["count"], joint.RANKS)
  for k in ("center", "spread"):
    np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(own[k]), err_msg=k)
  with np.errstate(all="ignore"), warnings.catch_warnings():
    warnings.simplefilter("ignore", RuntimeWarning)
    big = np.nanmax(np.abs(own["x"]), axis=3)
  there = ~np.isnan(own["center"])
  assert (np.abs(got["center"] - own["center"])[there] <= 1e-10 * big[there]).all()
  assert ((np.abs(got["spread"] - own["spread"]) / own["spread"])[there] <= 1e-10).all()
  want = _native.path_excursions_host(v, 1.0, 0.0, run["obs"], run["first"], run["count"], joint.RANKS,
                                      center=got["center"], spread=got["spread"])
  for k in joint.BITWISE:
    np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("link", list(LINKS))
def test_pools_from_the_device_values(kind, link):
  run = _run(kind)
  v = run[link]["v"]
  np.testing.assert_array_equal(run[link]["pool"], _native.pool_host(v, 1.0, 0.0, GROUPS))
  np.testing.assert_array_equal(run[link]["event"],
                                _native.pool_event_host(v, 1.0, 0.0, _event_groups(run["windows"], GROUPS)))


def _ordinary(positions):
  """The ordinary session of `_run("ordinary")` cut to the consecutive `positions`: the same series on
  the same streams (keyed by series_offset + b)."""
  series = [win._series(70, 3, 40 + 7 * b, ()) for b in positions]          # pylint: disable=protected-access
  pb = _native.make_problem(T=70, P=3, has_slope=False, num_warmup=3, num_results=S_, num_chains=C_,
                            num_series=len(positions), seed=(5, 9), series_offset=positions[0])
  return _native.Session(pb, np.stack([s[0] for s in series]), np.stack([s[1] for s in series]),
                         np.stack([s[2] for s in series]), None, _native.make_params([s[3] for s in series]))


@pytest.mark.parametrize("link", ["log", "log1p"])
def test_a_pool_cut_into_two_sessions_equals_the_uncut_pool(link):
  whole = _run("ordinary")[link]
  first, second = _ordinary([0, 1]), _ordinary([2])
  try:
    for sess in (first, second):
      sess.set_link(LINKS[link])
      sess.run()
    part = first.pool_trajectories(SCALE[:2], SHIFT[:2], [{0: 1.5}, {0: 1.0, 1: 2.0}, {1: 1.0}])
    both = second.pool_trajectories(SCALE[2:], SHIFT[2:], [{0: -0.25}, {0: 0.5}, {}], init=part)
    np.testing.assert_array_equal(both, whole["pool"])
    windows = KINDS["ordinary"][3]
    groups = _event_groups(windows, GROUPS)
    part = first.pool_event_trajectories(SCALE[:2], SHIFT[:2], [
        ({b: m for b, m in members.items() if b < 2}, width) for members, width in groups])
    both = second.pool_event_trajectories(SCALE[2:], SHIFT[2:], [
        ({b - 2: m for b, m in members.items() if b >= 2}, width) for members, width in groups], init=part)
    np.testing.assert_array_equal(both, whole["event"])
  finally:
    first.close()
    second.close()


# ---- 4. errors ---------------------------------------------------------------------------------------------

def test_refusals():
  sess, _ = win._open((70,), (), False, C_, S_)                  # pylint: disable=protected-access
  try:
    with pytest.raises(_native.NativeError, match="unknown link 7"):
      sess.set_link(7)
    with pytest.raises(_native.NativeError, match="unknown link -1"):
      sess.set_link(-1)
    sess.set_link(_native.LINK_LOG)                              # (any time after create)
    with pytest.raises(_native.NativeError, match="needs a finished ci_session_run"):
      sess.value_mean(1.0, 0.0)
    sess.run()
    assert sess.value_mean(0.5, 1.0).shape == (1, 70)
  finally:
    sess.close()


# ---- 5. package level --------------------------------------------------------------------------------------

ALPHA, SEED = 0.1, (5, 11)
OPTS = dict(num_chains=2, num_results=37)
NAMES = ["g0", "g1", "g2", "g3"]
RTOL, ATOL = 1e-10, 1e-12        # the device-vs-host tolerance of the existing frame tests


def _frames(lengths=(100,) * 4):
  """Positive outcomes with a multiplicative lift of 25 % from row T - 28 on, one covariate."""
  idx = pd.date_range("2022-03-01", periods=max(lengths), freq="D")
  frames = []
  for b, Tb in enumerate(lengths):
    rng = np.random.default_rng(300 + b)
    x = rng.normal(size=Tb).cumsum() * 0.1 + 3.0
    y = np.exp(4.0 + 0.2 * b + 0.3 * x + 0.05 * rng.normal(size=Tb))
    y[Tb - 28:] *= 1.25
    frames.append(pd.DataFrame({"y": y, "x0": x}, index=idx[:Tb]))
  return frames


def _setup():
  frames = _frames()
  frames[0].iloc[11, 0] = np.nan                          # a missing value inside the pre-period
  frames[1].iloc[80, 0] = np.nan                          # ... and one inside the post-period
  idx = frames[0].index
  windows = {"all": (idx[72], idx[97]), "w1": (idx[72], idx[79]), "rest": (idx[80], idx[97])}
  return frames, ((idx[1], idx[69]), (idx[72], idx[97])), windows


@functools.lru_cache(maxsize=None)
def _single(on_device=True, link="log"):
  frames, periods, windows = _setup()
  return ci.fit_causalimpact(frames[0], *periods, alpha=ALPHA, seed=SEED, effect_windows=windows,
                             inference_options=ci.InferenceOptions(summarize_on_device=on_device, **OPTS),
                             outcome_link=link)


@functools.lru_cache(maxsize=None)
def _hand_logged(keep_draws=False):
  """The fit of the user's own log y with the same seed; keep_draws: (the fit, its predictive draws z
  [N, T] on the log scale), through the sink the per-series batch routes read them with."""
  frames, periods, _ = _setup()
  frame = frames[0].copy()
  frame["y"] = np.log(frame["y"])
  caught = {}
  kw = dict(_trajectory_sink=lambda m, tr, sc, sh: caught.update(z=np.asarray(tr, np.float64) * sc + sh)) if keep_draws else {}
  got = ci.fit_causalimpact(frame, *periods, alpha=ALPHA, seed=SEED,
                            inference_options=ci.InferenceOptions(**OPTS), **kw)
  return (got, caught["z"]) if keep_draws else got


def _assert_frames_close(a: pd.DataFrame, b: pd.DataFrame, what):
  assert list(a.columns) == list(b.columns) and a.index.equals(b.index), what
  for c in a.columns:
    if pd.api.types.is_numeric_dtype(a[c]):
      np.testing.assert_allclose(a[c].to_numpy(float), b[c].to_numpy(float), rtol=RTOL, atol=ATOL,
                                 err_msg=f"{what}: {c}")
    else:
      assert (a[c] == b[c]).all(), (what, c)


def test_single_fit_on_the_device_agrees_with_the_host_route():
  frames, _, _ = _setup()
  dev, host = _single(True), _single(False)
  for name in ("series", "summary", "window_summary"):
    _assert_frames_close(getattr(dev, name), getattr(host, name), name)
  pd.testing.assert_frame_equal(dev.window_summary.loc["all"], dev.summary, check_exact=True)
  for got in (dev, host):
    np.testing.assert_array_equal(got.series["observed"].to_numpy(), frames[0]["y"].to_numpy())
  # a 25 % lift on the data scale, not 0.22 in log units
  assert 0.1 < dev.summary.loc["average", "rel_effect"] < 0.5
  assert dev.summary.loc["average", "actual"] > 50.0


def test_the_model_is_that_of_the_hand_logged_frame_and_the_mean_is_of_the_linked_draws():
  linked, plain = _single(True), _hand_logged()
  _, z = _hand_logged(keep_draws=True)
  for f in ("observation_noise_scale", "level_scale", "level", "weights"):
    np.testing.assert_array_equal(getattr(linked.posterior_samples, f), getattr(plain.posterior_samples, f), err_msg=f)
  # Jensen: the mean of exp(draws) lies strictly above exp(mean of the draws), at every step
  mean = linked.series["posterior_mean"].to_numpy()[1:]    # (the model's steps: row 0 lies before the pre-period)
  assert z.shape == (N, mean.shape[0])
  assert (mean > np.exp(z.mean(axis=0))).all()
  np.testing.assert_allclose(mean, np.exp(z).mean(axis=0), rtol=1e-9)


def test_log1p_single_fit_agrees_with_the_host_route():
  dev, host = _single(True, "log1p"), _single(False, "log1p")
  for name in ("series", "summary", "window_summary"):
    _assert_frames_close(getattr(dev, name), getattr(host, name), name)


@functools.lru_cache(maxsize=None)
def _batch(devices=(0,)):
  frames, periods, windows = _setup()
  return ci.fit_causalimpact_batch(
      frames, *periods, alpha=ALPHA, seed=SEED, names=NAMES, effect_windows=windows, outcome_link="log",
      inference_options=ci.InferenceOptions(devices=list(devices), **OPTS),
      aggregates={"solo": ["g0"], "pair": {"g1": 1.0, "g2": 2.0}})


def test_batch_series_and_aggregates():
  frames, _, _ = _setup()
  got, one = _batch(), _single(True)
  assert type(got) is ci.CausalImpactBatchAnalysis             # (the one-launch route)
  # series 0 draws from the streams of the single fit.  Its own scaler and the batch's vectorised one
  # may differ in the last bit (`batch.scaler_stats`), which moves z by an ulp: the device-vs-host
  # tolerance, not bit equality
  _assert_frames_close(got[0].series, one.series, "series 0")
  _assert_frames_close(got[0].summary, one.summary, "summary 0")
  _assert_frames_close(got[0].window_summary, one.window_summary, "window_summary 0")
  _assert_frames_close(got.summary.loc["g0"], one.summary, "table row 0")
  for b, frame in enumerate(frames):
    np.testing.assert_array_equal(got[b].series["observed"].to_numpy(), frame["y"].to_numpy())
  # a group of one series with weight 1 has that series' own frames
  solo = got.aggregates["solo"]
  numeric = [c for c in solo.series.columns if pd.api.types.is_numeric_dtype(solo.series[c])]
  _assert_frames_close(solo.series[numeric], got[0].series[numeric], "solo series")
  _assert_frames_close(solo.summary, got[0].summary, "solo summary")
  _assert_frames_close(solo.window_summary, got[0].window_summary, "solo window_summary")
  # a pooled draw is the weighted sum of the members' linked draws: so is its expected total
  pair = got.aggregate_summary.loc[("pair", "cumulative"), "predicted"]
  members = (got.summary.loc[("g1", "cumulative"), "predicted"] + 2.0 * got.summary.loc[("g2", "cumulative"), "predicted"])
  np.testing.assert_allclose(pair, members, rtol=1e-10)
  pd.testing.assert_frame_equal(got.aggregate_window_summary.xs("all", level="window"), got.aggregate_summary,
                                check_exact=True, check_names=False)


def test_batch_does_not_depend_on_the_split_into_launches():
  one, two = _batch(), _batch((0, 0))
  pd.testing.assert_frame_equal(one.summary, two.summary, check_exact=True)
  pd.testing.assert_frame_equal(one.window_summary, two.window_summary, check_exact=True)
  pd.testing.assert_frame_equal(one.aggregate_summary, two.aggregate_summary, check_exact=True)
  for name in ("solo", "pair"):
    pd.testing.assert_frame_equal(one.aggregates[name].series, two.aggregates[name].series, check_exact=True)
  pd.testing.assert_frame_equal(one[3].series, two[3].series, check_exact=True)


def test_panel_with_event_aggregates_agrees_with_the_single_fits():
  """Lengths in two classes of the ragged route (<= 256 steps, 512); every series equals
  `fit_causalimpact` on its own frame with the key of its position, as tests/test_gpu_panel.py
  compares them -- here to the device-vs-host tolerance, for the scaler's last bit."""
  frames = _frames((100, 300, 90))
  periods = []
  for frame in frames:
    idx, Tb = frame.index, len(frame)
    periods.append(((idx[2], idx[Tb - 31]), (idx[Tb - 28], idx[Tb - 1])))
  got = ci.fit_causalimpact_panel(frames, periods, alpha=ALPHA, seed=SEED, outcome_link="log",
                                  inference_options=ci.InferenceOptions(**OPTS),
                                  event_aggregates={"every": "all", "first": [0]})
  assert type(got) is ci.CausalImpactPanelAnalysis
  for b, frame in enumerate(frames):
    one = ci.fit_causalimpact(frame, *periods[b], alpha=ALPHA, outcome_link="log",
                              seed=_native.series_stream_key(SEED, b),
                              inference_options=ci.InferenceOptions(**OPTS))
    _assert_frames_close(got[b].summary, one.summary, f"summary {b}")
    _assert_frames_close(got[b].series, one.series, f"series {b}")
    np.testing.assert_array_equal(got[b].series["observed"].to_numpy(), frame["y"].to_numpy())
  first = got.aggregates["first"]
  _assert_frames_close(first.summary, got[0].summary, "group of one")
  every = got.aggregate_summary.loc[("every", "cumulative"), "predicted"]
  assert every > got.summary.loc[(0, "cumulative"), "predicted"] > 0.0
