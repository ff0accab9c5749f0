"""`joint_bands=True` at package level: single fits, batches, panels and the one-launch HMC batch.
The option changes no other frame, alone or with every other feature on; `result[b]` of a batch is the
single fit of that series; the host routes agree with the device on the same draws."""
import functools

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import causalimpact_lib as lib
from causalimpact import _synthetic as syn

pytestmark = pytest.mark.gpu

ALPHA, SEED = 0.1, 11
OPTS = dict(num_chains=2, num_results=37)
HMC = dict(sampler="hmc", num_chains=2, num_results=25, num_warmup_steps=15)
NAMES = ["g0", "g1", "g2"]
FRAMES = ("series", "summary", "window_summary", "components", "coefficients", "prediction_errors",
          "fit_quality", "placebo", "placebo_quality")
TABLES = ("summary", "window_summary", "fit_quality", "placebo_quality")


def _frames(lengths):
  idx = pd.date_range("2022-03-01", periods=max(lengths), freq="D")
  frames = []
  for b, Tb in enumerate(lengths):
    y, X = syn.make_raw_series(max(lengths), 1, 70 + b, effect=4.0 + b)
    frame = pd.DataFrame(np.column_stack([y, X]), index=idx, columns=["y", "x0"]).iloc[:Tb].copy()
    frame.iloc[9 + b, 0] = np.nan                       # a missing value inside the pre-period
    frames.append(frame)
  return frames


def _batch_setup():
  """Three series of 70 rows: a row before the pre-period, a gap of two, 24 post rows, a tail of one;
  series 1 misses an observation inside the post-period."""
  frames = _frames((70,) * 3)
  frames[1].iloc[50, 0] = np.nan
  idx = frames[0].index
  windows = {"w1": (idx[45], idx[52]), "rest": (idx[53], idx[68])}
  return frames, ((idx[1], idx[42]), (idx[45], idx[68])), windows


def _panel_setup():
  frames = _frames((80, 55, 72))
  periods = []
  for b, frame in enumerate(frames):
    n_post = 10 if b == 1 else 30
    start, idx = len(frame) - n_post - b, frame.index
    periods.append(((idx[start - 35], idx[start - 3]), (idx[start], idx[start + n_post - 1])))
  return frames, periods, {"w1": (0, 6), "w2": (7, 13)}


def _everything(on):
  return dict(inference_options=ci.InferenceOptions(components=on, prediction_errors=on, **OPTS),
              placebo=True if on else None)


@functools.lru_cache(maxsize=None)
def _single(joint, everything=False, b=1, **options):
  frames, periods, windows = _batch_setup()
  if everything:
    kw = _everything(True)
  elif "dtype" not in options:
    kw = dict(inference_options=ci.InferenceOptions(**(options or OPTS)))
  else:
    kw = dict(inference_options=ci.InferenceOptions(**{k: v for k, v in options.items() if k != "dtype"}),
              data_options=ci.DataOptions(dtype=options["dtype"]))
  return ci.fit_causalimpact(frames[b], *periods, alpha=ALPHA, seed=SEED, effect_windows=windows,
                             joint_bands=joint, **kw)


@functools.lru_cache(maxsize=None)
def _batch(joint, everything=False, hmc=False, shared=False):
  frames, periods, windows = _batch_setup()
  kw = _everything(True) if everything else dict(inference_options=ci.InferenceOptions(**(HMC if hmc else OPTS)))
  return ci.fit_causalimpact_batch(frames, *periods, alpha=ALPHA, seed=SEED, names=NAMES, effect_windows=windows,
                                   shared_streams=shared, joint_bands=joint, **kw)


@functools.lru_cache(maxsize=None)
def _panel(joint, everything=False):
  frames, periods, windows = _panel_setup()
  kw = _everything(True) if everything else dict(inference_options=ci.InferenceOptions(**OPTS))
  return ci.fit_causalimpact_panel(frames, periods, alpha=ALPHA, seed=SEED, effect_windows=windows,
                                   joint_bands=joint, **kw)


def _assert_same(a, b, what):
  if a is None or b is None:
    assert a is None and b is None, what
  elif isinstance(a, pd.Series):
    pd.testing.assert_series_equal(a, b, check_exact=True, obj=what)
  else:
    pd.testing.assert_frame_equal(a, b, check_exact=True, obj=what)


def _assert_joint(one, num_draws, window_names, post_rows):
  bands, table = one.joint_bands, one.joint_summary
  assert tuple(bands.columns) == lib.JOINT_BAND_COLUMNS and bands.index.equals(one.series.index)
  assert tuple(table.columns) == lib.JOINT_SUMMARY_COLUMNS and tuple(table.index) == lib.JOINT_PATHS
  assert int(bands["posterior_lower"].notna().sum()) == post_rows
  inside = bands[bands["posterior_lower"].notna()]
  assert (inside["posterior_lower"] < inside["posterior_upper"]).all()
  # a simultaneous band holds the pointwise one
  pointwise = one.series.loc[inside.index]
  assert (inside["posterior_lower"] < pointwise["posterior_mean"]).all()
  assert (inside["posterior_upper"] > pointwise["posterior_mean"]).all()
  for path in lib.JOINT_PATHS:
    row = table.loc[path]
    assert 1.0 < row["critical_value"] < (num_draws - 1) / np.sqrt(num_draws)   # (the largest z of N values)
    assert 1.0 / (1 + num_draws) <= row["p"] <= 1.0 and row["at"] in inside.index
    assert bool(row["significant"]) == (row["max_excursion"] > row["critical_value"])
  assert bool(table.loc["pointwise", "significant"]) == bool(bands["outside"].any())
  assert table.loc["pointwise", "n_outside"] == bands["outside"].sum()
  if window_names:
    assert list(one.window_joint_summary.index.get_level_values("window").unique()) == list(window_names)


def test_single_fit_changes_no_other_frame_alone_or_with_everything_on():
  for everything in (False, True):
    on, off = _single(True, everything), _single(False, everything)
    for f in FRAMES:
      _assert_same(getattr(on, f), getattr(off, f), f)
    assert off.joint_bands is None and off.joint_summary is None and off.window_joint_summary is None
    _assert_joint(on, 74, ("w1", "rest"), 24)
  # the feature does not depend on the others either
  for f in ("joint_bands", "joint_summary", "window_joint_summary"):
    _assert_same(getattr(_single(True, True), f), getattr(_single(True, False), f), f)


@pytest.mark.parametrize("kind", ["batch", "panel", "hmc_batch"])
def test_launches_change_no_other_frame_alone_or_with_everything_on(kind):
  fit = {"batch": _batch, "panel": _panel, "hmc_batch": functools.partial(_batch, hmc=True)}[kind]
  for everything in ((False,) if kind == "hmc_batch" else (False, True)):
    on, off = fit(True, everything), fit(False, everything)
    assert type(on) is type(off) and "PerSeries" not in type(on).__name__
    for f in TABLES:
      _assert_same(getattr(on, f), getattr(off, f), f)
    assert off.joint_summary is None and off.window_joint_summary is None and off[0].joint_bands is None
    table = on.joint_summary
    assert table.index.names == ["series", None] and len(table) == 3 * 2
    wtable = on.window_joint_summary
    assert wtable.index.names == ["series", "window", None] and len(wtable) == 3 * 2 * 2
    for b in range(3):
      for f in FRAMES:
        _assert_same(getattr(on[b], f), getattr(off[b], f), f"{f} of series {b}")
      name = on._names[b]                                         # pylint: disable=protected-access
      _assert_same(on[b].joint_summary, table.loc[name], "joint_summary")
      _assert_same(on[b].window_joint_summary, wtable.loc[name], "window_joint_summary")
      post_rows = (10 if b == 1 else 30) if kind == "panel" else 24
      _assert_joint(on[b], 50 if kind == "hmc_batch" else 74, ("w1", "w2") if kind == "panel" else ("w1", "rest"),
                    post_rows)
    if kind == "panel":      # series 1 has 10 post rows: it covers w1 (0 .. 6) and not w2 (7 .. 13)
      assert wtable.loc[(1, "w2")][["critical_value", "max_excursion", "p"]].isna().all().all()
      assert wtable.loc[(1, "w1")][["critical_value", "max_excursion", "p"]].notna().all().all()
      assert wtable.loc[0][["critical_value", "max_excursion", "p"]].notna().all().all()


def _assert_close(got, want, what):
  """Bands to 1e-10 (what separates the batch's scaler from the single fit's), integers and labels equal."""
  assert list(got.columns) == list(want.columns) and got.index.equals(want.index), what
  for c in got.columns:
    if c in ("at", "first_outside", "n_outside", "significant", "outside"):
      assert got[c].isna().tolist() == want[c].isna().tolist(), (what, c)
      assert got[c].dropna().tolist() == want[c].dropna().tolist(), (what, c)
    else:
      np.testing.assert_allclose(got[c].to_numpy(float), want[c].to_numpy(float), rtol=1e-10, atol=1e-10,
                                 err_msg=f"{what} {c}")


def test_batch_with_shared_streams_equals_the_single_fits():
  got = _batch(True, shared=True)
  for b in range(3):
    one = _single(True, b=b)
    for f in ("joint_bands", "joint_summary", "window_joint_summary"):
      _assert_close(getattr(got[b], f), getattr(one, f), f"{f} of series {b}")


def test_host_route_on_the_same_draws_agrees_with_the_device():
  dev, host = _single(True), _single(True, summarize_on_device=False, **OPTS)
  for f in ("joint_bands", "joint_summary", "window_joint_summary"):
    _assert_close(getattr(host, f), getattr(dev, f), f)


@pytest.mark.parametrize("route", ["float64", "hmc"])
def test_routes_with_draws_of_their_own_have_the_shape_and_sane_values(route):
  one = _single(True, dtype=np.float64, **OPTS) if route == "float64" else _single(True, **HMC)
  _assert_joint(one, 74 if route == "float64" else 50, ("w1", "rest"), 24)
  assert one.window_joint_summary[["critical_value", "max_excursion", "p"]].notna().all().all()


def test_without_effect_windows_there_is_no_window_table():
  frames, periods, _ = _batch_setup()
  kw = dict(alpha=ALPHA, seed=SEED, inference_options=ci.InferenceOptions(**OPTS), joint_bands=True)
  one = ci.fit_causalimpact(frames[1], *periods, **kw)
  assert one.window_joint_summary is None and one.window_summary is None
  for f in ("joint_bands", "joint_summary"):
    _assert_same(getattr(one, f), getattr(_single(True), f), f)      # (the windows do not move the post-period's)
  got = ci.fit_causalimpact_batch(frames, *periods, names=NAMES, **kw)
  assert got.window_joint_summary is None and got[1].window_joint_summary is None
  _assert_same(got.joint_summary, _batch(True).joint_summary, "joint_summary")


def test_batch_fitted_series_by_series_stacks_the_fits_own_tables():
  frames, periods, windows = _batch_setup()
  got = ci.fit_causalimpact_batch(frames[:2], *periods, alpha=ALPHA, seed=SEED, names=NAMES[:2],
                                  data_options=ci.DataOptions(dtype=np.float64),
                                  inference_options=ci.InferenceOptions(**OPTS), effect_windows=windows,
                                  joint_bands=True)
  assert type(got).__name__ == "PerSeriesBatchAnalysis"
  assert got.joint_summary.index.names == ["series", None] and len(got.joint_summary) == 2 * 2
  assert got.window_joint_summary.index.names == ["series", "window", None] and len(got.window_joint_summary) == 2 * 2 * 2
  for b, name in enumerate(NAMES[:2]):
    _assert_same(got[b].joint_summary, got.joint_summary.loc[name], "joint_summary")
    _assert_same(got[b].window_joint_summary, got.window_joint_summary.loc[name], "window_joint_summary")
    _assert_joint(got[b], 74, ("w1", "rest"), 24)
  one = _single(True, b=0, dtype=np.float64, **OPTS)              # (series 0 of a batch is its single fit)
  for f in ("joint_bands", "joint_summary", "window_joint_summary"):
    _assert_same(getattr(got[0], f), getattr(one, f), f)
