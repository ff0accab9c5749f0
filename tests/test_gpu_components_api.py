"""`InferenceOptions(components=True)` through the public API: the `components` / `coefficients`
frames of `fit_causalimpact_batch` and `fit_causalimpact_panel` (which keep no draws: the frames
come from the device, csrc/ci_components.h) against `fit_causalimpact` on every series, and those
against numpy on the single fit's `posterior_samples`."""
import functools

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _synthetic as syn
from causalimpact import batch
from causalimpact import data as cid

pytestmark = pytest.mark.gpu

B, T, ALPHA, SEED = 3, 60, 0.1, 11
N = 2 * 40
OPTS = dict(num_results=40, num_chains=2)
WEEKLY = ci.ModelOptions(seasons=[ci.Seasons(num_seasons=7)])


def _frames(lengths=(T,) * B, weekly=False):
  idx = pd.date_range("2022-03-01", periods=T, freq="D")
  frames = []
  for b, Tb in enumerate(lengths):
    y, X = syn.make_raw_series(T, 2, 70 + b, effect=4.0 + b)
    if weekly:
      y = y + 3.0 * np.sin(2 * np.pi * (np.arange(T) + b) / 7.0)
    frames.append(pd.DataFrame(np.column_stack([y, X]), index=idx, columns=["y", "x0", "x1"]).iloc[:Tb])
  return frames


PERIODS = ((pd.Timestamp("2022-03-03"), pd.Timestamp("2022-04-11")),     # a row or two before the
           (pd.Timestamp("2022-04-13"), pd.Timestamp("2022-04-27")))     # pre-period, a gap, a tail


def _own_periods(frames):
  out = []
  for b, f in enumerate(frames):
    last_pre = (6 * len(f)) // 10 + b
    out.append(((f.index[1 + b], f.index[last_pre]), (f.index[last_pre + 2], f.index[len(f) - 1 - b])))
  return out


@functools.lru_cache(maxsize=None)
def _single(b, lengths=(T,) * B, weekly=False, own=False):
  frames = _frames(lengths, weekly)
  periods = _own_periods(frames)[b] if own else PERIODS
  return ci.fit_causalimpact(frames[b], *periods, alpha=ALPHA, seed=SEED,
                             model_options=WEEKLY if weekly else None,
                             inference_options=ci.InferenceOptions(components=True, **OPTS)), periods


def _tolerance(one, frame, periods):
  """A batch standardises all series in one vectorised pass, the single fit with its own scaler:
  mean and standard deviation of at most T values summed in another order, each within T 2^-53 of
  the exact value relatively, so (scale, shift) agree to T 2^-52.  A component x * scale + shift
  then moves by at most T 2^-52 (|x * scale| + |shift|) <= 2 T 2^-52 (peak + |shift|), `peak` the
  largest entry of the frame; the two roundings of the map and the interpolation of a band add a
  few 2^-53 of the same size.  Doubled once more for slack in the argument, not for the data."""
  data = cid.CausalImpactData(frame, *periods)
  shift = abs(float(np.ravel(data.outcome_scaler.mean_)[0]))
  peak = float(np.nanmax(np.abs(one.components.to_numpy())))
  return 4 * len(frame) * 2.0**-52 * (peak + shift)


def _assert_frames_equal_single(mine, one, frame, periods):
  assert list(mine.components.columns) == list(one.components.columns)
  assert mine.components.index.equals(one.components.index)
  assert mine.components.index.equals(mine.series.index)
  tol = _tolerance(one, frame, periods)
  got, want = mine.components.to_numpy(), one.components.to_numpy()
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
  err = np.nanmax(np.abs(got - want))
  print(f"components: largest difference {err:.3e}, tolerance {tol:.3e}")
  assert err <= tol
  # the weights live on the model's scale, which no scaler touches: equal draws, equal frames
  pd.testing.assert_frame_equal(mine.coefficients, one.coefficients, check_exact=True)


def _assert_single_equals_numpy(one, frame, periods, num_blocks):
  """The single fit's frames against numpy on its own draws (the definitions of
  include/causalimpact_amd.h): bands to 1e-12 relative -- both sides interpolate the same order
  statistics -- and means within N 2^-52 max|x|."""
  data = cid.CausalImpactData(frame, *periods)
  scale = float(np.ravel(data.outcome_scaler.stddev_)[0])
  shift = float(np.ravel(data.outcome_scaler.mean_)[0])
  ps = one.posterior_samples
  model_rows = one.components.index.isin(data.feature_ts.index)
  assert one.components[~model_rows].isna().all().all()
  comp = one.components[model_rows]
  q = (ALPHA / 2, 1 - ALPHA / 2)

  def check(prefix, m, frame_, names=("", "_lower", "_upper")):          # m [N, X]
    mean, lower, upper = (frame_[prefix + s].to_numpy() for s in names)
    bound = N * 2.0**-52 * np.abs(m).max(axis=0)
    print(f"{prefix or 'weights'}: largest mean error {np.abs(mean - m.mean(axis=0)).max():.3e}")
    assert (np.abs(mean - m.mean(axis=0)) <= bound).all(), prefix
    lo, hi = np.quantile(m, q, axis=0)
    np.testing.assert_allclose(lower, lo, rtol=1e-12, atol=0, err_msg=prefix)
    np.testing.assert_allclose(upper, hi, rtol=1e-12, atol=0, err_msg=prefix)

  level = np.asarray(ps.level, np.float32).astype(np.float64)
  assert level.shape == (N, len(comp))
  check("trend", level * scale + shift, comp)
  seasonal = np.asarray(ps.seasonal_levels, np.float32).astype(np.float64)
  assert seasonal.shape[-1] == num_blocks
  for k in range(num_blocks):
    check(f"seasonal_{k}", seasonal[:, :, k] * scale, comp)
  w = np.asarray(ps.weights, np.float32).astype(np.float64)
  X = data.feature_ts.to_numpy().astype(np.float32).astype(np.float64)
  acc = np.zeros((N, X.shape[0]))
  for j in range(w.shape[1]):
    acc += X[None, :, j] * w[:, j, None]
  check("regression", acc * scale, comp)
  expected = ["trend"] + [f"seasonal_{k}" for k in range(num_blocks)] + ["regression"]
  assert list(comp.columns) == [c + s for c in expected for s in ("", "_lower", "_upper")]
  coef = one.coefficients
  assert list(coef.index) == ["x0", "x1", "intercept_"]
  assert list(coef.columns) == ["inclusion_probability", "mean", "lower", "upper"]
  np.testing.assert_array_equal(coef["inclusion_probability"].to_numpy(),
                                np.count_nonzero(w, axis=0) / N)
  check("", w, coef, names=("mean", "lower", "upper"))


def test_batch_frames_equal_the_single_fits_and_numpy():
  frames = _frames()
  on = ci.fit_causalimpact_batch(frames, *PERIODS, alpha=ALPHA, seed=SEED, shared_streams=True,
                                 inference_options=ci.InferenceOptions(components=True, **OPTS))
  assert type(on) is ci.CausalImpactBatchAnalysis             # (the one-launch route)
  for b in range(B):
    one, periods = _single(b)
    _assert_frames_equal_single(on[b], one, frames[b], periods)
    _assert_single_equals_numpy(one, frames[b], periods, 0)
  # the option does not disturb what was there: the same table, and no frames without it
  off = ci.fit_causalimpact_batch(frames, *PERIODS, alpha=ALPHA, seed=SEED, shared_streams=True,
                                  inference_options=ci.InferenceOptions(**OPTS))
  pd.testing.assert_frame_equal(off.summary, on.summary, check_exact=True)
  for b in range(B):
    assert off[b].components is None and off[b].coefficients is None
    pd.testing.assert_frame_equal(off[b].series, on[b].series, check_exact=True)


@pytest.mark.parametrize("weekly", [False, True])
def test_panel_frames_equal_the_single_fits_and_numpy(weekly):
  """Lengths 60, 45 and 52 with their own periods: the ragged trend launch, and with Seasons(7)
  the ragged launch of the time-parallel kernel; every frame cut to the series' own index."""
  lengths = (60, 45, 52)
  frames = _frames(lengths, weekly)
  got = ci.fit_causalimpact_panel(frames, _own_periods(frames), alpha=ALPHA, seed=SEED,
                                  shared_streams=True, model_options=WEEKLY if weekly else None,
                                  inference_options=ci.InferenceOptions(components=True, **OPTS))
  assert type(got) is ci.CausalImpactPanelAnalysis
  for b in range(B):
    one, periods = _single(b, lengths, weekly, True)
    assert got[b].components.index.equals(frames[b].index)
    _assert_frames_equal_single(got[b], one, frames[b], periods)
    _assert_single_equals_numpy(one, frames[b], periods, 1 if weekly else 0)


def test_float64_batch_returns_the_frames_through_the_per_series_route():
  frames = _frames()
  kw = dict(alpha=ALPHA, seed=SEED, data_options=ci.DataOptions(dtype=np.float64),
            inference_options=ci.InferenceOptions(components=True, **OPTS))
  got = ci.fit_causalimpact_batch(frames, *PERIODS, shared_streams=True, **kw)
  assert type(got) is batch.PerSeriesBatchAnalysis
  for b in range(B):
    one = ci.fit_causalimpact(frames[b], *PERIODS, **kw)
    assert list(got[b].components.columns) == [
        "trend", "trend_lower", "trend_upper", "regression", "regression_lower", "regression_upper"]
    assert got[b].components.index.equals(got[b].series.index)
    pd.testing.assert_frame_equal(got[b].components, one.components, check_exact=True)
    pd.testing.assert_frame_equal(got[b].coefficients, one.coefficients, check_exact=True)
    # the same definitions in numpy on the float64 draws
    ps = one.posterior_samples
    data = cid.CausalImpactData(frames[b], *PERIODS)
    scale = float(np.ravel(data.outcome_scaler.stddev_)[0])
    shift = float(np.ravel(data.outcome_scaler.mean_)[0])
    rows = one.components.index.isin(data.feature_ts.index)
    trend = np.asarray(ps.level, np.float64) * scale + shift
    np.testing.assert_allclose(one.components["trend"][rows], trend.mean(axis=0), rtol=1e-13)
    np.testing.assert_allclose(one.components["trend_upper"][rows],
                               np.quantile(trend, 1 - ALPHA / 2, axis=0), rtol=1e-12)
    np.testing.assert_array_equal(one.coefficients["inclusion_probability"],
                                  np.count_nonzero(np.asarray(ps.weights), axis=0) / N)
