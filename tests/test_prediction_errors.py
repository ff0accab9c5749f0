"""InferenceOptions(prediction_errors=True) without a GPU: `_prediction_summary_host` against the
float64 oracle's Kalman filter, the frames built from a summary, the option's defaults and the
refusal of a state the filter does not take."""
import dataclasses

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _model
from causalimpact import batch
from causalimpact import causalimpact_lib as lib
from oracle import ci_oracle as orc


def _case(T, P, has_slope, seasons, seed=0, num_draws=20):
  """A series whose last 30 % and steps 11, 12, 40 are masked, and `num_draws` random parameter rows
  rounded to float32, as the sampler stores them."""
  rng = np.random.default_rng(seed)
  y = np.cumsum(rng.normal(scale=0.1, size=T)) + rng.normal(scale=0.3, size=T)
  X = np.concatenate([rng.normal(size=(T, P - 1)), np.ones((T, 1))], axis=1) if P else None
  mask = np.zeros(T, bool)
  mask[int(0.7 * T):] = True
  mask[[11, 12, 40]] = True
  spec = orc.default_spec(y, mask, X, has_slope=has_slope, seasons=seasons)
  K = len(seasons)
  f32 = lambda a: a.astype(np.float32)
  draws = dict(observation_noise_scale=f32(rng.uniform(0.1, 0.6, num_draws)),
               level_scale=f32(rng.uniform(0.01, 0.2, num_draws)),
               slope_scale=f32(rng.uniform(0.001, 0.02, num_draws)),
               seasonal_drift_scales=f32(rng.uniform(0.01, 0.1, (num_draws, K))),
               weights=f32(rng.normal(scale=0.3, size=(num_draws, P)) * (rng.random((num_draws, P)) < 0.6)))
  return y, mask, X, spec, draws


@pytest.mark.parametrize("T,P,has_slope,seasons", [
    (70, 3, False, ()), (70, 0, False, ()), (70, 3, True, ()), (70, 0, True, ()),
    (133, 4, False, ((7, 1),)), (133, 4, False, ((4, 2),)),
])
def test_host_summary_matches_the_oracle(T, P, has_slope, seasons):
  """Per draw, loglik == oracle.kalman_loglik(ssm of the draw, y - X w) to rtol 1e-8: a numpy
  transcription of the recursion reproduces the oracle to 8e-16 relative on these shapes and two
  orderings of its covariance update differ by at most 2e-12, four orders below the tolerance."""
  y, mask, X, spec, draws = _case(T, P, has_slope, seasons)
  num_seasons, season_change = _model.expand_seasons(seasons, T)
  ranks = [0, 9, 19]
  got = lib._prediction_summary_host(y, mask, X, season_change, num_seasons, has_slope, spec, draws,
                                     2.5, -3.0, ranks)
  want = np.zeros(20)
  for n in range(20):
    ssm = orc.make_ssm(spec, mask, obs_scale=draws["observation_noise_scale"][n],
                       level_scale=draws["level_scale"][n],
                       slope_scale=draws["slope_scale"][n] if has_slope else 0.0,
                       drift_scale=draws["seasonal_drift_scales"][n])
    resid = y - (X @ draws["weights"][n].astype(np.float64) if P else 0.0)
    want[n] = orc.kalman_loglik(ssm, np.where(mask, 0.0, resid))
  print("largest relative deviation of loglik:", np.max(np.abs(got["loglik"] - want) / np.abs(want)))
  np.testing.assert_allclose(got["loglik"], want, rtol=1e-8)
  assert got["forecast_mean"].shape == got["variance_mean"].shape == got["pit_mean"].shape == (T,)
  assert got["forecast_order"].shape == (3, T)
  assert (np.diff(got["forecast_order"], axis=0) >= 0).all()
  assert (got["pit_mean"][mask] == 0).all() and (got["variance_mean"] > 0).all()
  assert ((got["pit_mean"][~mask] > 0) & (got["pit_mean"][~mask] < 1)).all()
  # over the masked tail no observation arrives: the predictive variance does not shrink
  tail = got["variance_mean"][int(0.7 * T):]
  assert (np.diff(tail) > 0).all()


def test_host_summary_of_a_static_level_is_the_conjugate_update():
  """sigma_level = 0, no design: the filter is the normal-normal update, in closed form."""
  T, s0, so = 6, 2.0, 0.5
  y = np.array([1.0, 2.0, 0.5, np.nan, 1.5, 1.0])
  mask = np.isnan(y)
  draws = dict(observation_noise_scale=np.array([so]), level_scale=np.array([0.0]),
               slope_scale=np.zeros(1), seasonal_drift_scales=np.zeros((1, 0)), weights=np.zeros((1, 0)))
  spec = dict(init_level_loc=0.25, init_level_scale=s0, init_slope_scale=1.0, init_seasonal_scale=1.0)
  got = lib._prediction_summary_host(np.where(mask, 0.0, y), mask, None, np.zeros((0, T)), [], False,
                                     spec, draws, 1.0, 0.0, [0])
  m, v = 0.25, s0 * s0
  for t in range(T):
    np.testing.assert_allclose(got["forecast_mean"][t], m, rtol=1e-14)
    np.testing.assert_allclose(got["variance_mean"][t], v + so * so, rtol=1e-14)
    if not mask[t]:
      k = v / (v + so * so)
      m, v = m + k * (y[t] - m), v * (1 - k)


# ---- frames ------------------------------------------------------------------------------------

def _hand_summary():
  """Six model steps, four draws; forecast_sd = 2 everywhere."""
  return dict(forecast_mean=np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]),
              forecast_order=np.stack([np.arange(6.0) + r for r in range(4)]),     # ranks 0..3
              variance_mean=np.full(6, 4.0),
              pit_mean=np.array([0.5, 0.01, 0.3, 0.0, 0.99, 0.0]),
              loglik=np.array([-10.0, -12.0, -14.0, -16.0]))


def test_frames_schema_index_and_nan_placement():
  full = pd.RangeIndex(8)                       # two rows before the pre-period
  model = full[2:]
  observed = np.array([2.0, 1.0, 5.0, np.nan, 4.0, 9.0])     # step 3 missing, step 5 post-period
  conditioned = np.array([True, True, True, False, True, False])
  frame, quality = lib._prediction_frames(_hand_summary(), [0, 1, 2, 3], 0.5, observed, conditioned, 1,
                                          model, full)
  assert list(frame.columns) == list(lib.PREDICTION_COLUMNS) and frame.index.equals(full)
  assert frame.iloc[:2].isna().all().all()                   # rows the model never sees
  body = frame.iloc[2:]
  np.testing.assert_array_equal(body["forecast"], [1, 2, 3, 4, 5, 6])
  np.testing.assert_array_equal(body["forecast_sd"], np.full(6, 2.0))
  # alpha = 0.5 over 4 draws: the quartiles, numpy's linear interpolation at 0.75 and 2.25
  np.testing.assert_array_equal(body["forecast_lower"], np.arange(6.0) + 0.75)
  np.testing.assert_array_equal(body["forecast_upper"], np.arange(6.0) + 2.25)
  np.testing.assert_array_equal(body["error"], [1.0, -1.0, 2.0, np.nan, -1.0, np.nan])
  np.testing.assert_array_equal(body["standardized_error"], [0.5, -0.5, 1.0, np.nan, -0.5, np.nan])
  np.testing.assert_array_equal(body["pit"], [0.5, 0.01, 0.3, np.nan, 0.99, np.nan])
  # forecast, its band and its sd are there on every model step, also the missing and post-period ones
  assert not body[["forecast", "forecast_lower", "forecast_upper", "forecast_sd"]].isna().any().any()
  assert list(quality.index) == list(lib.FIT_QUALITY_ENTRIES)
  # a model that starts at the first row of the data keeps the index as it is
  same, _ = lib._prediction_frames(_hand_summary(), [0, 1, 2, 3], 0.5, observed, conditioned, 1, model, model)
  assert same.index.equals(model) and not same["forecast"].isna().any()


def test_fit_quality_by_hand():
  """State dimension 1: step 0 is not scored.  Scored steps 1, 2, 4 with errors -1, 2, -1."""
  observed = np.array([2.0, 1.0, 5.0, np.nan, 4.0, 9.0])
  conditioned = np.array([True, True, True, False, True, False])
  _, q = lib._prediction_frames(_hand_summary(), [0, 1, 2, 3], 0.5, observed, conditioned, 1,
                                pd.RangeIndex(6), pd.RangeIndex(6))
  assert q["n_scored"] == 3
  assert q["rmse"] == np.sqrt((1 + 4 + 1) / 3) and q["mae"] == 4 / 3
  # random walk: |1 - 2| at step 1, |5 - 1| at step 2; step 4 follows a missing value
  assert q["mase"] == (4 / 3) / 2.5
  # alpha = 0.5: pit within [0.25, 0.75] at step 2 only (0.01, 0.3, 0.99)
  assert q["coverage"] == 1 / 3
  assert q["loglik_mean"] == -13.0 and q["loglik_sd"] == np.std([-10, -12, -14, -16], ddof=1)
  # a wider state scores later steps only
  _, q3 = lib._prediction_frames(_hand_summary(), [0, 1, 2, 3], 0.5, observed, conditioned, 3,
                                 pd.RangeIndex(6), pd.RangeIndex(6))
  assert q3["n_scored"] == 1 and q3["mae"] == 1.0 and np.isnan(q3["mase"]) and q3["coverage"] == 0.0


# ---- the option ----------------------------------------------------------------------------------

def test_the_option_is_off_by_default_and_changes_no_other_default():
  assert ci.InferenceOptions().prediction_errors is False
  assert ci.InferenceOptions(prediction_errors=True).prediction_errors is True
  assert dataclasses.asdict(ci.InferenceOptions()) == dict(
      num_results=900, num_warmup_steps=100, num_chains=1, devices=None, sampler="gibbs",
      hmc_init="gibbs", hmc_prior="slab", summarize_on_device=True, kernel_flags=0, components=False)
  assert ci.InferenceOptions(prediction_errors=True) == ci.InferenceOptions()   # (not a field)
  one = lib.CausalImpactAnalysis(pd.DataFrame(), pd.DataFrame(), None)
  assert one.prediction_errors is None and one.fit_quality is None
  kept = dataclasses.replace(lib.CausalImpactAnalysis(1, 2, 3, None, None, None, "errors", "quality"),
                             posterior_samples=None)
  assert (kept.prediction_errors, kept.fit_quality) == ("errors", "quality")


def test_a_state_over_64_components_is_refused_before_any_fit(monkeypatch):
  def no_fit(*a, **k):
    raise AssertionError("the sampler was reached")
  monkeypatch.setattr(lib, "_run_sampler", no_fit)
  monkeypatch.setattr(batch, "_assemble", no_fit)
  monkeypatch.setattr(batch, "_fit_per_series", no_fit)
  T = 120
  rng = np.random.default_rng(0)
  df = pd.DataFrame({"y": rng.normal(size=T), "x": rng.normal(size=T)})
  wide = ci.ModelOptions(seasons=[ci.Seasons(40), ci.Seasons(26)])          # 1 + 39 + 25 = 65
  opts = ci.InferenceOptions(num_results=5, prediction_errors=True)
  with pytest.raises(ValueError, match="at most 64 components, this model has 65"):
    ci.fit_causalimpact(df, (0, 79), (80, 119), model_options=wide, inference_options=opts)
  with pytest.raises(ValueError, match="at most 64 components, this model has 65"):
    batch.fit_causalimpact_batch([df, df], (0, 79), (80, 119), model_options=wide, inference_options=opts)
  with pytest.raises(ValueError, match="at most 64 components, this model has 65"):
    batch.fit_causalimpact_panel([df, df], [((0, 79), (80, 119))] * 2, model_options=wide,
                                 inference_options=opts)
  assert lib.check_prediction_state(True, [ci.Seasons(40), ci.Seasons(24)]) == 64      # 2 + 39 + 23
  # ... and without the option nothing is checked: a wide state is fitted as before
  assert batch._state_dim(wide, ci.InferenceOptions()) == 0                   # pylint: disable=protected-access
  with pytest.raises(ValueError, match="this model has 65"):
    batch._state_dim(wide, opts)                                              # pylint: disable=protected-access
  with pytest.raises(AssertionError, match="the sampler was reached"):
    ci.fit_causalimpact(df, (0, 79), (80, 119), model_options=wide,
                        inference_options=ci.InferenceOptions(num_results=5))


def test_device_filter_takes_a_trend_with_at_most_one_block_of_2_to_7_seasons():
  assert lib.device_predictions_supported([]) and lib.device_predictions_supported([7])
  assert lib.device_predictions_supported([2])
  assert not lib.device_predictions_supported([8]) and not lib.device_predictions_supported([4, 3])


def test_batch_container_hands_out_frames_and_one_quality_row_per_series():
  """`CausalImpactBatchAnalysis` over a hand-made prediction summary: every series' frames are those
  of `_prediction_frames` on its rows, `fit_quality` has a row per series."""
  B, T, R = 2, 6, 4
  prep = dataclasses.make_dataclass("P", ["observed", "mask"])(
      observed=np.array([[2.0, 1.0, 5.0, np.nan, 4.0, 9.0], [0.0, 1.0, 2.0, 3.0, np.nan, 5.0]]),
      mask=np.array([[False, False, False, True, False, True], [False, False, False, False, True, True]]))
  one = _hand_summary()
  psum = {k: np.stack([v, v + 1.0]) for k, v in one.items()}
  res = batch.CausalImpactBatchAnalysis.__new__(batch.CausalImpactBatchAnalysis)
  res._prep, res._names, res.alpha, res._ranks = prep, ["a", "b"], 0.5, [0, 1, 2, 3]
  res._psum, res._state_dim, res._quality = psum, 1, None
  res._series_view = lambda b: (None, None, None, T)
  q = res.fit_quality
  assert list(q.index) == ["a", "b"] and list(q.columns) == list(lib.FIT_QUALITY_ENTRIES)
  for b in range(B):
    _, want = lib._prediction_frames({k: v[b] for k, v in psum.items()}, [0, 1, 2, 3], 0.5,
                                     prep.observed[b], ~prep.mask[b], 1, pd.RangeIndex(T), pd.RangeIndex(T))
    pd.testing.assert_series_equal(q.iloc[b], want, check_names=False)
  res._psum = None
  assert res.fit_quality is None
