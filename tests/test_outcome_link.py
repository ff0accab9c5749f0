"""`outcome_link` without a GPU: the host definition of the link, every refusal before the native
library is touched, the model's copy of the frame, and the host summariser on synthetic log-scale
draws against a brute-force transcription in numpy (a stand-in for the sampler hands the draws to
the very code `summarize_on_device=False` runs)."""
import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _native
from causalimpact import batch
from causalimpact import causalimpact_lib as lib
from causalimpact import data as cid

# Quantiles commute with exp, numpy's linear interpolation between two order statistics does not: with
# (N - 1) * ALPHA / 2 = 2 and (N - 1) * (1 - ALPHA / 2) = 38 whole numbers both band edges ARE order
# statistics, and the data-scale bands equal the link of the log-scale bands to round-off.
ALPHA = 0.1
N, T_ALL = 41, 60


def test_link_values_host():
  z = np.array([-745.2, -3.5, -1e-20, 0.0, 1e-20, 0.25, 4.0, 709.0, 710.0])
  assert (_native.LINK_IDENTITY, _native.LINK_LOG, _native.LINK_LOG1P) == (0, 1, 2)
  same = _native.link_values_host(z.astype(np.float32), _native.LINK_IDENTITY)
  assert same.dtype == np.float64
  np.testing.assert_array_equal(same, z.astype(np.float32).astype(np.float64))
  with np.errstate(over="ignore"):
    np.testing.assert_array_equal(_native.link_values_host(z, _native.LINK_LOG), np.exp(z))
    np.testing.assert_array_equal(_native.link_values_host(z, _native.LINK_LOG1P), np.expm1(z))
  assert np.isinf(_native.link_values_host(z, _native.LINK_LOG)[-1])       # no clamp
  assert _native.link_values_host(z, _native.LINK_LOG1P)[4] == 1e-20        # expm1, not exp - 1
  with pytest.raises(ValueError, match="unknown link 7"):
    _native.link_values_host(z, 7)


def _frame(seed=0, T=T_ALL):
  rng = np.random.default_rng(seed)
  x = rng.normal(size=T).cumsum() * 0.1 + 2.0
  y = np.exp(3.0 + 0.4 * x + 0.05 * rng.normal(size=T))
  y[45:] *= 1.3
  return pd.DataFrame({"y": y, "x0": x}, index=pd.date_range("2023-01-02", periods=T, freq="D"))


def _periods(frame):
  idx = frame.index
  return (idx[1], idx[41]), (idx[45], idx[57])


@pytest.fixture
def no_native(monkeypatch):
  """Any use of the native library is an error."""
  def refuse(*_, **__):
    raise AssertionError("the native library was touched")
  monkeypatch.setattr(_native, "load", refuse)


def test_refusals_come_before_the_native_library(no_native):      # pylint: disable=unused-argument,redefined-outer-name
  frame = _frame()
  pre, post = _periods(frame)
  idx = frame.index
  bad = frame.copy()
  bad.iloc[7, 0] = 0.0
  with pytest.raises(ValueError, match=r"outcome_link='log'.*'y' > 0.*2023-01-09.*holds 0\.0"):
    ci.fit_causalimpact(bad, pre, post, outcome_link="log")
  bad.iloc[7, 0] = -1.0
  with pytest.raises(ValueError, match=r"outcome_link='log1p'.*'y' > -1.*2023-01-09"):
    ci.fit_causalimpact(bad, pre, post, outcome_link="log1p")
  with pytest.raises(ValueError, match="`outcome_link` must be None, 'log' or 'log1p', got 'sqrt'"):
    ci.fit_causalimpact(frame, pre, post, outcome_link="sqrt")
  with pytest.raises(ValueError, match="`placebo=` is not available with `outcome_link`"):
    ci.fit_causalimpact(frame, pre, post, outcome_link="log", placebo=True)
  # batches and panels name the series too
  frames = [_frame(0), bad, _frame(2)]
  with pytest.raises(ValueError, match=r"outcome_link='log1p'.*2023-01-09.*of series 'b'.*holds -1\.0"):
    ci.fit_causalimpact_batch(frames, pre, post, names=["a", "b", "c"], outcome_link="log1p")
  bad.iloc[7, 0] = -2.5
  with pytest.raises(ValueError, match=r"outcome_link='log'.*2023-01-09.*of series 'b'.*holds -2\.5"):
    ci.fit_causalimpact_batch(np.stack([f.to_numpy() for f in frames]), pre, post, index=idx,
                              names=["a", "b", "c"], outcome_link="log")
  with pytest.raises(ValueError, match=r"outcome_link='log'.*2023-01-09.*of series 'b'"):
    ci.fit_causalimpact_panel(frames, [(pre, post)] * 3, names=["a", "b", "c"], outcome_link="log")
  for fit, args in ((ci.fit_causalimpact_batch, (pre, post)), (ci.fit_causalimpact_panel, ([(pre, post)] * 3,))):
    with pytest.raises(ValueError, match="must be None, 'log' or 'log1p'"):
      fit([_frame(b) for b in range(3)], *args, outcome_link="exp")
    with pytest.raises(ValueError, match="`placebo=` is not available with `outcome_link`"):
      fit([_frame(b) for b in range(3)], *args, outcome_link="log", placebo=True)


def test_the_models_copy_transforms_the_outcome_column_alone():
  frame = _frame()
  pre, post = _periods(frame)
  frame.iloc[9, 0] = np.nan           # a missing value stays missing
  frame.iloc[0, 0] = -3.0             # before the pre-period: the model never reads it
  frame.iloc[50, 0] = 0.0             # a campaign may drive sales to 0
  before = frame.copy()
  got = lib.link_outcome(frame, pre, post, None, _native.LINK_LOG)
  pd.testing.assert_frame_equal(frame, before, check_exact=True)            # (the input is not written to)
  np.testing.assert_array_equal(got["x0"].to_numpy(), frame["x0"].to_numpy())
  want = np.log(frame["y"].to_numpy()[1:50])
  np.testing.assert_array_equal(got["y"].to_numpy()[1:50], want)
  assert np.isnan(got["y"].iloc[[0, 9, 50]]).all() and not np.isnan(got["y"].iloc[51:]).any()
  one = lib.link_outcome(frame, pre, post, "y", _native.LINK_LOG1P)
  np.testing.assert_array_equal(one["y"].to_numpy()[1:9], np.log1p(frame["y"].to_numpy()[1:9]))
  assert one["y"].iloc[50] == 0.0 and np.isnan(one["y"].iloc[0])            # log1p(0) = 0 is in the domain


def _fake_sampler(draws):
  """Stands in for `_run_sampler`: predictive draws [N, T] on the model's scale, nothing on a device."""
  def run(**kw):
    n, T = draws.shape
    assert kw["request"].on_device is False
    samples = dict(observation_noise_scale=np.ones(n), level_scale=np.ones(n), slope_scale=np.zeros(n),
                   weights=np.zeros((n, 2)), level=np.zeros((n, T)), slope=None,
                   seasonal_drift_scales=np.zeros((n, 0)), seasonal_levels=np.zeros((n, T, 0)))
    return samples, draws.mean(axis=0), draws, lib.SummaryRecord()
  return run


def _fit(monkeypatch, frame, draws, **kw):
  monkeypatch.setattr(lib, "_run_sampler", _fake_sampler(draws))
  pre, post = _periods(frame)
  return ci.fit_causalimpact(frame, pre, post, alpha=ALPHA,
                             inference_options=ci.InferenceOptions(summarize_on_device=False), **kw)


@pytest.mark.parametrize("link", ["log", "log1p"])
def test_host_summary_of_log_scale_draws_against_brute_force(monkeypatch, no_native, link):   # pylint: disable=unused-argument,redefined-outer-name
  frame = _frame()
  frame.iloc[50, 0] = 0.0                                   # accepted: the model never reads the post-period
  frame.iloc[48, 0] = np.nan
  fwd, inv = (np.log, np.exp) if link == "log" else (np.log1p, np.expm1)
  T = T_ALL - 1                                             # the model's steps: row 0 lies before the pre-period
  draws = np.random.default_rng(5).normal(size=(N, T)) * 0.6 + 0.3
  windows = {"first": (frame.index[45], frame.index[49])}
  got = _fit(monkeypatch, frame, draws, outcome_link=link, effect_windows=windows)
  y = frame["y"].to_numpy()
  # `observed` is the input column, bit for bit, the zero included
  np.testing.assert_array_equal(got.series["observed"].to_numpy(), y)
  assert got.series["observed"].iloc[50] == 0.0
  # brute force: z on the transformed data scale with the scaler of the pre-period's log y, then the link
  logged = fwd(y[1:42])
  mu, sd = np.nanmean(logged), np.nanstd(logged, ddof=1)
  z = draws * sd + mu
  v = inv(z)
  series = got.series.iloc[1:]
  np.testing.assert_allclose(series["posterior_mean"].to_numpy(), v.mean(axis=0), rtol=1e-12)
  jensen = inv(z.mean(axis=0))
  assert (series["posterior_mean"].to_numpy() > jensen).all()
  for name, q in (("posterior_lower", ALPHA / 2), ("posterior_upper", 1 - ALPHA / 2)):
    np.testing.assert_allclose(series[name].to_numpy(), inv(np.quantile(z, q, axis=0)), rtol=1e-12)
  post = np.arange(45, 58) - 1                              # the model steps of the post-period
  obs = y[45:58]
  totals = v[:, post].sum(axis=1)
  summary = got.summary
  np.testing.assert_allclose(summary.loc["cumulative", "predicted"], v.mean(axis=0)[post].sum(), rtol=1e-12)
  np.testing.assert_allclose(summary.loc["cumulative", ["predicted_lower", "predicted_upper"]].to_numpy(float),
                             np.quantile(totals, [ALPHA / 2, 1 - ALPHA / 2]), rtol=1e-12)
  np.testing.assert_allclose(summary.loc["cumulative", "actual"], np.nansum(obs), rtol=1e-15)
  effect = np.nansum(obs[None, :] - v[:, post], axis=1)     # (the step without an observation is skipped)
  np.testing.assert_allclose(summary.loc["cumulative", ["abs_effect_lower", "abs_effect_upper"]].to_numpy(float),
                             np.quantile(effect, [ALPHA / 2, 1 - ALPHA / 2]), rtol=1e-12)
  rel = np.nansum(obs) / totals - 1.0
  np.testing.assert_allclose(summary.loc["cumulative", "rel_effect"], rel.mean(), rtol=1e-12)
  np.testing.assert_allclose(summary.loc["cumulative", ["rel_effect_lower", "rel_effect_upper"]].to_numpy(float),
                             np.quantile(rel, [ALPHA / 2, 1 - ALPHA / 2]), rtol=1e-12)
  pool = np.append(totals, np.nansum(obs))
  p = min((np.nansum(obs) <= pool).mean(), (np.nansum(obs) >= pool).mean())
  assert summary.loc["cumulative", "p_value"] == p
  # a window: every draw's total over its own steps
  first = v[:, 44:49].sum(axis=1)
  np.testing.assert_allclose(
      got.window_summary.loc[("first", "cumulative"), ["predicted_lower", "predicted_upper"]].to_numpy(float),
      np.quantile(first, [ALPHA / 2, 1 - ALPHA / 2]), rtol=1e-12)


def test_without_a_link_the_host_path_returns_todays_frames(monkeypatch, no_native):   # pylint: disable=unused-argument,redefined-outer-name
  frame = _frame()
  pre, post = _periods(frame)
  draws = np.random.default_rng(6).normal(size=(N, T_ALL - 1))
  windows = {"first": (frame.index[45], frame.index[49])}
  got = _fit(monkeypatch, frame, draws, effect_windows=windows)
  same = _fit(monkeypatch, frame, draws, effect_windows=windows, outcome_link=None)
  ci_data = cid.CausalImpactData(frame, pre, post)
  resolved = lib.resolve_windows(windows, ci_data.data.index, lib.posterior_processing.model_index(ci_data),
                                 ci_data.post_period)
  series, summary, window_summary = lib._compute_impact(      # pylint: disable=protected-access
      draws.mean(axis=0), draws, ci_data, ALPHA, windows=resolved)
  for one in (got, same):
    pd.testing.assert_frame_equal(one.series, series, check_exact=True)
    pd.testing.assert_frame_equal(one.summary, summary, check_exact=True)
    pd.testing.assert_frame_equal(one.window_summary, window_summary, check_exact=True)


def test_an_hmc_batch_with_a_link_takes_the_per_series_route():
  kw = dict(float64=False, standardize_data=True, num_seasonal_blocks=0, T=100, P=2, hmc_init="gibbs")
  assert batch.hmc_batch_route(**kw) == "one_launch"
  assert batch.hmc_batch_route(**kw, outcome_link=False) == "one_launch"
  assert batch.hmc_batch_route(**kw, outcome_link=True) == "per_series"


def test_the_request_and_the_prepared_batch_carry_the_link():
  assert lib.SummaryRequest(1.0, 0.0, np.zeros(3), np.zeros(3, np.uint8), [0]).link == 0
  assert [f.name for f in lib.dataclasses.fields(lib.SummaryRequest)][-1] == "link"
  frames = [_frame(b) for b in range(3)]
  pre, post = _periods(frames[0])
  raw = np.stack([f.to_numpy() for f in frames])
  logged = raw.copy()
  logged[:, :, 0] = np.log(raw[:, :, 0])
  index = frames[0].index
  model = batch.prepare_batch(logged, index, pre, post)
  prep = batch._under_link(model, batch.prepare_batch(raw, index, pre, post), _native.LINK_LOG)   # pylint: disable=protected-access
  assert prep.link == _native.LINK_LOG and prep.model is model and model.link == 0
  np.testing.assert_array_equal(prep.values, raw)                           # what the frames read
  np.testing.assert_array_equal(prep.observed[:, :prep.num_pre], raw[:, prep.model_rows[:prep.num_pre], 0])
  np.testing.assert_array_equal(prep.y, model.y)                            # what the sampler reads
  np.testing.assert_array_equal(prep.outcome_sd, model.outcome_sd)
