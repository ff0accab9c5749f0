"""Prediction errors and placebo forecasts of the fits whose draws lie on the host -- a float64 fit, an
HMC fit, a fit over two device shares, a seasonal HMC batch fitted series by series, the one-launch
HMC batch with aggregates -- filtered on the device through a session made from the draws
(`causalimpact_lib.open_draws_session`).

For every route: the frames equal those of the same call with `summarize_on_device=False` (the numpy
twins) at rtol 1e-8, atol 1e-8 with identical NaN placement; `posterior_samples`, `series` and
`summary` equal, bit for bit, those of the call without the options; and the calls succeed with the
five host filters replaced by functions that raise.  70 steps, 2 chains x 40 draws."""
import dataclasses

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _synthetic as syn
from causalimpact import causalimpact_lib as lib

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-8, atol=1e-8)
ALPHA, SEED = 0.1, (0, 11)
OPTS = dict(num_chains=2, num_results=40, num_warmup_steps=30)
HOST_FILTERS = ("_host_prediction_summaries", "_host_placebo_summaries", "_host_placebo_simulations",
                "_placebo_entry_host", "_placebo_entry_simulated_host")
CHECKS = ("prediction_errors", "fit_quality", "placebo", "placebo_quality")
AGGREGATES = {"all": "all", "weighted": {0: 0.5, 2: 2.0}}


def _frames(positive=False):
  idx = pd.date_range("2022-03-01", periods=70, freq="D")
  frames = []
  for b in range(3):
    y, X = syn.make_raw_series(70, 2, 70 + b, effect=4.0 + b)
    if positive:                      # (for the log link: outcomes around 20 that move multiplicatively)
      y = np.exp(3.0 + 0.25 * (y - y.mean()) / y.std())
    frame = pd.DataFrame(np.column_stack([y, X]), index=idx, columns=["y", "x0", "x1"])
    frame.iloc[9 + b, 0] = np.nan     # a missing value inside the pre-period
    frames.append(frame)
  return frames


def _periods(frame):
  return (frame.index[1], frame.index[42]), (frame.index[44], frame.index[69])


def _no_host_filters(monkeypatch):
  def refuse(*args, **kw):
    raise AssertionError("a numpy filter was reached on a route that filters on the device")
  for name in HOST_FILTERS:
    monkeypatch.setattr(lib, name, refuse)


def _assert_agree(got, want, what):
  """A frame or series of the device route against the numpy route: the same labels, NaNs in the same
  places, numbers within the tolerance, everything else equal."""
  if want is None:
    assert got is None, what
    return
  got, want = pd.DataFrame(got), pd.DataFrame(want)
  assert list(got.columns) == list(want.columns) and got.index.equals(want.index), what
  for col in want.columns:
    a, b = got[col], want[col]
    if pd.api.types.is_float_dtype(b):
      np.testing.assert_array_equal(np.isnan(a.to_numpy()), np.isnan(b.to_numpy()), err_msg=f"{what} {col}: NaN placement")
      np.testing.assert_allclose(a.to_numpy(), b.to_numpy(), err_msg=f"{what} {col}", **TOL)
    else:
      assert list(a) == list(b), f"{what} {col}"


def _assert_same_fit(got, plain, what):
  pd.testing.assert_frame_equal(got.series, plain.series, check_exact=True)
  pd.testing.assert_frame_equal(got.summary, plain.summary, check_exact=True)
  if plain.posterior_samples is None:       # (a batch keeps no latent draws)
    assert got.posterior_samples is None, what
    return
  for f in (f.name for f in dataclasses.fields(plain.posterior_samples)):
    a, b = getattr(got.posterior_samples, f), getattr(plain.posterior_samples, f)
    assert (a is None and b is None) or np.array_equal(np.asarray(a), np.asarray(b)), f"{what}: {f}"


SINGLE = {
    "float64": dict(data_options=ci.DataOptions(dtype=np.float64)),
    "hmc": dict(sampler="hmc"),
    "two device shares": dict(devices=[0, 0]),
    "float64, blocks": dict(data_options=ci.DataOptions(dtype=np.float64),
                            model_options=ci.ModelOptions(seasons=[ci.Seasons(4), ci.Seasons(3)])),
}


@pytest.mark.parametrize("route", list(SINGLE))
def test_single_fits_filter_on_the_device(route, monkeypatch):
  frame = _frames()[0]
  periods = _periods(frame)
  extra = dict(SINGLE[route])
  outer = {k: extra.pop(k) for k in ("data_options", "model_options") if k in extra}

  def fit(on_device=True, **kw):
    options = ci.InferenceOptions(summarize_on_device=on_device, prediction_errors=bool(kw), **OPTS, **extra)
    return ci.fit_causalimpact(frame, *periods, alpha=ALPHA, seed=SEED, inference_options=options, **outer, **kw)

  calls = dict(analytic=dict(placebo=True), simulated=dict(placebo=ci.Placebo(simulate=True)))
  host = {k: fit(False, **kw) for k, kw in calls.items()}
  _no_host_filters(monkeypatch)
  plain = fit()
  for k, kw in calls.items():
    got = fit(**kw)
    for check in CHECKS:
      assert getattr(got, check) is not None, (route, k, check)
      _assert_agree(getattr(got, check), getattr(host[k], check), f"{route}, {k}: {check}")
    assert len(got.placebo) >= 2 and got.prediction_errors["pit"].notna().sum() > 30
    _assert_same_fit(got, plain, f"{route}, {k}")


BATCH = {
    # fitted series by series: every fit hands its pooled terms to the batch's sink
    "seasonal hmc, series by series": dict(
        options=dict(sampler="hmc"), model_options=ci.ModelOptions(seasons=[ci.Seasons(7)]),
        calls=dict(analytic=dict(placebo=True), pooled=dict(placebo=ci.Placebo(max_origins=6, simulate=True, pool=True)))),
    # one launch of B x chains HMC chains: one draws session over the launch's series
    "hmc batch, one launch": dict(
        options=dict(sampler="hmc"), positive=True, outcome_link="log",
        calls=dict(pooled=dict(placebo=ci.Placebo(max_origins=6, simulate=True, pool=True)))),
    "hmc batch, one launch, analytic": dict(options=dict(sampler="hmc"), calls=dict(analytic=dict(placebo=True))),
}


@pytest.mark.parametrize("route", list(BATCH))
def test_batches_filter_on_the_device(route, monkeypatch):
  case = BATCH[route]
  frames = _frames(case.get("positive", False))
  periods = _periods(frames[0])
  outer = {k: case[k] for k in ("model_options", "outcome_link") if k in case}

  def fit(on_device=True, **kw):
    options = ci.InferenceOptions(summarize_on_device=on_device, prediction_errors=bool(kw), **OPTS, **case["options"])
    return ci.fit_causalimpact_batch(frames, *periods, alpha=ALPHA, seed=SEED, inference_options=options,
                                     aggregates=AGGREGATES, **outer, **kw)

  host = {k: fit(False, **kw) for k, kw in case["calls"].items()}
  _no_host_filters(monkeypatch)
  plain = fit()
  for k, kw in case["calls"].items():
    got = fit(**kw)
    for b in range(3):
      for check in CHECKS:
        assert getattr(got[b], check) is not None, (route, k, b, check)
        _assert_agree(getattr(got[b], check), getattr(host[k][b], check), f"{route}, {k}, series {b}: {check}")
      _assert_same_fit(got[b], plain[b], f"{route}, {k}, series {b}")
    for check in ("fit_quality", "placebo_quality", "aggregate_placebo_quality"):
      _assert_agree(getattr(got, check), getattr(host[k], check), f"{route}, {k}: {check}")
    pd.testing.assert_frame_equal(got.summary, plain.summary, check_exact=True)
    for name in AGGREGATES:
      one, twin = got.aggregates[name], host[k].aggregates[name]
      assert one.placebo is not None and len(one.placebo) >= 2, (route, k, name)
      _assert_agree(one.placebo, twin.placebo, f"{route}, {k}, aggregate {name}: placebo")
      _assert_agree(one.placebo_quality, twin.placebo_quality, f"{route}, {k}, aggregate {name}: placebo_quality")
      pd.testing.assert_frame_equal(one.series, plain.aggregates[name].series, check_exact=True)
      pd.testing.assert_frame_equal(one.summary, plain.aggregates[name].summary, check_exact=True)
