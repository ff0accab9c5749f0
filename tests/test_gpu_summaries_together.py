"""Every device summary of a fit asked for at once against each asked for alone, bit for bit.

`causalimpact_lib.take_summaries` calls the session's summaries in one order for every caller --
`summarize`, `summarize_components`, `summarize_predictions`, `summarize_windows`,
`summarize_placebo` -- which is sound only if no entry leaves anything behind for the next: every one
uploads its own scale, shift, ranks and observations, and the shared scratch carries nothing from one
call to the next.  So a fit with components, prediction errors, effect windows and placebo forecasts
together must return, frame for frame, what the fits with one of them return.

72 steps (54 before the treatment, 18 from it on), 2 covariates, 2 chains of 40 draws after 20
warm-up iterations: the placebo defaults give horizon 18 and 19 origins.  Models: a trend; a trend
with seven seasons (the device filter); a trend with two seasonal blocks (the numpy filter inside the
launch, one fetch of the parameter draws for prediction errors and placebo forecasts)."""
import functools

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _synthetic as syn
from causalimpact import batch

pytestmark = pytest.mark.gpu

ALPHA, SEED = 0.1, 23
T, N_PRE = 72, 54
OPTS = dict(num_chains=2, num_results=40, num_warmup_steps=20)
MODELS = {"trend": (), "weekly": (ci.Seasons(num_seasons=7),),
          "two_blocks": (ci.Seasons(num_seasons=7), ci.Seasons(num_seasons=4, num_steps_per_season=2))}
FEATURES = ("components", "prediction_errors", "effect_windows", "placebo")
PANEL_LENGTHS = (72, 60, 72)
# what each feature adds to a single fit's result
FRAMES = dict(components=("components", "coefficients"), prediction_errors=("prediction_errors", "fit_quality"),
              effect_windows=("window_summary",), placebo=("placebo", "placebo_quality"))
# ... and the tables over all series it adds to a batch's or panel's
TABLES = dict(components=(), prediction_errors=("fit_quality",), effect_windows=("window_summary",),
              placebo=("placebo_quality",))


def frames(lengths=(T, T, T)):
  idx = pd.date_range("2023-05-01", periods=max(lengths), freq="D")
  out = []
  for b, Tb in enumerate(lengths):
    y, X = syn.make_raw_series(max(lengths), 2, 310 + b, effect=3.0 + b)
    y = y + 1.5 * np.sin(2 * np.pi * np.arange(max(lengths)) / 7.0)
    frame = pd.DataFrame(np.column_stack([y, X]), index=idx, columns=["y", "x0", "x1"]).iloc[:Tb].copy()
    frame.iloc[11 + b, 0] = np.nan                      # a missing value inside the pre-period
    out.append(frame)
  return out


def periods(frame, b=0):
  """Three quarters of the rows before the treatment; series 2 of the panel with a row before its
  pre-period, a gap before the post-period and a tail behind it."""
  n_pre = (3 * len(frame)) // 4
  if b == 2:
    return (frame.index[1], frame.index[n_pre - 3]), (frame.index[n_pre], frame.index[len(frame) - 2])
  return (frame.index[0], frame.index[n_pre - 1]), (frame.index[n_pre], frame.index[len(frame) - 1])


def fit(route, model, features, series=0):
  """The fit of `route` -- "single" (series `series` of the batch), "batch", "panel" or "hmc_batch" --
  with the features of `features` on and the others off."""
  hmc = route == "hmc_batch"
  options = ci.InferenceOptions(components="components" in features,
                                prediction_errors="prediction_errors" in features,
                                sampler="hmc" if hmc else "gibbs", **OPTS)
  common = dict(alpha=ALPHA, seed=SEED, model_options=ci.ModelOptions(seasons=list(MODELS[model])),
                inference_options=options, placebo=True if "placebo" in features else None)
  windows = "effect_windows" in features
  if route == "panel":
    data = frames(PANEL_LENGTHS)
    return ci.fit_causalimpact_panel(data, [periods(f, b) for b, f in enumerate(data)], shared_streams=True,
                                     effect_windows={"first": (0, 6), "rest": (7, 13)} if windows else None,
                                     **common)
  data = frames()
  idx = data[0].index
  labels = {"first": (idx[N_PRE], idx[N_PRE + 8]), "rest": (idx[N_PRE + 9], idx[T - 1])} if windows else None
  if route == "single":
    return ci.fit_causalimpact(data[series], *periods(data[series]), effect_windows=labels, **common)
  return ci.fit_causalimpact_batch(data, *periods(data[0]), shared_streams=not hmc, effect_windows=labels,
                                   **common)


def features_of(route):
  """The features a route takes together.  An HMC batch asked for components leaves the one-launch
  path (it keeps no latent draws): there the other three."""
  return tuple(f for f in FEATURES if not (route == "hmc_batch" and f == "components"))


def result_frames(result, features):
  """{name: frame} of everything `features` put into `result`, and `series` / `summary`."""
  names = ("series", "summary") + tuple(n for f in features for n in FRAMES[f])
  if isinstance(result, ci.CausalImpactAnalysis):
    return {n: getattr(result, n) for n in names}
  out = {f"{b}/{n}": getattr(result[b], n) for b in range(len(result)) for n in names}
  out["summary"] = result.summary
  out.update({f"all/{n}": getattr(result, n) for f in features for n in TABLES[f]})
  return out


def assert_equal_bit_for_bit(got, want, what):
  assert (got is None) == (want is None), what
  if isinstance(want, pd.DataFrame):
    pd.testing.assert_frame_equal(got, want, check_exact=True, obj=what)
  elif want is not None:
    pd.testing.assert_series_equal(got, want, check_exact=True, obj=what)


@functools.lru_cache(maxsize=None)
def _single_together(model, series):
  return fit("single", model, FEATURES, series)


@pytest.mark.parametrize("route,model", [(r, m) for r in ("single", "batch", "panel") for m in MODELS]
                         + [("hmc_batch", "trend")])
def test_all_summaries_together_equal_each_one_alone(route, model):
  wanted = features_of(route)
  together = _single_together(model, 0) if route == "single" else fit(route, model, wanted)
  if route != "single":
    kind = ci.CausalImpactPanelAnalysis if route == "panel" else ci.CausalImpactBatchAnalysis
    assert type(together) is kind                              # (one launch, not series by series)
  all_frames = result_frames(together, wanted)
  assert not any(v is None for v in all_frames.values())
  first = together if route == "single" else together[0]
  if "placebo" in wanted and route != "panel":                 # (the shapes of the docstring)
    assert len(first.placebo) == 19 and first.placebo_quality["horizon"] == 18
  for feature in wanted:
    alone = fit(route, model, (feature,))
    for name, frame in result_frames(alone, (feature,)).items():
      assert_equal_bit_for_bit(all_frames[name], frame, f"{route}/{model}: {name} together vs {feature} alone")
    # ... and nothing but its own frames
    one = alone if route == "single" else alone[0]
    for f in wanted:
      if f != feature:
        assert all(getattr(one, n) is None for n in FRAMES[f])


@pytest.mark.parametrize("model", list(MODELS))
def test_batch_series_together_equal_their_single_fits(model):
  """shared_streams=True: series b of the batch is `fit_causalimpact` on it alone, with everything on
  in both.  Bit for bit the frames the one-feature tests pin so for a batch (prediction errors and
  coefficients are taken with every series' own scaler statistics); the placebo table to their 1e-8.
  `summary` and `window_summary` are put on the data scale with the batch's vectorised mean and sd,
  which may differ from the single fit's in the last bit: values of O(100) then move by O(1e-14), and
  the effects are differences of such values -- 1e-10 leaves four digits of room."""
  got = fit("batch", model, FEATURES)
  for b in range(len(got)):
    one = _single_together(model, b)
    for name in ("coefficients", "prediction_errors", "fit_quality"):
      assert_equal_bit_for_bit(getattr(got[b], name), getattr(one, name), f"{model}: series {b} {name}")
    for name in ("summary", "window_summary"):
      mine, want = getattr(got[b], name), getattr(one, name)
      assert mine.index.equals(want.index) and list(mine.columns) == list(want.columns)
      np.testing.assert_allclose(mine.to_numpy(np.float64), want.to_numpy(np.float64), rtol=1e-10, atol=1e-10,
                                 err_msg=f"{model}: series {b} {name}")
    numeric = [c for c in one.placebo.columns if c not in ("horizon_end", "significant")]
    assert got[b].placebo.index.equals(one.placebo.index)
    np.testing.assert_allclose(got[b].placebo[numeric].to_numpy(np.float64),
                               one.placebo[numeric].to_numpy(np.float64), rtol=1e-8, atol=1e-8)
    assert list(got[b].placebo["significant"]) == list(one.placebo["significant"])
    assert type(got) is batch.CausalImpactBatchAnalysis
