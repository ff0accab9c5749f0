"""Component summaries, host side (no GPU): the numpy definitions against a hand-computed example,
the schemas of the `components` / `coefficients` frames, the option's defaults and the argument
checks of `Session.summarize_components` that run before any native call."""
import dataclasses

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _native
from causalimpact import causalimpact_lib as lib

# three draws, two steps, two seasonal blocks, two design columns; every number is a small dyadic
# rational, so the expected values below are exact
LEVEL = np.array([[1, 2], [3, 4], [5, 6]], np.float32)
SEASONAL = np.stack([np.array([[1, -1], [0, 2], [2, 2]], np.float32),
                     np.array([[.5, 0], [.5, 1], [-1, 2]], np.float32)], axis=-1)      # [N, T, K]
WEIGHTS = np.array([[1, 0], [2, .5], [0, 0]], np.float32)                               # a zero weight
X = np.array([[1, 2], [3, 4]], np.float32)
SCALE, SHIFT = 2.0, 10.0


def _host():
  return lib._component_summary_host(LEVEL, SEASONAL, WEIGHTS, X, SCALE, SHIFT, [0, 1, 2])


def test_host_summary_matches_the_hand_computed_example():
  got = _host()
  # trend = level * 2 + 10 = [[12, 14], [16, 18], [20, 22]]
  np.testing.assert_array_equal(got["trend_mean"], [16, 18])
  np.testing.assert_array_equal(got["trend_order"], [[12, 14], [16, 18], [20, 22]])
  # block 0 * 2 = [[2, -2], [0, 4], [4, 4]]; block 1 * 2 = [[1, 0], [1, 2], [-2, 4]]
  np.testing.assert_array_equal(got["seasonal_mean"], [[2, 2], [0, 2]])
  np.testing.assert_array_equal(got["seasonal_order"],
                                [[[0, -2], [2, 4], [4, 4]], [[-2, 0], [1, 2], [1, 4]]])
  # X w: draw 0 [1, 3], draw 1 [2 + 1, 6 + 2], draw 2 [0, 0]; * 2 = [[2, 6], [6, 16], [0, 0]]
  np.testing.assert_allclose(got["regression_mean"], [8 / 3, 22 / 3], rtol=1e-15)
  np.testing.assert_array_equal(got["regression_order"], [[0, 0], [2, 6], [6, 16]])
  np.testing.assert_array_equal(got["inclusion_prob"], [2 / 3, 1 / 3])
  np.testing.assert_allclose(got["weight_mean"], [1, .5 / 3], rtol=1e-15)
  np.testing.assert_array_equal(got["weight_order"], [[0, 0], [1, 0], [2, .5]])


def test_host_summary_leaves_out_what_the_model_lacks():
  got = lib._component_summary_host(LEVEL, np.zeros((3, 2, 0), np.float32), None, None, SCALE, SHIFT,
                                    [0, 2])
  assert sorted(got) == ["trend_mean", "trend_order"]
  assert got["trend_order"].shape == (2, 2)


def test_frames_have_the_documented_schema_and_index():
  full = pd.date_range("2024-01-01", periods=3)          # one row before the pre-period
  model = full[1:]
  comp, coef = lib._component_frames(_host(), [0, 1, 2], 3, 0.5, model, full, ["x0", "intercept_"])
  assert list(comp.columns) == [
      "trend", "trend_lower", "trend_upper", "seasonal_0", "seasonal_0_lower", "seasonal_0_upper",
      "seasonal_1", "seasonal_1_lower", "seasonal_1_upper", "regression", "regression_lower",
      "regression_upper"]
  assert comp.index.equals(full)
  assert comp.iloc[0].isna().all()                       # the model never saw that row
  # alpha = 0.5 over three draws: the quantiles 0.25 / 0.75 lie half-way between neighbours
  np.testing.assert_array_equal(comp["trend"].to_numpy()[1:], [16, 18])
  np.testing.assert_array_equal(comp["trend_lower"].to_numpy()[1:], [14, 16])
  np.testing.assert_array_equal(comp["trend_upper"].to_numpy()[1:], [18, 20])
  np.testing.assert_array_equal(comp["seasonal_1_lower"].to_numpy()[1:], [-.5, 1])
  np.testing.assert_array_equal(comp["regression_upper"].to_numpy()[1:], [4, 11])
  assert list(coef.columns) == ["inclusion_probability", "mean", "lower", "upper"]
  assert list(coef.index) == ["x0", "intercept_"]
  np.testing.assert_array_equal(coef["inclusion_probability"], [2 / 3, 1 / 3])
  np.testing.assert_array_equal(coef["lower"], [.5, 0])
  np.testing.assert_array_equal(coef["upper"], [1.5, .25])
  # a model without covariates or seasons: trend columns only, no coefficients frame
  bare = lib._component_summary_host(LEVEL, np.zeros((3, 2, 0), np.float32), None, None, 1.0, 0.0,
                                     [0, 1, 2])
  comp, coef = lib._component_frames(bare, [0, 1, 2], 3, 0.5, model, model, None)
  assert list(comp.columns) == ["trend", "trend_lower", "trend_upper"] and coef is None
  assert comp.index.equals(model)


def test_the_option_is_off_by_default_and_changes_no_other_default():
  opts = dataclasses.asdict(ci.InferenceOptions())
  assert opts.pop("components") is False
  assert opts == dict(num_results=900, num_warmup_steps=100, num_chains=1, devices=None,
                      sampler="gibbs", hmc_init="gibbs", hmc_prior="slab", summarize_on_device=True,
                      kernel_flags=0)
  names = [f.name for f in dataclasses.fields(lib.CausalImpactAnalysis)]
  assert names == ["series", "summary", "posterior_samples", "diagnostics", "components",
                   "coefficients"]
  one = lib.CausalImpactAnalysis(pd.DataFrame(), pd.DataFrame(), None)
  assert one.components is None and one.coefficients is None


def _unbound_session(**kw):
  """A Session object without a native handle: the checks under test run before it is used."""
  base = dict(T=20, P=2, has_slope=0, num_warmup=1, num_results=5, num_chains=2, num_series=3)
  base.update(kw)
  s = _native.Session.__new__(_native.Session)
  s.pb, s._lib, s._h = _native.make_problem(**base), None, None
  return s


def test_summarize_components_checks_rank_count_and_shapes_before_any_native_call():
  s = _unbound_session()
  with pytest.raises(ValueError, match="1 to 8 order statistics, got 0"):
    s.summarize_components(1.0, 0.0, [])
  with pytest.raises(ValueError, match="1 to 8 order statistics, got 9"):
    s.summarize_components(1.0, 0.0, list(range(9)))
  with pytest.raises(ValueError, match="`scale` must be a scalar or have one entry per series"):
    s.summarize_components(np.ones(2), 0.0, [0])
  with pytest.raises(ValueError, match="`shift` must be a scalar or have one entry per series"):
    s.summarize_components(np.ones(3), np.zeros((3, 1)), [0])
  with pytest.raises(ValueError, match="unknown component outputs"):
    s.summarize_components(1.0, 0.0, [0], want=["trend_mean", "slope_mean"])
  assert _native.MAX_SUMMARY_RANKS == 8
  assert "ci_session_summarize_components" in _native.exported_symbols()
