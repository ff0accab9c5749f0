"""The block-model filters (ci_session_summarize_predictions_blocks, ci_session_summarize_placebo_blocks)
without a device: which models they take, which entry the summaries routine picks, what the header
declares, and that the numpy twin the device tests compare against is well-conditioned on the
shapes they use."""
import os
import re

import numpy as np
import pytest

from causalimpact import _model
from causalimpact import _native
from causalimpact import _synthetic as syn
from causalimpact import causalimpact_lib as lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "causalimpact_amd.h")


@pytest.mark.parametrize("has_slope,num_seasons,want", [
    (False, [], True), (True, [], True), (True, [7], True), (True, [4, 3], True), (False, [7, 4, 6], True),
    (True, [63], True),                     # d = 64 exactly
    (True, [64], False),                    # d = 65
    (False, [40, 30], False),               # d = 69
    (True, [40, 30], False),
])
def test_the_predicate_takes_every_block_list_up_to_64_state_components(has_slope, num_seasons, want):
  assert lib.device_block_predictions_supported(has_slope, num_seasons) is want
  d = lib.prediction_state_dim(has_slope, num_seasons)
  assert want == (d <= lib.PREDICTION_MAX_STATE == 64)


def test_the_one_lane_predicate_is_what_it_was():
  for ns, want in (([], True), ([2], True), ([7], True), ([8], False), ([4, 3], False), ([12], False)):
    assert lib.device_predictions_supported(ns) is want


class _Stub:
  """A session that records which entries the summaries routine calls."""
  summaries = ("effect", "components", "predictions", "windows", "placebo", "paths")

  def __init__(self, B, T, blocks_entries=True):
    self.B, self.T, self.calls = B, T, []
    if blocks_entries:
      self.summarize_predictions_blocks = lambda *a, **k: self._pred("summarize_predictions_blocks")
      self.summarize_placebo_blocks = lambda sc, sh, org, hz, **k: self._plac("summarize_placebo_blocks", org)

  def summarize(self, *a, **k):
    self.calls.append("summarize")
    return dict(value_order=np.zeros((self.B, 1, self.T)))

  def _pred(self, name):
    self.calls.append(name)
    return dict(loglik=np.zeros((self.B, 4)))

  def _plac(self, name, origins):
    self.calls.append(name)
    return {k: np.zeros(np.shape(origins)) for k in _native.PLACEBO_OUTPUTS}

  def summarize_predictions(self, *a, **k):
    return self._pred("summarize_predictions")

  def summarize_placebo(self, sc, sh, org, hz, **k):
    return self._plac("summarize_placebo", org)

  def fetch(self, names):
    self.calls.append("fetch")
    raise _Fetched()


class _Fetched(Exception):
  pass


def _request_and_inputs(num_seasons, has_slope, T=40):
  y, mask = np.zeros(T), np.zeros(T, bool)
  sc = np.zeros((len(num_seasons), T), np.uint8)
  one = lib.SeriesInputs(y, mask, None, sc, list(num_seasons), has_slope, {})
  request = lib.SummaryRequest(
      scale=np.ones(1), shift=np.zeros(1), observed=np.zeros((1, T)), flags=np.zeros(T, np.uint8), ranks=[0],
      predictions=lib.Affine(np.ones(1), np.zeros(1)),
      placebo=lib.PlaceboPart(np.ones(1), np.zeros(1), np.array([[20, 25, -1]], np.int32), np.array([5])))
  return request, [one]


@pytest.mark.parametrize("num_seasons,has_slope,want", [
    ([7], True, ["summarize_predictions", "summarize_placebo"]),
    ([], False, ["summarize_predictions", "summarize_placebo"]),
    ([4, 3], True, ["summarize_predictions_blocks", "summarize_placebo_blocks"]),
    ([12], False, ["summarize_predictions_blocks", "summarize_placebo_blocks"]),
    ([63], True, ["summarize_predictions_blocks", "summarize_placebo_blocks"]),
])
def test_the_summaries_routine_picks_the_entry_by_the_model(num_seasons, has_slope, want):
  request, inputs = _request_and_inputs(num_seasons, has_slope)
  sess = _Stub(1, 40)
  record = lib.take_summaries(sess, request, inputs)
  assert sess.calls == ["summarize"] + want
  assert record.predictions is not None and record.placebo["predicted_mean"].shape == (1, 3)


@pytest.mark.parametrize("num_seasons,has_slope,blocks_entries", [([64], True, True), ([4, 3], True, False)])
def test_models_beyond_64_and_sessions_without_the_entries_stay_in_numpy(num_seasons, has_slope, blocks_entries):
  request, inputs = _request_and_inputs(num_seasons, has_slope)
  sess = _Stub(1, 40, blocks_entries)
  with pytest.raises(_Fetched):                   # (the numpy route begins by fetching the parameter draws)
    lib.take_summaries(sess, request, inputs)
  assert sess.calls == ["summarize", "fetch"]


def test_the_header_declares_both_entries_and_the_binding_lists_them():
  text = open(HEADER).read()
  for name in ("ci_session_summarize_predictions_blocks", "ci_session_summarize_placebo_blocks"):
    assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert name in _native.exported_symbols()
  assert callable(_native.Session.summarize_predictions_blocks)
  assert callable(_native.Session.summarize_placebo_blocks)


@pytest.mark.parametrize("has_slope,seasons,T", [
    (True, ((4, 1), (3, 1)), 90), (True, ((7, 1), (4, 1), (6, 1)), 90), (False, ((4, 3), (3, 1)), 90),
    (False, ((12, 1),), 90), (True, ((34, 1),), 150), (True, ((63, 1),), 150)])
def test_the_numpy_twin_is_finite_and_well_conditioned_on_the_shapes_of_the_device_tests(has_slope, seasons, T):
  """What tests/test_gpu_block_predictions.py compares the device against, on draws of the size a short
  fit gives: every one-step variance F stays positive (F >= sigma_obs^2 > 0) and everything is finite."""
  y, mask, X, _ = syn.standardize_for_sampler(*syn.make_raw_series(T, 2, 3), int(0.7 * T))
  mask = mask.copy()
  mask[[11, 12, 40]] = True
  num_seasons, sc = _model.expand_seasons(seasons, T)
  spec = _model.series_params(np.where(mask, np.nan, y), mask, X, has_slope=has_slope,
                              num_seasonal_blocks=len(seasons))
  rng = np.random.default_rng(1)
  N, sd = 6, spec["outcome_sd"]
  draws = dict(observation_noise_scale=sd * rng.uniform(0.3, 0.9, N), level_scale=sd * rng.uniform(0.005, 0.05, N),
               slope_scale=sd * rng.uniform(0.001, 0.01, N),
               seasonal_drift_scales=sd * rng.uniform(0.005, 0.03, (N, len(seasons))),
               weights=rng.normal(0, 0.3, (N, X.shape[1])))
  got = lib._prediction_summary_host(np.where(mask, 0, y), mask, X, sc, num_seasons, has_slope, spec, draws,  # pylint: disable=protected-access
                                     3.7, -12.25, [0, 3, 5])
  assert all(np.isfinite(v).all() for v in got.values())
  floor = np.mean((draws["observation_noise_scale"] * 3.7) ** 2)
  assert (got["variance_mean"] >= floor * (1 - 1e-9)).all()
  d = lib.prediction_state_dim(has_slope, num_seasons)
  plac = lib._placebo_summary_host(np.where(mask, 0, y), mask, X, sc, num_seasons, has_slope, spec, draws,  # pylint: disable=protected-access
                                   3.7, -12.25, [d + 2, int(0.7 * T) - 6, -1], 5, per_draw=True)
  assert all(np.isfinite(v).all() for v in plac.values()) and (plac["V"][:2] > 0).all()
