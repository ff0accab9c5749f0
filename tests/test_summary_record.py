"""`causalimpact_lib.take_summaries` over a fake session, and the map from the caller's scale to the
sampler's internal units: no device, no library."""
import numpy as np
import pytest

from causalimpact import _model
from causalimpact import causalimpact_lib as lib

_T, _C, _S, _R, _P = 12, 2, 3, 2, 2      # steps, chains, draws per chain, order statistics, columns
_ALL = ("effect", "components", "predictions", "windows", "placebo")


@pytest.mark.parametrize("cond_mu,cond_s", [(0.0, 1.0), (100.0001, 3.7), (-2.5e4, 1e-3)])
def test_conditioning_map_is_the_float64_expression(cond_mu, cond_s):
  for scale, shift in [(1.0, 0.0), (3.25, -17.5), (1e-4, 100.0001), (np.float32(0.3), np.float32(1e6)),
                       (np.array([2.0, 0.1]), np.array([-1.0, 7e3]))]:
    got = lib._to_internal_units(scale, shift, cond_mu, cond_s)     # pylint: disable=protected-access
    scale64, shift64 = np.asarray(scale, np.float64), np.asarray(shift, np.float64)
    np.testing.assert_array_equal(np.asarray(got.scale, np.float64).view(np.uint64),
                                  np.asarray(scale64 * cond_s).view(np.uint64))
    np.testing.assert_array_equal(np.asarray(got.shift, np.float64).view(np.uint64),
                                  np.asarray(shift64 + cond_mu * scale64).view(np.uint64))


class _FakeSession:
  """Records the calls `take_summaries` makes; `summaries`: the kinds it claims to take."""

  def __init__(self, num_series, summaries=_ALL):
    self.n, self.summaries, self.calls = num_series, summaries, []

  def _log(self, name, scale, shift):
    self.calls.append((name, np.asarray(scale, np.float64).copy(), np.asarray(shift, np.float64).copy()))

  def summarize(self, scale, shift, observed, flags, ranks):
    self._log("summarize", scale, shift)
    lead = () if self.n == 1 else (self.n,)           # (`Session.summarize` drops the axis of one series)
    return dict(value_order=np.zeros(lead + (len(ranks), _T)), cum_order=np.zeros(lead + (len(ranks), _T)),
                per_draw=np.zeros(lead + (2, _C * _S)), per_draw_order=np.zeros(lead + (2, len(ranks))))

  def summarize_components(self, scale, shift, ranks):
    self._log("summarize_components", scale, shift)
    return dict(trend_mean=np.zeros((self.n, _T)), weight_order=np.zeros((self.n, len(ranks), _P)))

  def summarize_predictions(self, scale, shift, ranks):
    self._log("summarize_predictions", scale, shift)
    return dict(forecast_mean=np.zeros((self.n, _T)), loglik=np.zeros((self.n, _C * _S)))

  def summarize_windows(self, scale, shift, observed, first, count, ranks):
    self._log("summarize_windows", scale, shift)
    return dict(per_draw=np.zeros((self.n, len(first), 2, _C * _S)))

  def summarize_placebo(self, scale, shift, origins, horizon):
    self._log("summarize_placebo", scale, shift)
    return {k: np.ones(np.shape(origins)) for k in ("predicted_mean", "spread_mean", "pit_mean")}

  def fetch(self, want):
    self.calls.append(("fetch", tuple(want)))
    rng = np.random.default_rng(5)
    return dict(observation_noise_scale=0.5 + rng.random((self.n, _C, _S)),
                level_scale=0.1 + rng.random((self.n, _C, _S)), slope_scale=np.zeros((self.n, _C, _S)),
                seasonal_drift_scales=np.zeros((self.n, _C, _S, 0)), weights=rng.normal(size=(self.n, _C, _S, _P)))


def _inputs(num_series):
  rng = np.random.default_rng(3)
  out = []
  for _ in range(num_series):
    y, X = rng.normal(size=_T), rng.normal(size=(_T, _P))
    mask = np.arange(_T) >= 9
    mask[4] = True
    params = _model.series_params(np.where(mask, np.nan, y), mask, X)
    out.append(lib.SeriesInputs(y, mask, X, np.zeros((0, _T), np.uint8), (), False, params))
  return out


def _request(num_series, **parts):
  lead = () if num_series == 1 else (num_series,)
  return lib.SummaryRequest(scale=np.full(lead, 2.0), shift=np.full(lead, -3.0), observed=np.zeros(lead + (_T,)),
                            flags=np.zeros(_T, np.uint8), ranks=[0, _C * _S - 1], **parts)


_EVERYTHING = dict(components=True, predictions=lib.Affine(5.0, 7.0), windows=lib.Windows([9], [3]),
                   placebo=lib.PlaceboPart(11.0, 13.0, np.array([3, 5, -1]), 2))


def test_take_calls_the_five_summaries_in_one_order_with_the_mapped_scales():
  cond_mu, cond_s = 100.0001, 3.7
  request = lib._request_in_internal_units(_request(1, **_EVERYTHING), cond_mu, cond_s)   # pylint: disable=protected-access
  sess = _FakeSession(1)
  record = lib.take_summaries(sess, request, _inputs(1))
  assert [c[0] for c in sess.calls] == ["summarize", "summarize_components", "summarize_predictions",
                                        "summarize_windows", "summarize_placebo"]
  own = {"summarize": (2.0, -3.0), "summarize_components": (2.0, -3.0), "summarize_predictions": (5.0, 7.0),
         "summarize_windows": (2.0, -3.0), "summarize_placebo": (11.0, 13.0)}
  for name, scale, shift in sess.calls:
    want = own[name]
    assert np.all(scale == want[0] * cond_s) and np.all(shift == want[1] + cond_mu * want[0]), name
  assert all(arrays is not None for _, arrays in record.kinds())
  # the placebo summary of the device with `_placebo_seen`'s two rows, the unused slot included
  assert set(record.placebo) == set(lib.SUMMARY_KINDS["placebo"].whole)
  assert record.placebo["n_counted"].shape == (1, 3) and record.placebo["n_counted"][0, 2] == 0
  assert np.isnan(record.placebo["seen_sum"][0, 2])


def test_request_is_left_as_it_was():
  request = _request(2, **_EVERYTHING)
  before = {f: getattr(request, f) for f in ("scale", "shift", "ranks", "predictions", "windows", "placebo")}
  lib.take_summaries(_FakeSession(2), request, _inputs(2))
  assert all(getattr(request, f) is v for f, v in before.items())
  with pytest.raises(Exception):
    request.ranks = [1]                                       # (frozen)


@pytest.mark.parametrize("num_series", [1, 3])
def test_session_without_the_filter_entries_takes_the_host_route_on_one_fetch(num_series):
  sess = _FakeSession(num_series, summaries=("effect", "windows"))
  inputs = _inputs(num_series)
  request = _request(num_series, **_EVERYTHING)
  record = lib.take_summaries(sess, request, inputs)
  names = [c[0] for c in sess.calls]
  assert names == ["summarize", "fetch", "summarize_windows"]
  assert sess.calls[1][1] == lib._PARAMETER_DRAWS              # pylint: disable=protected-access
  assert record.components is None                            # (a kind this session lacks: the caller's business)
  draws = sess.fetch(lib._PARAMETER_DRAWS)                     # pylint: disable=protected-access
  for b, one in enumerate(inputs):
    pooled = {k: v[b].reshape((_C * _S,) + v.shape[3:]) for k, v in draws.items()}
    want = lib._prediction_summary_host(*one.filter_inputs(), pooled, 5.0, 7.0, request.ranks)   # pylint: disable=protected-access
    for k, v in want.items():
      np.testing.assert_array_equal(record.predictions[k][b], v)
    want = lib._placebo_summary_host(*one.filter_inputs(), pooled, 11.0, 13.0, [3, 5, -1], 2)    # pylint: disable=protected-access
    for k, v in want.items():
      np.testing.assert_array_equal(record.placebo[k][b], v)
    n_counted, seen_sum = lib._placebo_seen(one.outcome(), one.mask, [3, 5, -1], 2, 11.0, 13.0)   # pylint: disable=protected-access
    np.testing.assert_array_equal(record.placebo["n_counted"][b], n_counted)
    np.testing.assert_array_equal(record.placebo["seen_sum"][b], seen_sum)


def test_model_the_device_filter_does_not_take_goes_to_the_host_on_a_full_session():
  sess = _FakeSession(1)
  inputs = [lib.SeriesInputs(**{**vars(_inputs(1)[0]), "num_seasons": (7, 4),
                                "season_change": np.zeros((2, _T), np.uint8)})]
  inputs[0].params["init_seasonal_scale"] = 1.0
  rng = np.random.default_rng(9)
  fetch = sess.fetch
  sess.fetch = lambda want: dict(fetch(want), seasonal_drift_scales=0.1 + rng.random((1, _C, _S, 2)))
  record = lib.take_summaries(sess, _request(1, predictions=lib.Affine(1.0, 0.0),
                                             placebo=lib.PlaceboPart(1.0, 0.0, [3], 2)), inputs)
  assert [c[0] for c in sess.calls] == ["summarize", "fetch"]
  assert record.predictions["forecast_mean"].shape == (1, _T) and record.placebo["pit_mean"].shape == (1, 1)


def test_one_series_session_returns_the_effect_with_the_series_axis():
  record = lib.take_summaries(_FakeSession(1), _request(1))
  assert record.effect["value_order"].shape == (1, 2, _T) and record.effect["per_draw"].shape == (1, 2, _C * _S)
  assert [arrays is None for _, arrays in record.kinds()] == [False, True, True, True, True]
  several = lib.take_summaries(_FakeSession(3), _request(3))
  assert several.effect["value_order"].shape == (3, 2, _T)
  assert record.of_series(0).effect["value_order"].shape == (2, _T)
