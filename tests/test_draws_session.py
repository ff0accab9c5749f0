"""A session made from draws (ci_session_create_from_draws[_f64], `_native.DrawsSession`) without a
device: the symbols behind header, binding and library, every validation error of the create entry
(all raised before the first device call: this file runs where there is no GPU), the route the
package chooses for draws that lie on the host, and the power of the float64 test of
tests/test_gpu_draws_session.py on its own inputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from causalimpact import _native
from causalimpact import causalimpact_lib as lib

import draws_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ci_session_create_from_draws", "ci_session_create_from_draws_f64")


def test_header_binding_and_library_agree_on_the_new_symbols():
  text = open(os.path.join(ROOT, "include", "causalimpact_amd.h")).read()
  L = _native.load()
  for name, real in zip(NEW, ("float", "double")):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
    assert m, name
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const ci_problem* problem", f"const {real}* y", "const uint8_t* mask", f"const {real}* X",
                      "const uint8_t* season_change", "const ci_series_params* params",
                      f"const {real}* observation_noise_scale", f"const {real}* level_scale",
                      f"const {real}* slope_scale", f"const {real}* seasonal_drift_scales", f"const {real}* weights",
                      "ci_session** session"]
    assert name in _native.exported_symbols()
    assert len(getattr(L, name).argtypes) == len(params)
  assert issubclass(_native.DrawsSession, _native.Session)
  assert set(_native.DrawsSession.summaries) == {"predictions", "placebo"}
  for method in ("summarize_predictions", "summarize_placebo", "simulate_placebo", "pool_placebo",
                 "pool_simulated_placebo"):
    assert callable(getattr(_native.DrawsSession, method)) and callable(getattr(_native.DrawsSession, method + "_blocks"))


def _create(name, dtype, *, inp=None, draws=None, pb=None):
  inp = dc.inputs(name) if inp is None else inp
  draws = dc.synthetic_draws(name) if draws is None else draws
  return _native.DrawsSession(dc.problem(name) if pb is None else pb, inp["y"], inp["mask"], inp["X"], inp["sc"],
                              _native.make_params(inp["specs"]), draws, dtype=dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_validation_error_is_raised_without_a_device(dtype):
  name = "slope+7 d=8"
  inp, draws = dc.inputs(name), dc.synthetic_draws(name)
  # an unmasked outcome that is not finite (a masked one is never read)
  bad = dict(inp, y=inp["y"].copy())
  bad["y"][1, 11] = np.nan
  bad["y"][2, 5] = np.inf
  with pytest.raises(_native.NativeError, match=r"y\[2, 5\] is not finite but unmasked"):
    _create(name, dtype, inp=bad)
  # scale draws: negative, NaN, infinite -- the message names the array, the series and the pooled draw
  for field, at, value, where in (("observation_noise_scale", (1, 1, 3), -0.5, "series 1, draw 43"),
                                  ("level_scale", (0, 0, 7), np.nan, "series 0, draw 7"),
                                  ("slope_scale", (2, 1, 39), np.inf, "series 2, draw 79"),
                                  ("seasonal_drift_scales", (1, 0, 2, 0), -1e-9, "series 1, draw 2, block 0")):
    wrong = dict(draws, **{field: draws[field].copy()})
    wrong[field][at] = value
    with pytest.raises(_native.NativeError, match=f"{field} of {where} must be finite and not negative"):
      _create(name, dtype, draws=wrong)
  # the problem record
  pb = dc.problem(name)
  pb.abi_version += 1
  with pytest.raises(_native.NativeError, match="ABI mismatch"):
    _create(name, dtype, pb=pb)
  pb = dc.problem(name)
  pb.chain_offset = -1
  with pytest.raises(_native.NativeError, match="series_offset and chain_offset must be >= 0"):
    _create(name, dtype, pb=pb)
  # shapes, and a missing array the model reads: the binding's own errors
  with pytest.raises(ValueError, match=r"draws\['weights'\] must be \[3, 2, 40, 2\], got \[3, 2, 40, 3\]"):
    _create(name, dtype, draws=dict(draws, weights=np.zeros((dc.B, dc.C, dc.S, 3), np.float32)))
  with pytest.raises(ValueError, match="`draws` lacks 'slope_scale'"):
    _create(name, dtype, draws={k: v for k, v in draws.items() if k != "slope_scale"})
  with pytest.raises(ValueError, match="`dtype` must be float32 or float64"):
    _create(name, np.float16)


@pytest.mark.parametrize("entry,real", zip(NEW, (np.float32, np.float64)))
def test_null_pointers_are_refused_without_a_device(entry, real):
  name = "slope+7 d=8"
  inp, draws = dc.inputs(name), dc.synthetic_draws(name)
  fn = getattr(_native.load(), entry)
  pb = dc.problem(name)
  keep = [np.ascontiguousarray(inp["y"], real), np.ascontiguousarray(inp["mask"].astype(np.uint8)),
          np.ascontiguousarray(inp["X"], real), np.ascontiguousarray(inp["sc"], np.uint8)]
  keep += [np.ascontiguousarray(draws[k], real) for k in dc.DRAW_FIELDS]
  params = _native.make_params(inp["specs"])
  h = C.c_void_p()
  messages = {0: "NULL argument", 1: "NULL argument", 2: "X is NULL but P=2", 3: "season_change is NULL but num_blocks > 0",
              4: "NULL argument", 5: "NULL argument", 6: "slope_scale is NULL but has_slope is set",
              7: "seasonal_drift_scales is NULL but num_blocks > 0", 8: "weights is NULL but P=2"}
  for missing, message in messages.items():
    ptrs = [None if i == missing else a.ctypes.data for i, a in enumerate(keep)]
    assert fn(C.byref(pb), *ptrs[:4], params, *ptrs[4:], C.byref(h)) != 0
    assert message in _native.load().ci_last_error().decode(), (missing, _native.load().ci_last_error())
  ptrs = [a.ctypes.data for a in keep]
  assert fn(C.byref(pb), *ptrs[:4], None, *ptrs[4:], C.byref(h)) != 0
  assert fn(C.byref(pb), *ptrs[:4], params, *ptrs[4:], None) != 0
  assert fn(None, *ptrs[:4], params, *ptrs[4:], C.byref(h)) != 0
  assert "problem is NULL" in _native.load().ci_last_error().decode()
  assert not h.value


def test_the_route_of_draws_that_lie_on_the_host():
  route = lib.draws_filter_route
  assert route(False, ()) == "one_lane" and route(True, (7,)) == "one_lane" and route(False, (2,)) == "one_lane"
  assert route(False, (8,)) == "blocks" and route(False, (4, 3)) == "blocks" and route(True, (12,)) == "blocks"
  assert route(True, (63,)) == "blocks"                         # d = 64 exactly
  assert lib.prediction_state_dim(True, (63,)) == lib.PREDICTION_MAX_STATE == 64
  # beyond 64 components the numpy twins stay, and the options refuse the model before any fit
  assert route(True, (64,)) == "host" and route(False, (40, 27)) == "host"
  with pytest.raises(ValueError, match="takes a state of at most 64 components, this model has 65"):
    lib.check_prediction_state(True, [lib.Seasons(64)])
  # `InferenceOptions(summarize_on_device=False)`: numpy, whatever the model
  for model in ((False, ()), (True, (7,)), (False, (4, 3)), (True, (64,))):
    assert route(*model, on_device=False) == "host"
  assert lib.InferenceOptions().summarize_on_device is True


def test_a_session_with_the_entries_is_not_doubled():
  """`_draws_session_beside` opens nothing beside a session that has the filter entries itself (it
  came to the host route for its model or its library), nor with the option off."""
  class Sess:
    summaries = _native.Session.summaries
    pb = dc.problem("4+3 d=6")
  one = lib.SeriesInputs(np.zeros(9), np.zeros(9, bool), None, np.zeros((2, 9), np.uint8), (4, 3), False, {})
  assert lib._draws_session_beside(Sess(), [one], {}, True) == (None, False)            # pylint: disable=protected-access
  Sess.summaries = _native.BatchLogLikSession.summaries
  assert lib._draws_session_beside(Sess(), [one], {}, False) == (None, False)           # pylint: disable=protected-access


@pytest.mark.parametrize("name", list(dc.MODELS))
def test_the_float64_test_has_the_power_to_tell_float32_inputs(name):
  """On the inputs of the float64 test the twin on float64 inputs and the twin on the same inputs
  rounded to float32 differ by more than 100 x the tolerance, in the one-step forecasts and in the
  placebo's predicted sums: a float64 entry that rounded its inputs would fail that test."""
  inp, draws = dc.f64_case(name)
  for arrays in (inp["y"], inp["X"], *draws.values()):
    assert arrays.dtype == np.float64 and (not arrays.size or np.mean(arrays.astype(np.float32) == arrays) < 0.01)
  for b in range(dc.B):
    wide = dc.twin_predictions(inp, draws, b, dc.F64_SCALE, dc.F64_SHIFT)["forecast_mean"]
    narrow = dc.twin_predictions(inp, draws, b, dc.F64_SCALE, dc.F64_SHIFT, np.float32)["forecast_mean"]
    print(f"{name} series {b}: forecast_mean moves by {np.abs(wide - narrow).max():.2e} (values up to {np.abs(wide).max():.2f})")
    assert dc.beyond(narrow, wide)
    wide = dc.twin_placebo(inp, draws, b, dc.F64_SCALE, dc.F64_SHIFT)["predicted_mean"]
    narrow = dc.twin_placebo(inp, draws, b, dc.F64_SCALE, dc.F64_SHIFT, np.float32)["predicted_mean"]
    print(f"{name} series {b}: predicted_mean moves by {np.abs(wide - narrow).max():.2e} (values up to {np.abs(wide).max():.2f})")
    assert dc.beyond(narrow, wide)
