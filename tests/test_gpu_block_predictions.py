"""ci_session_summarize_predictions_blocks and ci_session_summarize_placebo_blocks on the device -- the
prediction-error and placebo filters for any block list with a state of at most 64 components, a
group of lanes per filter (csrc/ci_predict_blocks.h) -- against their numpy twins
`_prediction_summary_host` / `_placebo_summary_host` on the draws fetched from the same session,
against the one-lane kernels where both take the model, bit for bit across launches, and through
`fit_causalimpact`, `fit_causalimpact_batch` and `fit_causalimpact_panel`.

2 chains x 12 kept draws give N = 24 pooled draws: no multiple of the 8, 4, 2 or 1 filters a
wavefront holds plus a remainder for every group size but 8 -- one case runs N = 70.  The steps
11, 12 and 40 are missing inside the pre-period and the post-period (from 0.7 T on) is masked.
Every comparison to a twin is at rtol 1e-8, atol 1e-8, the project's float64 contract."""
import functools

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _model
from causalimpact import _native
from causalimpact import _synthetic as syn
from causalimpact import causalimpact_lib as lib

import prior_cases

pytestmark = pytest.mark.gpu

SCALE, SHIFT = 3.7, -12.25
TOL = dict(rtol=1e-8, atol=1e-8)
RANKS = [0, 1, 11, 22, 23]
PRED = ("forecast_mean", "forecast_order", "variance_mean", "pit_mean", "loglik")
PLAC = ("predicted_mean", "spread_mean", "pit_mean")
PARAM_FIELDS = ["observation_noise_scale", "level_scale", "slope_scale", "seasonal_drift_scales", "weights"]

# name: (has_slope, seasons as (num_seasons, num_steps_per_season), T)
MODELS = {
    "4+3 slope d=7": (True, ((4, 1), (3, 1)), 90),
    "7+4+6 slope d=16": (True, ((7, 1), (4, 1), (6, 1)), 90),          # the last lane of a 16-group
    "7+4+6 d=15": (False, ((7, 1), (4, 1), (6, 1)), 90),
    "4x3+3 d=6": (False, ((4, 3), (3, 1)), 90),                        # the blocks change at different steps
    "12 d=12": (False, ((12, 1),), 90),
    "34 slope d=35": (True, ((34, 1),), 150),                          # the first step beyond a 32-group
    "63 slope d=64": (True, ((63, 1),), 150),                          # d = 64 exactly
}


def _state_dim(has_slope, seasons):
  return lib.prediction_state_dim(has_slope, [s[0] for s in seasons])


def _series(T, P, seed, has_slope, seasons, distinct=None):
  y, mask, X, _ = syn.standardize_for_sampler(*syn.make_raw_series(T, max(P - 1, 0), seed), int(0.7 * T))
  if seasons:
    y = y + 0.8 * np.sin(2 * np.pi * np.arange(T) / 7.0)
  mask = mask.copy()
  mask[[11, 12, 40]] = True
  spec = _model.series_params(np.where(mask, np.nan, y), mask, X, has_slope=has_slope,
                              num_seasonal_blocks=len(seasons))
  if distinct is not None:           # record number `distinct` of tests/prior_cases.py: no two fields agree
    spec = prior_cases.filter_record(spec, P, has_slope, distinct)
  return y, mask, X, spec


def _open(B, T, has_slope, seasons, only=None, S=12, distinct=False, P=3):
  """(session, inputs) of B series of T steps, or with `only` = b of that series alone at series_offset b."""
  series = [_series(T, P, 40 + 7 * b + P, has_slope, seasons, b if distinct else None) for b in range(B)]
  which = list(range(B)) if only is None else [only]
  num_seasons, sc = _model.expand_seasons(seasons, T)
  pb = _native.make_problem(T=T, P=P, has_slope=has_slope, num_warmup=10, num_results=S, num_chains=2,
                            num_series=len(which), seed=(5, 9), series_offset=which[0], num_seasons=num_seasons)
  y = np.stack([series[b][0] for b in which])
  mask = np.stack([series[b][1] for b in which])
  X = np.stack([series[b][2] for b in which])
  specs = [series[b][3] for b in which]
  sess = _native.Session(pb, y, mask, X, sc, _native.make_params(specs))
  inputs = dict(y=np.where(mask, 0, y).astype(np.float32), mask=mask, X=X.astype(np.float32), sc=sc,
                num_seasons=num_seasons, specs=specs, T=T)
  return sess, inputs


def _plan(B, T, has_slope, seasons):
  """origins [B, 3]: series 0 uses every slot, the others leave the last one unused; the first origin
  lies right behind the state dimension, the second on the missing step 40 or behind it."""
  d, pre = _state_dim(has_slope, seasons), int(0.7 * T)
  first = max(d + 2, 13)
  rows = [[first, max(first + 3, 40), pre - 7]] + [[first + b, pre - 9 - b, -1] for b in range(1, B)]
  return np.asarray(rows, np.int32)


@functools.lru_cache(maxsize=None)
def _run(name, B=2, only=None, S=12, distinct=False, scale=SCALE, shift=SHIFT):
  """One session of a model: the fetched parameter draws, the block-model summaries (predictions; the
  placebo for H = 1 and H = 5), the same with subsets of the outputs, and the inputs."""
  has_slope, seasons, T = MODELS[name]
  sess, inp = _open(B, T, has_slope, seasons, only, S, distinct)
  origins = _plan(B, T, has_slope, seasons)
  if only is not None:
    origins = origins[only:only + 1]
  ranks = RANKS if S == 12 else [0, 1, S, 2 * S - 2, 2 * S - 1]
  try:
    sess.run()
    draws = sess.fetch(PARAM_FIELDS)
    scale = np.asarray(scale, np.float64) if np.ndim(scale) else scale
    shift = np.asarray(shift, np.float64) if np.ndim(shift) else shift
    pred = sess.summarize_predictions_blocks(scale, shift, ranks)
    plac = {H: sess.summarize_placebo_blocks(scale, shift, origins, H) for H in (1, 5)}
    # subsets, in another order than the full call builds them
    some = dict(sess.summarize_predictions_blocks(scale, shift, ranks, want=["pit_mean"]))
    some.update(sess.summarize_predictions_blocks(scale, shift, ranks, want=["loglik", "variance_mean"]))
    some.update(sess.summarize_predictions_blocks(scale, shift, ranks, want=["forecast_order"]))
    some_plac = dict(sess.summarize_placebo_blocks(scale, shift, origins, 5, want=["pit_mean"]))
    some_plac.update(sess.summarize_placebo_blocks(scale, shift, origins, 5, want=["spread_mean", "predicted_mean"]))
    return dict(draws=draws, pred=pred, plac=plac, some=some, some_plac=some_plac, inp=inp, origins=origins,
                ranks=ranks, kernel=sess.kernel_name())
  finally:
    sess.close()


def _pooled(draws, b):
  return {k: v[b].reshape((v.shape[1] * v.shape[2],) + v.shape[3:]) for k, v in draws.items()}


def _twin(run, name, b, scale, shift):
  """(prediction summary, {H: placebo summary}) of series b in numpy from the session's own draws."""
  has_slope, _, _ = MODELS[name]
  inp = run["inp"]
  args = (inp["y"][b], inp["mask"][b], inp["X"][b], inp["sc"], inp["num_seasons"], has_slope, inp["specs"][b],
          _pooled(run["draws"], b))
  pred = lib._prediction_summary_host(*args, scale, shift, run["ranks"])          # pylint: disable=protected-access
  plac = {H: lib._placebo_summary_host(*args, scale, shift, run["origins"][b], H) for H in (1, 5)}   # pylint: disable=protected-access
  return pred, plac


def _check_against_twin(run, name, scales, shifts):
  for b in range(run["inp"]["y"].shape[0]):
    pred, plac = _twin(run, name, b, scales[b], shifts[b])
    assert all(np.isfinite(v).all() for v in pred.values()) and (pred["variance_mean"] > 0).all()
    worst = {k: float(np.abs(run["pred"][k][b] - pred[k]).max()) for k in PRED}
    worst.update({f"H{H}.{k}": float(np.abs(run["plac"][H][k][b] - plac[H][k]).max()) for H in (1, 5) for k in PLAC})
    print(f"{name} [{run['kernel']}] series {b}: largest deviation " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k in PRED:
      np.testing.assert_allclose(run["pred"][k][b], pred[k], err_msg=f"{name} series {b} {k}", **TOL)
    for H in (1, 5):
      for k in PLAC:
        np.testing.assert_allclose(run["plac"][H][k][b], plac[H][k], err_msg=f"{name} series {b} H={H} {k}", **TOL)
      unused = run["origins"][b] < 0
      assert all((run["plac"][H][k][b][unused] == 0.0).all() for k in PLAC)


# ---- 1. the numpy twins ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(MODELS))
def test_both_entries_equal_the_numpy_twins_on_the_fetched_draws(name):
  run = _run(name)
  _check_against_twin(run, name, [SCALE] * 2, [SHIFT] * 2)
  assert (run["pred"]["pit_mean"][:, [11, 12, 40]] == 0.0).all()            # masked: nothing to score


def test_seventy_draws_fill_wavefronts_with_a_remainder():
  """N = 70 over groups of 8 lanes: eight wavefronts of 8 filters and one of 6."""
  run = _run("4+3 slope d=7", S=35)
  assert run["pred"]["loglik"].shape == (2, 70)
  _check_against_twin(run, "4+3 slope d=7", [SCALE] * 2, [SHIFT] * 2)


# ---- 2. the one-lane kernels -----------------------------------------------------------------------

@pytest.mark.parametrize("has_slope,seasons", [(False, ()), (True, ()), (True, ((7, 1),)), (False, ((2, 1),))])
def test_models_both_families_take_agree_with_the_one_lane_kernels(has_slope, seasons):
  sess, _ = _open(2, 90, has_slope, seasons)
  origins = _plan(2, 90, has_slope, seasons)
  try:
    sess.run()
    old = dict(pred=sess.summarize_predictions(SCALE, SHIFT, RANKS))
    new = dict(pred=sess.summarize_predictions_blocks(SCALE, SHIFT, RANKS))
    for H in (1, 5):
      old[H] = sess.summarize_placebo(SCALE, SHIFT, origins, H)
      new[H] = sess.summarize_placebo_blocks(SCALE, SHIFT, origins, H)
  finally:
    sess.close()
  gap, equal = 0.0, True
  for part in old:
    for k, want in old[part].items():
      got = new[part][k]
      gap = max(gap, float((np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max()))
      equal = equal and np.array_equal(got, want)
  print(f"slope={has_slope} seasons={seasons}: largest relative gap to the one-lane kernels {gap:.3e}, "
        f"bit-identical: {equal}")
  for part in old:
    for k, want in old[part].items():
      np.testing.assert_allclose(new[part][k], want, err_msg=f"{part} {k}", **TOL)


# ---- 3. bit for bit --------------------------------------------------------------------------------

def test_a_batch_and_its_series_one_by_one_agree_bit_for_bit():
  name = "7+4+6 slope d=16"
  whole = _run(name, B=3)
  for b in range(3):
    one = _run(name, B=3, only=b)
    for k in PRED:
      np.testing.assert_array_equal(one["pred"][k][0], whole["pred"][k][b], err_msg=f"series {b} {k}")
    for H in (1, 5):
      for k in PLAC:
        np.testing.assert_array_equal(one["plac"][H][k][0], whole["plac"][H][k][b], err_msg=f"series {b} H={H} {k}")


@pytest.mark.parametrize("name", ["7+4+6 slope d=16", "34 slope d=35"])
def test_any_subset_of_the_outputs_equals_the_full_call_bit_for_bit(name):
  run = _run(name)
  for k, v in run["some"].items():
    np.testing.assert_array_equal(v, run["pred"][k], err_msg=k)
  assert set(run["some"]) == {"pit_mean", "loglik", "variance_mean", "forecast_order"}
  for k in PLAC:
    np.testing.assert_array_equal(run["some_plac"][k], run["plac"][5][k], err_msg=k)


@pytest.mark.parametrize("name", ["4x3+3 d=6", "7+4+6 slope d=16", "63 slope d=64"])
def test_horizon_one_is_the_one_step_forecast_bit_for_bit(name):
  """H = 1 at observed origins: predicted_mean and pit_mean are the predictions entry's forecast_mean
  and pit_mean there; at a missing origin (step 40, where an origin falls on it) the window counts nothing."""
  run = _run(name)
  for b in range(2):
    org = run["origins"][b]
    seen = [i for i, o in enumerate(org) if o >= 0 and not run["inp"]["mask"][b, o]]
    assert len(seen) >= 2
    np.testing.assert_array_equal(run["plac"][1]["predicted_mean"][b, seen], run["pred"]["forecast_mean"][b, org[seen]])
    np.testing.assert_array_equal(run["plac"][1]["pit_mean"][b, seen], run["pred"]["pit_mean"][b, org[seen]])
    for i, o in enumerate(org):
      if o >= 0 and run["inp"]["mask"][b, o]:
        assert run["plac"][1]["predicted_mean"][b, i] == 0.0 and run["plac"][1]["pit_mean"][b, i] == 0.0


# ---- 4. every series' own prior record -----------------------------------------------------------------

def test_every_series_filters_from_its_own_distinct_prior_record():
  """Three series fitted with three records in which init_level_loc and the three init_*_scale differ
  from each other and between the series (tests/prior_cases.py), each with its own scale and shift."""
  name, scale, shift = "7+4+6 slope d=16", (3.7, 0.5, 2.0), (-12.25, 4.0, 0.0)
  run = _run(name, B=3, distinct=True, scale=scale, shift=shift)
  _check_against_twin(run, name, scale, shift)
  # the early steps feel the initial state: another series' record is far off there
  other, _ = _twin(dict(run, inp=dict(run["inp"], specs=run["inp"]["specs"][1:] + run["inp"]["specs"][:1])),
                   name, 0, scale[0], shift[0])
  assert np.abs(other["variance_mean"][:20] - run["pred"]["variance_mean"][0, :20]).max() > 1e-3


# ---- 5. errors before any device work ----------------------------------------------------------------

def test_errors_are_reported_before_any_device_work():
  L = _native.load()
  sess, _ = _open(2, 90, True, ((4, 1), (3, 1)))
  one, out = np.ones(2), np.zeros((2, 2))
  good = np.array([[13, 19], [13, -1]], np.int32)
  hz = np.array([5, 5], np.int32)
  rk = np.array([0, 1], np.int32)
  ptr = lambda a: None if a is None else a.ctypes.data

  def raw_placebo(scale, origins, horizon, O=2):
    rc = L.ci_session_summarize_placebo_blocks(sess._h, ptr(scale), one.ctypes.data, O, ptr(origins), ptr(horizon),  # pylint: disable=protected-access
                                               out.ctypes.data, None, None)
    return rc, L.ci_last_error().decode()

  def raw_predictions(scale, shift, ranks):
    rc = L.ci_session_summarize_predictions_blocks(sess._h, ptr(scale), ptr(shift), 2, ptr(ranks),  # pylint: disable=protected-access
                                                   None, None, None, None, None)
    return rc, L.ci_last_error().decode()

  try:
    with pytest.raises(_native.NativeError, match="ci_session_summarize_predictions_blocks needs a finished ci_session_run"):
      sess.summarize_predictions_blocks(1.0, 0.0, [0])
    with pytest.raises(_native.NativeError, match="ci_session_summarize_placebo_blocks needs a finished ci_session_run"):
      sess.summarize_placebo_blocks(1.0, 0.0, good, 5)
    sess.run()
    for args in ((None, one, rk), (one, None, rk), (one, one, None)):
      rc, msg = raw_predictions(*args)
      assert rc != 0 and "NULL argument" in msg
    for args in ((None, good, hz), (one, None, hz), (one, good, None)):
      rc, msg = raw_placebo(*args)
      assert rc != 0 and "NULL argument" in msg
    with pytest.raises(_native.NativeError):                     # (ranks beyond the 24 draws)
      sess.summarize_predictions_blocks(1.0, 0.0, [24])
    for O in (0, 91):
      rc, msg = raw_placebo(one, good, hz, O)
      assert rc != 0 and f"max_origins must be in [1, 90], got {O}" in msg
    with pytest.raises(_native.NativeError, match=r"horizon\[1\] must be at least 1, got 0"):
      sess.summarize_placebo_blocks(1.0, 0.0, good, [5, 0])
    for bad in ([[3, 3], [3, -1]], [[9, 3], [3, -1]], [[3, 9], [-1, 3]]):
      with pytest.raises(_native.NativeError, match="strictly ascending with the unused slots"):
        sess.summarize_placebo_blocks(1.0, 0.0, bad, 5)
    with pytest.raises(_native.NativeError, match="must be a step or -1"):
      sess.summarize_placebo_blocks(1.0, 0.0, [[3, 9], [-2, -1]], 5)
    with pytest.raises(_native.NativeError, match=r"origins\[0, 1\] = 86 with horizon 5 reaches beyond the series' 90 steps"):
      sess.summarize_placebo_blocks(1.0, 0.0, [[3, 86], [3, -1]], 5)
    with pytest.raises(ValueError, match="unknown placebo outputs"):
      sess.summarize_placebo_blocks(1.0, 0.0, good, 5, want=["pit"])
    with pytest.raises(ValueError, match="unknown prediction outputs"):
      sess.summarize_predictions_blocks(1.0, 0.0, [0], want=["pit"])
    got = sess.summarize_placebo_blocks(1.0, 0.0, [[13, 85], [13, -1]], 5)     # 85 + 5 = 90: the last admissible
    assert got["predicted_mean"].shape == (2, 2) and got["predicted_mean"][1, 1] == 0.0
  finally:
    sess.close()
  big, _ = _open(1, 150, True, ((64, 1),))                         # d = 65
  try:
    for call in (lambda: big.summarize_predictions_blocks(1.0, 0.0, [0]),
                 lambda: big.summarize_placebo_blocks(1.0, 0.0, [70], 5)):
      with pytest.raises(_native.NativeError, match=r"ci_session_summarize_p\w+_blocks takes a state of at most 64 "
                                                    r"components, this session has 65 with the blocks \(64\)"):
        call()
  finally:
    big.close()
  pb = _native.make_problem(T=90, P=3, has_slope=0, num_warmup=3, num_results=12, num_chains=2, num_series=2, seed=(5, 9))
  series = [_series(T, 3, 61 + T, False, ()) for T in (90, 70)]
  pad = lambda a, fill: np.concatenate([a, np.full((90 - a.shape[0],) + a.shape[1:], fill, a.dtype)])
  rag = _native.Session.ragged(pb, [90, 70], np.stack([pad(s[0], np.nan) for s in series]),
                               np.stack([pad(s[1], True) for s in series]), np.stack([pad(s[2], 7.5) for s in series]),
                               _native.make_params([s[3] for s in series]))
  try:
    rag.run()
    with pytest.raises(_native.NativeError, match="ci_session_summarize_predictions_blocks takes no ragged session"):
      rag.summarize_predictions_blocks(1.0, 0.0, [0])
    with pytest.raises(_native.NativeError, match="ci_session_summarize_placebo_blocks takes no ragged session"):
      rag.summarize_placebo_blocks(1.0, 0.0, [[13], [13]], 5)
    assert rag.summarize_predictions(1.0, 0.0, [0])["loglik"].shape == (2, 24)     # (theirs is the other entry)
  finally:
    rag.close()


# ---- 6. package level ----------------------------------------------------------------------------------

ALPHA, SEED = 0.1, 11
OPTS = dict(num_chains=2, num_results=12, num_warmup_steps=10)
PLACEBO = ci.Placebo(max_origins=5)
WIDE = [ci.Seasons(7), ci.Seasons(4), ci.Seasons(6)]
TWO = [ci.Seasons(4), ci.Seasons(3)]


def _frames(lengths):
  idx = pd.date_range("2022-03-01", periods=max(lengths), freq="D")
  frames = []
  for b, Tb in enumerate(lengths):
    y, X = syn.make_raw_series(max(lengths), 2, 70 + b, effect=4.0 + b)
    frame = pd.DataFrame(np.column_stack([y, X]), index=idx, columns=["y", "x0", "x1"]).iloc[:Tb].copy()
    frame.iloc[9 + b, 0] = np.nan                       # a missing value inside the pre-period
    frames.append(frame)
  return frames


def _periods(frame, b):
  last_pre = (7 * len(frame)) // 10 + b
  return ((frame.index[1 + b], frame.index[last_pre]), (frame.index[last_pre + 2], frame.index[len(frame) - 1 - b]))


def _fit(frame, periods, seasons, on=True):
  return ci.fit_causalimpact(
      frame, *periods, alpha=ALPHA, seed=SEED, placebo=PLACEBO if on else None,
      model_options=ci.ModelOptions(seasons=seasons, local_linear_trend=True),
      inference_options=ci.InferenceOptions(prediction_errors=on, **OPTS))


def _assert_frames(got, want, exact, what):
  for attr in ("prediction_errors", "placebo"):
    g, w = getattr(got, attr), getattr(want, attr)
    num = [c for c in g.columns if pd.api.types.is_float_dtype(g[c])]
    assert len(g) >= 3 and list(g.columns) == list(w.columns) and g.index.equals(w.index)
    if exact:
      pd.testing.assert_frame_equal(g, w, check_exact=True)
    else:
      print(what, attr, "largest deviation per column:", (g[num] - w[num]).abs().max().to_dict())
      np.testing.assert_allclose(g[num].to_numpy(np.float64), w[num].to_numpy(np.float64), err_msg=f"{what} {attr}", **TOL)
  for attr in ("fit_quality", "placebo_quality"):
    g, w = getattr(got, attr), getattr(want, attr)
    if exact:
      pd.testing.assert_series_equal(g, w, check_exact=True, check_names=False)
    else:
      np.testing.assert_allclose(g.to_numpy(np.float64), w.to_numpy(np.float64), err_msg=f"{what} {attr}", **TOL)


def test_single_fit_takes_the_device_route_equals_the_host_summaries_and_disturbs_nothing(monkeypatch):
  frame = _frames([100])[0]
  periods = _periods(frame, 0)
  calls = []
  for entry in ("summarize_predictions_blocks", "summarize_placebo_blocks"):
    inner = getattr(_native.Session, entry)
    monkeypatch.setattr(_native.Session, entry,
                        lambda self, *a, _inner=inner, _entry=entry, **k: (calls.append(_entry), _inner(self, *a, **k))[1])
  one = _fit(frame, periods, WIDE)
  assert calls == ["summarize_predictions_blocks", "summarize_placebo_blocks"]
  off = _fit(frame, periods, WIDE, on=False)
  assert calls == ["summarize_predictions_blocks", "summarize_placebo_blocks"]         # off: no new kernel runs
  assert off.prediction_errors is None and off.placebo is None
  pd.testing.assert_frame_equal(one.series, off.series, check_exact=True)
  pd.testing.assert_frame_equal(one.summary, off.summary, check_exact=True)
  for k in ("observation_noise_scale", "level_scale", "weights"):
    np.testing.assert_array_equal(np.asarray(getattr(one.posterior_samples, k)), np.asarray(getattr(off.posterior_samples, k)))
  # the same fit with the block-model route switched off: numpy on the draws of the very same session
  monkeypatch.setattr(lib, "device_block_predictions_supported", lambda *a: False)
  host = _fit(frame, periods, WIDE)
  assert len(calls) == 2
  pd.testing.assert_frame_equal(one.series, host.series, check_exact=True)
  _assert_frames(one, host, False, "single fit 7+4+6")
  assert (one.placebo["predicted_sd"] > 0).all() and one.fit_quality["n_scored"] > 30


def test_batch_frames_equal_the_single_fits_bit_for_bit():
  frames = _frames([100, 100, 100])
  periods = _periods(frames[0], 0)
  got = ci.fit_causalimpact_batch(
      frames, *periods, alpha=ALPHA, seed=SEED, shared_streams=True, placebo=PLACEBO,
      model_options=ci.ModelOptions(seasons=WIDE, local_linear_trend=True),
      inference_options=ci.InferenceOptions(prediction_errors=True, **OPTS))
  assert type(got) is ci.CausalImpactBatchAnalysis             # (the one-launch route)
  for b in range(3):
    _assert_frames(got[b], _fit(frames[b], periods, WIDE), True, f"batch series {b}")


def test_a_panel_with_two_lengths_agrees_with_the_single_fits():
  lengths = (100, 90, 100)
  frames = _frames(lengths)
  got = ci.fit_causalimpact_panel(
      frames, [_periods(f, b) for b, f in enumerate(frames)], alpha=ALPHA, seed=SEED, shared_streams=True,
      placebo=PLACEBO, model_options=ci.ModelOptions(seasons=TWO, local_linear_trend=True),
      inference_options=ci.InferenceOptions(prediction_errors=True, **OPTS))
  for b in range(3):
    _assert_frames(got[b], _fit(frames[b], _periods(frames[b], b), TWO), False, f"panel series {b}")
