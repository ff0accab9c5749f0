"""ci_session_summarize_predictions on the device -- the one-step-ahead prediction errors of every
fit -- at session level against numpy written here, from the parameter draws fetched from the same
session, and at package level (`InferenceOptions(prediction_errors=True)`) against
`_prediction_summary_host` and across the routes.

T = 70 crosses one 64-step tile with a remainder; C = 2, S = 37 gives N = 74 draws: one full
wavefront of lanes and a remainder.  Every comparison is to rtol 1e-8, atol 1e-8, the project's
float64 contract (tests/test_gpu_float64.py); the order statistics are compared with a sort of the
reference (sorting does not enlarge a sup-norm error)."""
import dataclasses
import functools
import math

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _model
from causalimpact import _native
from causalimpact import _synthetic as syn
from causalimpact import causalimpact_lib as lib
from causalimpact import data as cid
from oracle import ci_oracle as orc

import prior_cases

pytestmark = pytest.mark.gpu

SCALE, SHIFT = 3.7, -12.25
RANKS = [1, 2, 36, 71, 72]          # the ranks of a 95 % band over 74 draws, and the median
TOL = dict(rtol=1e-8, atol=1e-8)
OUTPUTS = ("forecast_mean", "forecast_order", "variance_mean", "pit_mean", "loglik")
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def _series(T, P, seed, has_slope, seasons, distinct=None):
  """Sampler inputs of one series with P design columns (the intercept is the last one); the steps
  11, 12 and 40 are missing inside the pre-period."""
  y, mask, X, _ = syn.standardize_for_sampler(*syn.make_raw_series(T, max(P - 1, 0), seed), int(0.7 * T))
  if P == 1:
    X = np.ones((T, 1))
  if seasons:
    y = y + 0.8 * np.sin(2 * np.pi * np.arange(T) / 7.0)
  mask = mask.copy()
  mask[[11, 12, 40]] = True
  spec = _model.series_params(np.where(mask, np.nan, y), mask, X, has_slope=has_slope,
                              num_seasonal_blocks=len(seasons))
  if distinct is not None:           # record number `distinct` of tests/prior_cases.py: no two fields agree
    spec = prior_cases.filter_record(spec, P, has_slope, distinct)
  return y, mask, X, spec


def _pad(arrs, T, fill):
  out = np.full((len(arrs), T) + arrs[0].shape[1:], fill, arrs[0].dtype)
  for b, a in enumerate(arrs):
    out[b, :a.shape[0]] = a
  return out


def _open(lengths, P, has_slope, seasons, ragged=False, only=None, C_=2, S=37, seed=(5, 9), distinct=False):
  """(session, inputs): the batch of len(lengths) series, or with `only` = b the session of that
  series alone at series_offset b.  inputs: what the reference needs, as the session holds it."""
  K = len(seasons)
  series = [_series(T, P, 40 + 7 * b + P, has_slope, seasons, b if distinct else None)
            for b, T in enumerate(lengths)]
  T = max(lengths)
  if ragged and K:
    T = (T + 3) & ~3
  which = list(range(len(lengths))) if only is None else [only]
  pb = _native.make_problem(T=T, P=P, has_slope=has_slope, num_warmup=3, num_results=S, num_chains=C_,
                            num_series=len(which), seed=seed, series_offset=which[0],
                            num_seasons=_model.expand_seasons(seasons, 1)[0])
  y = _pad([series[b][0] for b in which], T, np.nan)
  mask = _pad([series[b][1] for b in which], T, True)
  X = None if P == 0 else _pad([series[b][2] for b in which], T, 7.5)   # (padding rows are never read)
  specs = [series[b][3] for b in which]
  sc = _model.expand_seasons(seasons, T)[1]
  if ragged:
    sess = _native.Session.ragged(pb, [lengths[b] for b in which], y, mask, X,
                                  _native.make_params(specs), season_change=sc if K else None)
  else:
    sess = _native.Session(pb, y, mask, X, sc, _native.make_params(specs))
  inputs = dict(y=np.where(mask, 0, y).astype(np.float32), mask=mask, sc=sc, specs=specs, T=T,
                X=None if X is None else X.astype(np.float32), lengths=[lengths[b] for b in which])
  return sess, inputs


def _reference(inp, draws, b, has_slope, seasons, scale, shift):
  """The definitions of include/causalimpact_amd.h in numpy for series b over its own steps, all N
  draws at once with dense d x d matrices: forecast, variance, pit [N, T_b] and loglik [N]."""
  Tb, spec = inp["lengths"][b], inp["specs"][b]
  pool = lambda a: a[b].reshape((a.shape[1] * a.shape[2],) + a.shape[3:]).astype(np.float64)
  s_obs, s_level = pool(draws["observation_noise_scale"]), pool(draws["level_scale"])
  s_slope, w = pool(draws["slope_scale"]), pool(draws["weights"])
  N, hs = s_obs.shape[0], int(has_slope)
  ns = seasons[0][0] if seasons else 0
  n1, o = max(ns - 1, 0), 1 + hs
  d = o + n1
  reg = np.zeros((N, Tb))
  for j in range(w.shape[1]):
    reg += inp["X"][b, :Tb, j].astype(np.float64)[None, :] * w[:, j, None]
  Z = np.zeros(d)
  Z[0] = 1.0
  Tm, Tseason = np.eye(d), np.eye(d)
  if hs:
    Tm[0, 1] = 1.0
  a, Pm = np.zeros((N, d)), np.zeros((N, d, d))
  a[:, 0] = spec["init_level_loc"]
  Pm[:, 0, 0] = spec["init_level_scale"] ** 2
  if hs:
    Pm[:, 1, 1] = spec["init_slope_scale"] ** 2
  if ns:
    Z[o] = 1.0
    Pm[:, o:, o:] = spec["init_seasonal_scale"] ** 2 * (np.eye(n1) - 1.0 / ns)
    Tseason[o:, o:] = np.vstack([np.eye(n1)[1:], -np.ones((1, n1))])
    qd = (pool(draws["seasonal_drift_scales"])[:, 0] / ns) ** 2
  Tseason = Tseason @ Tm
  fc, var, pit, ll = np.zeros((N, Tb)), np.zeros((N, Tb)), np.zeros((N, Tb)), np.zeros(N)
  y = inp["y"][b].astype(np.float64)
  for t in range(Tb):
    pz = np.einsum("nij,j->ni", Pm, Z)
    F = pz @ Z + s_obs ** 2
    f = a @ Z + reg[:, t]
    fc[:, t], var[:, t] = f * scale + shift, F * scale * scale
    if not inp["mask"][b, t]:
      v = y[t] - f
      pit[:, t] = 0.5 * _erfc(-v / np.sqrt(2.0 * F))
      ll += -0.5 * (np.log(2.0 * np.pi * F) + v * v / F)
      a = a + pz * (v / F)[:, None]
      Pm = Pm - np.einsum("ni,nj->nij", pz, pz) / F[:, None, None]
    change = bool(ns) and bool(inp["sc"][0, t])
    Tt = Tseason if change else Tm
    a = a @ Tt.T
    Pm = np.einsum("ij,njk,lk->nil", Tt, Pm, Tt)
    Pm[:, 0, 0] += s_level ** 2
    if hs:
      Pm[:, 1, 1] += s_slope ** 2
    if change:
      Pm[:, o:, o:] += qd[:, None, None]
  return dict(forecast=fc, variance=var, pit=pit, loglik=ll)


def _oracle_loglik(inp, draws, b, has_slope, seasons):
  """oracle.kalman_loglik of y - X w for every fetched draw of series b."""
  Tb = inp["lengths"][b]
  spec = dict(inp["specs"][b], T=Tb, has_slope=int(has_slope), num_seasons=[s[0] for s in seasons],
              season_change=[inp["sc"][k, :Tb] for k in range(len(seasons))])
  pool = lambda a: a[b].reshape((a.shape[1] * a.shape[2],) + a.shape[3:]).astype(np.float64)
  s_obs, s_level, s_slope = (pool(draws[k]) for k in ("observation_noise_scale", "level_scale", "slope_scale"))
  drift, w = pool(draws["seasonal_drift_scales"]), pool(draws["weights"])
  y, mask = inp["y"][b, :Tb].astype(np.float64), inp["mask"][b, :Tb]
  out = np.zeros(s_obs.shape[0])
  for n in range(out.shape[0]):
    resid = y - (inp["X"][b, :Tb].astype(np.float64) @ w[n] if w.shape[1] else 0.0)
    ssm = orc.make_ssm(spec, mask, obs_scale=s_obs[n], level_scale=s_level[n],
                       slope_scale=s_slope[n] if has_slope else 0.0, drift_scale=drift[n])
    out[n] = orc.kalman_loglik(ssm, np.where(mask, 0.0, resid))
  return out


PARAM_FIELDS = ["observation_noise_scale", "level_scale", "slope_scale", "seasonal_drift_scales", "weights"]


@functools.lru_cache(maxsize=None)
def _run(lengths, P, has_slope, seasons, ragged=False, only=None, scale=SCALE, shift=SHIFT, distinct=False):
  """One session: its parameter draws, its prediction summary (all outputs, then pit_mean alone),
  the inputs as it holds them and the kernel it ran."""
  sess, inp = _open(list(lengths), P, has_slope, seasons, ragged, only, distinct=distinct)
  try:
    sess.run()
    draws = sess.fetch(PARAM_FIELDS)
    scale = np.asarray(scale, np.float64) if np.ndim(scale) else scale
    shift = np.asarray(shift, np.float64) if np.ndim(shift) else shift
    full = sess.summarize_predictions(scale, shift, RANKS)
    some = sess.summarize_predictions(scale, shift, RANKS, want=["pit_mean"])
    return draws, full, some, inp, sess.kernel_name()
  finally:
    sess.close()


def _check(full, inp, draws, has_slope, seasons, scales, shifts, what):
  """Every output of every series against the reference over the series' own steps (largest
  deviations printed), the log-likelihood against the oracle too, and the padding convention
  beyond each length."""
  worst = dict.fromkeys(OUTPUTS, 0.0)
  for b, Tb in enumerate(inp["lengths"]):
    ref = _reference(inp, draws, b, has_slope, seasons, scales[b], shifts[b])
    pairs = dict(forecast_mean=(full["forecast_mean"][b, :Tb], ref["forecast"].mean(axis=0)),
                 forecast_order=(full["forecast_order"][b, :, :Tb], np.sort(ref["forecast"], axis=0)[RANKS]),
                 variance_mean=(full["variance_mean"][b, :Tb], ref["variance"].mean(axis=0)),
                 pit_mean=(full["pit_mean"][b, :Tb], ref["pit"].mean(axis=0)),
                 loglik=(full["loglik"][b], ref["loglik"]))
    for k, (got, want) in pairs.items():
      worst[k] = max(worst[k], float(np.abs(got - want).max()))
    print(f"{what} series {b}: largest deviation " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, (got, want) in pairs.items():
      np.testing.assert_allclose(got, want, err_msg=f"{what} series {b} {k}", **TOL)
    np.testing.assert_allclose(full["loglik"][b], _oracle_loglik(inp, draws, b, has_slope, seasons),
                               err_msg=f"{what} series {b} loglik against the oracle", **TOL)
    assert (full["pit_mean"][b, :Tb][inp["mask"][b, :Tb]] == 0.0).all()
    # padding: f = 0, so the forecast reads the shift; variance and pit 0
    assert (full["forecast_mean"][b, Tb:] == shifts[b]).all() and (full["forecast_order"][b, :, Tb:] == shifts[b]).all()
    assert (full["variance_mean"][b, Tb:] == 0.0).all() and (full["pit_mean"][b, Tb:] == 0.0).all()


@pytest.mark.parametrize("has_slope", [False, True])
@pytest.mark.parametrize("P", [0, 1, 5, 37])         # 37 crosses the regression kernel's 32-column chunk
def test_trend_models_equal_numpy_on_the_fetched_draws(P, has_slope):
  draws, full, some, inp, name = _run((70, 70, 70), P, has_slope, ())
  print("kernel:", name)
  assert full["forecast_order"].shape == (3, len(RANKS), 70) and full["loglik"].shape == (3, 74)
  _check(full, inp, draws, has_slope, (), [SCALE] * 3, [SHIFT] * 3, f"P={P} slope={has_slope}")
  # only pit_mean requested: the other outputs are absent, the one asked for does not change
  assert list(some) == ["pit_mean"]
  np.testing.assert_array_equal(some["pit_mean"], full["pit_mean"])


@pytest.mark.parametrize("has_slope", [False, True])
@pytest.mark.parametrize("seasons", [((7, 1),), ((4, 2),)])
def test_one_seasonal_block_equals_numpy_on_the_fetched_draws(seasons, has_slope):
  draws, full, some, inp, name = _run((133, 133), 3, has_slope, seasons)
  print("kernel:", name)
  _check(full, inp, draws, has_slope, seasons, [SCALE] * 2, [SHIFT] * 2, f"seasons={seasons} slope={has_slope}")
  np.testing.assert_array_equal(some["pit_mean"], full["pit_mean"])


def test_the_filter_starts_from_every_series_own_distinct_prior_record():
  """Trend + slope + weekly block, three series fitted with three records in which init_level_loc and
  the three init_*_scale differ from each other, from the default's and between the series
  (tests/prior_cases.py): the filter of series b starts from record b.  The same tolerances; and the
  reference on a record with one field swapped is far off, so a reader of the wrong field fails."""
  seasons, lengths = ((7, 1),), (133, 133, 133)
  draws, full, _, inp, name = _run(lengths, 3, True, seasons, distinct=True)
  print("kernel:", name)
  _check(full, inp, draws, True, seasons, [SCALE] * 3, [SHIFT] * 3, "distinct record")
  for b in range(3):
    spec = inp["specs"][b]
    swaps = dict(init_level_loc=float(inp["y"][b][~inp["mask"][b]][0]), init_level_scale=spec["init_slope_scale"],
                 init_slope_scale=spec["init_level_scale"], init_seasonal_scale=spec["init_level_scale"],
                 other_series=None)
    for f, v in swaps.items():
      other = dict(inp, specs=[inp["specs"][(b + 1) % 3] if f == "other_series" else dict(spec, **{f: v})] * 3)
      ref = _reference(other, draws, b, True, seasons, SCALE, SHIFT)
      assert np.abs(full["loglik"][b] - ref["loglik"]).max() > 1e-3, (b, f)


@pytest.mark.parametrize("seasons", [(), ((7, 1),)])
def test_ragged_sessions_use_every_series_own_length(seasons):
  """Lengths 70, 41 and 64 in one launch (the seasonal stride rounded up to 72), each series with its
  own scale and shift; beyond a series' length the padding convention."""
  scale, shift = (3.7, 0.5, 2.0), (-12.25, 4.0, 0.0)
  draws, full, _, inp, name = _run((70, 41, 64), 3, False, seasons, ragged=True, scale=scale, shift=shift)
  print("kernel:", name)
  assert "ragged" in name and inp["T"] == (72 if seasons else 70)
  _check(full, inp, draws, False, seasons, scale, shift, f"ragged seasons={seasons}")


def test_a_batch_and_its_series_one_by_one_agree_bit_for_bit():
  """The batch of three as one session, and as three sessions of one series at series_offset 0, 1,
  2: all five outputs are equal."""
  _, whole, _, _, _ = _run((70, 70, 70), 5, True, ())
  for b in range(3):
    _, one, _, _, _ = _run((70, 70, 70), 5, True, (), only=b)
    for k in OUTPUTS:
      np.testing.assert_array_equal(one[k][0], whole[k][b], err_msg=f"series {b} {k}")


def test_errors_are_reported_before_any_device_work():
  fn = _native.load().ci_session_summarize_predictions
  sess, _ = _open([70], 3, False, ())
  one, ranks = np.ones(1), np.asarray([0, 73], np.int32)
  out = np.zeros((1, 70))

  def raw(scale, num_ranks):
    rc = fn(sess._h, None if scale is None else scale.ctypes.data, one.ctypes.data, num_ranks,  # pylint: disable=protected-access
            ranks.ctypes.data, out.ctypes.data, None, None, None, None)
    return rc, _native.load().ci_last_error().decode()

  try:
    with pytest.raises(_native.NativeError, match="needs a finished ci_session_run"):
      sess.summarize_predictions(1.0, 0.0, [0, 73])
    sess.run()
    rc, msg = raw(None, 2)
    assert rc != 0 and "NULL argument" in msg
    for num_ranks in (0, 9):
      rc, msg = raw(one, num_ranks)
      assert rc != 0 and f"num_ranks must be in [1, 8], got {num_ranks}" in msg
    with pytest.raises(_native.NativeError, match=r"rank 74 out of range \[0, 74\)"):
      sess.summarize_predictions(1.0, 0.0, [0, 74])
    with pytest.raises(ValueError, match="unknown prediction outputs"):
      sess.summarize_predictions(1.0, 0.0, [0], want=["pit"])
    assert sess.summarize_predictions(1.0, 0.0, [0, 73])["forecast_order"].shape == (1, 2, 70)
  finally:
    sess.close()
  two, _ = _open([70], 2, False, ((4, 1), (3, 1)))
  try:
    with pytest.raises(_native.NativeError, match=r"at most one block of 2 to 7 seasons.*\(4, 3\)"):
      two.summarize_predictions(1.0, 0.0, [0])
  finally:
    two.close()


# ---- package level: InferenceOptions(prediction_errors=True) ----------------------------------------

ALPHA, SEED = 0.1, 11
OPTS = dict(num_chains=2, num_results=37)
PANEL_LENGTHS = (70, 41, 64)


def _frames(lengths=(70, 70, 70)):
  idx = pd.date_range("2022-03-01", periods=max(lengths), freq="D")
  frames = []
  for b, Tb in enumerate(lengths):
    y, X = syn.make_raw_series(max(lengths), 2, 70 + b, effect=4.0 + b)
    frame = pd.DataFrame(np.column_stack([y, X]), index=idx, columns=["y", "x0", "x1"]).iloc[:Tb].copy()
    frame.iloc[9 + b, 0] = np.nan                       # a missing value inside the pre-period
    frames.append(frame)
  return frames


def _periods(frame, b):
  """A row or two before the pre-period, a gap before the post-period and a tail behind it."""
  last_pre = (6 * len(frame)) // 10 + b
  return ((frame.index[1 + b], frame.index[last_pre]), (frame.index[last_pre + 2], frame.index[len(frame) - 1 - b]))


@functools.lru_cache(maxsize=None)
def _single(b, lengths=(70, 70, 70), own=False, on=True, dtype=np.float32):
  frames = _frames(lengths)
  periods = _periods(frames[b], b) if own else _periods(frames[0], 0)
  return ci.fit_causalimpact(frames[b], *periods, alpha=ALPHA, seed=SEED,
                             data_options=ci.DataOptions(dtype=dtype),
                             inference_options=ci.InferenceOptions(prediction_errors=on, **OPTS)), periods


def _host_frames(one, frame, periods, dtype=np.float32):
  """The two frames built by `_prediction_summary_host` from the fit's `posterior_samples`, on the
  outcome, the design and the parameter block the sampler saw (`causalimpact_lib._run_sampler`)."""
  data = cid.CausalImpactData(frame, *periods, dtype=dtype)
  n_after = data.model_after_pre_data.shape[0]
  y = np.concatenate([np.asarray(data.outcome_ts.time_series, np.float64), np.full(n_after, np.nan)])
  mask = np.concatenate([np.asarray(data.outcome_ts.is_missing, bool), np.ones(n_after, bool)])
  design = np.asarray(data.feature_ts.values, np.float64)
  params = _model.series_params(y, mask, design, outcome_sd=float(np.nanstd(y[:y.shape[0] - n_after], ddof=1)))
  ps = one.posterior_samples
  N = np.asarray(ps.level_scale).shape[0]
  draws = dict(observation_noise_scale=np.asarray(ps.observation_noise_scale), level_scale=np.asarray(ps.level_scale),
               slope_scale=np.zeros(N), seasonal_drift_scales=np.zeros((N, 0)), weights=np.asarray(ps.weights))
  rq = lib._device_summary_request(data, ALPHA)                               # pylint: disable=protected-access
  ranks = lib._summary_ranks(N, rq["quantiles"])                              # pylint: disable=protected-access
  psum = lib._prediction_summary_host(                                         # pylint: disable=protected-access
      np.where(mask, 0.0, y).astype(dtype), mask, design.astype(dtype), np.zeros((0, y.shape[0]), np.uint8), [],
      False, params, draws, rq["scale"], rq["shift"], ranks)
  return lib._prediction_frames(psum, ranks, ALPHA, rq["observed"], ~mask, 1,  # pylint: disable=protected-access
                                lib.posterior_processing.model_index(data), data.data.index)


def _assert_close_to_host(one, frame, periods, dtype=np.float32):
  want_frame, want_quality = _host_frames(one, frame, periods, dtype)
  got = one.prediction_errors
  assert list(got.columns) == list(lib.PREDICTION_COLUMNS) and got.index.equals(one.series.index)
  np.testing.assert_array_equal(np.isnan(got.to_numpy()), np.isnan(want_frame.to_numpy()))
  print("largest deviation per column:", (got - want_frame).abs().max().to_dict())
  np.testing.assert_allclose(got.to_numpy(), want_frame.to_numpy(), **TOL)
  np.testing.assert_allclose(one.fit_quality.to_numpy(), want_quality.to_numpy(), **TOL)
  assert list(one.fit_quality.index) == list(lib.FIT_QUALITY_ENTRIES)
  # NaN placement: the rows before the pre-period everywhere; error, standardized_error and pit also
  # at the missing value, in the gap, the post-period and the tail
  pre = periods[0]
  before = got.index < pre[0]
  assert before.sum() >= 1 and got[before].isna().all().all()
  seen = (got.index >= pre[0]) & (got.index <= pre[1]) & frame["y"].notna().to_numpy()
  assert not got.loc[~before, ["forecast", "forecast_lower", "forecast_upper", "forecast_sd"]].isna().any().any()
  for col in ("error", "standardized_error", "pit"):
    np.testing.assert_array_equal(got[col].notna().to_numpy(), seen)
  assert one.fit_quality["n_scored"] == seen.sum() - 1          # (state dimension 1: step 0 is not scored)


def test_single_fit_on_the_device_route_equals_the_host_summary_and_disturbs_nothing():
  frames = _frames()
  (one, periods), (off, _) = _single(0), _single(0, on=False)
  _assert_close_to_host(one, frames[0], periods)
  assert off.prediction_errors is None and off.fit_quality is None
  pd.testing.assert_frame_equal(one.series, off.series, check_exact=True)
  pd.testing.assert_frame_equal(one.summary, off.summary, check_exact=True)
  for f in (f.name for f in dataclasses.fields(one.posterior_samples)):
    a, b = getattr(one.posterior_samples, f), getattr(off.posterior_samples, f)
    assert (a is None and b is None) or np.array_equal(np.asarray(a), np.asarray(b)), f
  assert dict(one.diagnostics) == dict(off.diagnostics)
  assert one.components is None and one.coefficients is None


def _assert_frames_equal_single_bit_for_bit(mine, one):
  pd.testing.assert_frame_equal(mine.prediction_errors, one.prediction_errors, check_exact=True)
  pd.testing.assert_series_equal(mine.fit_quality, one.fit_quality, check_exact=True)


def test_batch_frames_equal_the_single_fits_bit_for_bit():
  frames = _frames()
  periods = _periods(frames[0], 0)
  got = ci.fit_causalimpact_batch(frames, *periods, alpha=ALPHA, seed=SEED, shared_streams=True,
                                  inference_options=ci.InferenceOptions(prediction_errors=True, **OPTS))
  assert type(got) is ci.CausalImpactBatchAnalysis             # (the one-launch route)
  quality = got.fit_quality
  assert quality.shape == (3, len(lib.FIT_QUALITY_ENTRIES)) and list(quality.index) == [0, 1, 2]
  for b in range(3):
    one, _ = _single(b)
    _assert_frames_equal_single_bit_for_bit(got[b], one)
    pd.testing.assert_series_equal(quality.iloc[b], one.fit_quality, check_exact=True, check_names=False)
  off = ci.fit_causalimpact_batch(frames, *periods, alpha=ALPHA, seed=SEED, shared_streams=True,
                                  inference_options=ci.InferenceOptions(**OPTS))
  assert off.fit_quality is None and off[1].prediction_errors is None
  pd.testing.assert_frame_equal(off.summary, got.summary, check_exact=True)
  pd.testing.assert_frame_equal(off[1].series, got[1].series, check_exact=True)


def test_panel_frames_equal_the_single_fits_bit_for_bit():
  """Lengths 70, 41 and 64 with their own periods in the ragged launch; every frame on the series'
  own index."""
  frames = _frames(PANEL_LENGTHS)
  got = ci.fit_causalimpact_panel(frames, [_periods(f, b) for b, f in enumerate(frames)], alpha=ALPHA,
                                  seed=SEED, shared_streams=True,
                                  inference_options=ci.InferenceOptions(prediction_errors=True, **OPTS))
  assert type(got) is ci.CausalImpactPanelAnalysis
  assert got.fit_quality.shape == (3, len(lib.FIT_QUALITY_ENTRIES))
  for b in range(3):
    one, _ = _single(b, PANEL_LENGTHS, own=True)
    assert got[b].prediction_errors.index.equals(frames[b].index)
    _assert_frames_equal_single_bit_for_bit(got[b], one)
    pd.testing.assert_series_equal(got.fit_quality.iloc[b], one.fit_quality, check_exact=True, check_names=False)


def test_float64_fit_takes_the_host_route():
  frames = _frames()
  one, periods = _single(0, dtype=np.float64)
  _assert_close_to_host(one, frames[0], periods, np.float64)
