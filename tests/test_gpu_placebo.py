"""ci_session_summarize_placebo on the device -- forecasts of the sum of the next H observations from
origins inside the observed series, without updates -- at session level against numpy written here,
from the parameter draws fetched from the same session, and at package level (`placebo=`) against
`_placebo_summary_host` on the same fit's draws.

The shapes of tests/test_gpu_predictions.py: T = 70, C = 2 and S = 37 give N = 74 draws (one full
wavefront of lanes and a remainder); the steps 11, 12 and 40 are missing, so some windows contain
gaps and one origin is itself missing.  The origins include two adjacent steps and the last
admissible one; H is 1 and 9.  Every comparison with numpy is to rtol 1e-8, atol 1e-8, the project's
float64 contract (tests/test_gpu_float64.py)."""
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

import prior_cases

pytestmark = pytest.mark.gpu

SCALE, SHIFT = 3.7, -12.25
TOL = dict(rtol=1e-8, atol=1e-8)
OUTPUTS = ("predicted_mean", "spread_mean", "pit_mean")
PARAM_FIELDS = ["observation_noise_scale", "level_scale", "slope_scale", "seasonal_drift_scales", "weights"]
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def _origins(Tb, H):
  """Early origins (3 and 4 adjacent; the window of 4 reaches the gap at 11, 12 when H = 9), the
  missing step 11, one whose window holds step 40, and the last admissible one; two unused slots."""
  return [3, 4, 11, 35, Tb - H, -1, -1]


def _series(T, P, seed, has_slope, seasons, distinct=None):
  """Sampler inputs of one series with P design columns (the intercept is the last one); the steps
  11, 12 and 40 are missing; the last 30 % are the masked post-period."""
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


def _reference(inp, draws, b, has_slope, seasons, scale, shift, origins, H):
  """The definitions of include/causalimpact_amd.h in numpy for series b, all N draws at once with
  dense d x d matrices: SUM, SPREAD, PIT [O, N]."""
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
  qd = None
  if ns:
    Z[o] = 1.0
    Pm[:, o:, o:] = spec["init_seasonal_scale"] ** 2 * (np.eye(n1) - 1.0 / ns)
    Tseason[o:, o:] = np.vstack([np.eye(n1)[1:], -np.ones((1, n1))])
    qd = (pool(draws["seasonal_drift_scales"])[:, 0] / ns) ** 2
  Tseason = Tseason @ Tm
  y, mask = inp["y"][b].astype(np.float64), inp["mask"][b]

  def step(t, a, Pm, r=None):                       # t -> t + 1 on the mean, the covariance and r
    change = bool(ns) and bool(inp["sc"][0, t])
    Tt = Tseason if change else Tm
    Pm = np.einsum("ij,njk,lk->nil", Tt, Pm, Tt)
    Pm[:, 0, 0] += s_level ** 2
    if hs:
      Pm[:, 1, 1] += s_slope ** 2
    if change:
      Pm[:, o:, o:] += qd[:, None, None]
    return a @ Tt.T, Pm, None if r is None else r @ Tt.T

  out = np.zeros((3, len(origins), N))
  for t in range(Tb):
    if t in origins:
      i = origins.index(t)
      fa, fP, r = a, Pm, np.zeros((N, d))
      C, V, A, cnt = np.zeros(N), np.zeros(N), 0.0, 0
      for h in range(H):
        pz = np.einsum("nij,j->ni", fP, Z)
        if not mask[t + h]:
          C, A, cnt = C + (fa @ Z + reg[:, t + h]), A + y[t + h], cnt + 1
          V = V + 2.0 * (r @ Z) + pz @ Z + s_obs ** 2
          r = r + pz
        if h + 1 < H:
          fa, fP, r = step(t + h, fa, fP, r)
      if cnt:
        out[0, i] = C * scale + cnt * shift
        out[1, i] = (V + (A - C) ** 2) * scale * scale
        out[2, i] = 0.5 * _erfc(-(A - C) / np.sqrt(2.0 * V))
    pz = np.einsum("nij,j->ni", Pm, Z)
    if not mask[t]:
      F = pz @ Z + s_obs ** 2
      v = y[t] - (a @ Z + reg[:, t])
      a = a + pz * (v / F)[:, None]
      Pm = Pm - np.einsum("ni,nj->nij", pz, pz) / F[:, None, None]
    if t + 1 < Tb:
      a, Pm, _ = step(t, a, Pm)
  return out


def _plan(lengths, H):
  """origins [B, 7] and horizon [B]: H a number, or one horizon per series."""
  Hs = [H] * len(lengths) if np.ndim(H) == 0 else list(H)
  return np.array([_origins(Tb, h) for Tb, h in zip(lengths, Hs)], np.int32), np.array(Hs, np.int32)


@functools.lru_cache(maxsize=None)
def _run(lengths, P, has_slope, seasons, H, ragged=False, only=None, scale=SCALE, shift=SHIFT, distinct=False):
  """One session: its parameter draws, its placebo summary (all outputs, then pit_mean alone), its
  prediction summary, the inputs as it holds them and the kernel it ran."""
  sess, inp = _open(list(lengths), P, has_slope, seasons, ragged, only, distinct=distinct)
  try:
    sess.run()
    draws = sess.fetch(PARAM_FIELDS)
    scale = np.asarray(scale, np.float64) if np.ndim(scale) else scale
    shift = np.asarray(shift, np.float64) if np.ndim(shift) else shift
    origins, horizon = _plan(inp["lengths"] if only is None else [lengths[only]], H)
    full = sess.summarize_placebo(scale, shift, origins, horizon)
    some = sess.summarize_placebo(scale, shift, origins, horizon, want=["pit_mean"])
    pred = sess.summarize_predictions(scale, shift, [0], want=["forecast_mean", "pit_mean"])
    return draws, full, some, pred, inp, sess.kernel_name()
  finally:
    sess.close()


def _check(full, inp, draws, has_slope, seasons, scales, shifts, H, what):
  origins, horizon = _plan(inp["lengths"], H)
  worst = dict.fromkeys(OUTPUTS, 0.0)
  for b in range(len(inp["lengths"])):
    used = [int(o) for o in origins[b] if o >= 0]
    ref = _reference(inp, draws, b, has_slope, seasons, scales[b], shifts[b], used, int(horizon[b]))
    for j, k in enumerate(OUTPUTS):
      worst[k] = max(worst[k], float(np.abs(full[k][b, :len(used)] - ref[j].mean(axis=1)).max()))
    print(f"{what} series {b}: largest deviation " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for j, k in enumerate(OUTPUTS):
      assert full[k].shape == origins.shape
      np.testing.assert_allclose(full[k][b, :len(used)], ref[j].mean(axis=1), err_msg=f"{what} series {b} {k}", **TOL)
      assert (full[k][b, len(used):] == 0.0).all()              # the unused slots
    counted = np.array([(~inp["mask"][b, o:o + int(horizon[b])]).sum() for o in used])
    for k in OUTPUTS:                                           # a window without observation reads 0
      assert ((full[k][b, :len(used)] == 0.0) == (counted == 0)).all()
    assert (counted < horizon[b]).any()


@pytest.mark.parametrize("H", [1, 9])
@pytest.mark.parametrize("has_slope", [False, True])
@pytest.mark.parametrize("P", [0, 5, 37])            # 37 crosses the regression kernel's 32-column chunk
def test_trend_models_equal_numpy_on_the_fetched_draws(P, has_slope, H):
  draws, full, some, _, inp, name = _run((70, 70, 70), P, has_slope, (), H)
  print("kernel:", name)
  _check(full, inp, draws, has_slope, (), [SCALE] * 3, [SHIFT] * 3, H, f"P={P} slope={has_slope} H={H}")
  # only pit_mean requested: the other outputs are absent, the one asked for does not change
  assert list(some) == ["pit_mean"]
  np.testing.assert_array_equal(some["pit_mean"], full["pit_mean"])


@pytest.mark.parametrize("H", [1, 9])
@pytest.mark.parametrize("has_slope", [False, True])
@pytest.mark.parametrize("seasons", [((7, 1),), ((4, 2),)])
def test_one_seasonal_block_equals_numpy_on_the_fetched_draws(seasons, has_slope, H):
  draws, full, some, _, inp, name = _run((133, 133), 3, has_slope, seasons, H)
  print("kernel:", name)
  _check(full, inp, draws, has_slope, seasons, [SCALE] * 2, [SHIFT] * 2, H, f"seasons={seasons} slope={has_slope} H={H}")
  np.testing.assert_array_equal(some["pit_mean"], full["pit_mean"])


def test_the_forecasts_start_from_every_series_own_distinct_prior_record():
  """Trend + slope + weekly block, three series fitted with three records in which init_level_loc and
  the three init_*_scale differ from each other, from the default's and between the series
  (tests/prior_cases.py).  The same tolerances; the early origins (3 and 4) still feel the initial
  state, and the reference on a record with one field swapped is far off there."""
  seasons, lengths, H = ((7, 1),), (133, 133, 133), 9
  draws, full, _, _, inp, name = _run(lengths, 3, True, seasons, H, distinct=True)
  print("kernel:", name)
  _check(full, inp, draws, True, seasons, [SCALE] * 3, [SHIFT] * 3, H, "distinct record")
  origins, _ = _plan(inp["lengths"], H)
  for b in range(3):
    spec = inp["specs"][b]
    used = [int(o) for o in origins[b] if o >= 0]
    swaps = dict(init_level_loc=float(inp["y"][b][~inp["mask"][b]][0]), init_level_scale=spec["init_slope_scale"],
                 init_slope_scale=spec["init_level_scale"], init_seasonal_scale=spec["init_level_scale"],
                 other_series=None)
    for f, v in swaps.items():
      other = dict(inp, specs=[inp["specs"][(b + 1) % 3] if f == "other_series" else dict(spec, **{f: v})] * 3)
      ref = _reference(other, draws, b, True, seasons, SCALE, SHIFT, used, H)
      moved = max(float(np.abs(full[k][b, :len(used)] - ref[j].mean(axis=1)).max()) for j, k in enumerate(OUTPUTS))
      assert moved > 1e-3, (b, f, moved)


@pytest.mark.parametrize("seasons", [(), ((7, 1),)])
def test_ragged_sessions_use_every_series_own_length_horizon_and_origins(seasons):
  """Lengths 70, 41 and 64 in one launch (the seasonal stride rounded up to 72), each series with its
  own scale, shift, horizon and origins (the last one at its own length minus its horizon)."""
  scale, shift, H = (3.7, 0.5, 2.0), (-12.25, 4.0, 0.0), (9, 1, 5)
  draws, full, _, _, inp, name = _run((70, 41, 64), 3, False, seasons, H, ragged=True, scale=scale, shift=shift)
  print("kernel:", name)
  assert "ragged" in name and inp["T"] == (72 if seasons else 70)
  _check(full, inp, draws, False, seasons, scale, shift, H, f"ragged seasons={seasons}")


def test_a_batch_and_its_series_one_by_one_agree_bit_for_bit():
  _, whole, _, _, _, _ = _run((70, 70, 70), 5, True, (), 9)
  for b in range(3):
    _, one, _, _, _, _ = _run((70, 70, 70), 5, True, (), 9, only=b)
    for k in OUTPUTS:
      np.testing.assert_array_equal(one[k][0], whole[k][b], err_msg=f"series {b} {k}")


@pytest.mark.parametrize("has_slope,seasons,lengths", [(True, (), (70, 70, 70)), (False, ((7, 1),), (133, 133))])
def test_horizon_one_is_the_one_step_forecast_bit_for_bit(has_slope, seasons, lengths):
  """H = 1 at observed origins: predicted_mean and pit_mean are `summarize_predictions`'
  forecast_mean and pit_mean there; at the missing origin 11 the window counts nothing."""
  P = 5 if not seasons else 3
  _, full, _, pred, inp, _ = _run(lengths, P, has_slope, seasons, 1)
  origins, _ = _plan(inp["lengths"], 1)
  for b in range(len(lengths)):
    seen = [i for i, o in enumerate(origins[b]) if o >= 0 and not inp["mask"][b, o]]
    assert len(seen) == 3                   # (3, 4 and 35: 11 is missing, the last step lies in the post-period)
    at = origins[b][seen]
    np.testing.assert_array_equal(full["predicted_mean"][b, seen], pred["forecast_mean"][b, at])
    np.testing.assert_array_equal(full["pit_mean"][b, seen], pred["pit_mean"][b, at])
    assert full["predicted_mean"][b, 2] == 0.0 and full["pit_mean"][b, 2] == 0.0


def test_errors_are_reported_before_any_device_work():
  fn = _native.load().ci_session_summarize_placebo
  sess, _ = _open([70, 70], 3, False, ())
  one, out = np.ones(2), np.zeros((2, 2))
  good = np.array([[3, 9], [3, -1]], np.int32)
  hz = np.array([5, 5], np.int32)

  def raw(scale, origins, horizon, O=2):
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = fn(sess._h, ptr(scale), one.ctypes.data, O, ptr(origins), ptr(horizon), out.ctypes.data, None, None)  # pylint: disable=protected-access
    return rc, _native.load().ci_last_error().decode()

  try:
    with pytest.raises(_native.NativeError, match="needs a finished ci_session_run"):
      sess.summarize_placebo(1.0, 0.0, good, 5)
    sess.run()
    for args in ((None, good, hz), (one, None, hz), (one, good, None)):
      rc, msg = raw(*args)
      assert rc != 0 and "NULL argument" in msg
    for O in (0, 71):
      rc, msg = raw(one, good, hz, O)
      assert rc != 0 and f"max_origins must be in [1, 70], got {O}" in msg
    with pytest.raises(_native.NativeError, match=r"horizon\[1\] must be at least 1, got 0"):
      sess.summarize_placebo(1.0, 0.0, good, [5, 0])
    for bad in ([[3, 3], [3, -1]], [[9, 3], [3, -1]], [[3, 9], [-1, 3]]):
      with pytest.raises(_native.NativeError, match="strictly ascending with the unused slots"):
        sess.summarize_placebo(1.0, 0.0, bad, 5)
    with pytest.raises(_native.NativeError, match="must be a step or -1"):
      sess.summarize_placebo(1.0, 0.0, [[3, 9], [-2, -1]], 5)
    with pytest.raises(_native.NativeError, match=r"origins\[0, 1\] = 66 with horizon 5 reaches beyond the series' 70 steps"):
      sess.summarize_placebo(1.0, 0.0, [[3, 66], [3, -1]], 5)
    with pytest.raises(ValueError, match="unknown placebo outputs"):
      sess.summarize_placebo(1.0, 0.0, good, 5, want=["pit"])
    with pytest.raises(ValueError, match=r"`origins` must be \[2, O\]"):
      sess.summarize_placebo(1.0, 0.0, [3, 9], 5)
    got = sess.summarize_placebo(1.0, 0.0, [[3, 65], [3, -1]], 5)       # 65 + 5 = 70: the last admissible
    assert got["predicted_mean"].shape == (2, 2) and got["predicted_mean"][1, 1] == 0.0
  finally:
    sess.close()
  # a ragged session checks against every series' own length
  rag, _ = _open([70, 41], 3, False, (), ragged=True)
  try:
    rag.run()
    with pytest.raises(_native.NativeError, match=r"origins\[1, 0\] = 37 with horizon 5 reaches beyond the series' 41 steps"):
      rag.summarize_placebo(1.0, 0.0, [[65], [37]], 5)
    assert rag.summarize_placebo(1.0, 0.0, [[65], [36]], 5)["pit_mean"].shape == (2, 1)
  finally:
    rag.close()
  two, _ = _open([70], 2, False, ((4, 1), (3, 1)))
  try:
    with pytest.raises(_native.NativeError, match=r"ci_session_summarize_placebo takes a trend with at most "
                                                  r"one block of 2 to 7 seasons.*\(4, 3\)"):
      two.summarize_placebo(1.0, 0.0, [3], 5)
  finally:
    two.close()


# ---- package level: placebo= ---------------------------------------------------------------------

ALPHA, SEED = 0.1, 11
OPTS = dict(num_chains=2, num_results=37)
PANEL_LENGTHS = (70, 41, 64)
PLACEBO = ci.Placebo(max_origins=6)
NUMERIC = [c for c in lib.PLACEBO_COLUMNS if c not in ("horizon_end", "significant")]


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
def _single(b, lengths=(70, 70, 70), own=False, on=True):
  frames = _frames(lengths)
  periods = _periods(frames[b], b) if own else _periods(frames[0], 0)
  return ci.fit_causalimpact(frames[b], *periods, alpha=ALPHA, seed=SEED, placebo=PLACEBO if on else None,
                             inference_options=ci.InferenceOptions(**OPTS)), periods


def _host_frames(one, frame, periods):
  """(placebo, placebo_quality) built by `_placebo_summary_host` from the fit's `posterior_samples`,
  on the outcome, the design and the parameter block the sampler saw (`causalimpact_lib._run_sampler`)."""
  data = cid.CausalImpactData(frame, *periods, dtype=np.float32)
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
  n_pre, n_post = y.shape[0] - n_after, int(np.count_nonzero(rq["flags"] & 2))
  H, origins = lib.placebo_plan(PLACEBO, n_pre, n_post, 1)
  y_seen = np.where(mask, 0.0, y).astype(np.float32)
  psum = lib._placebo_summary_host(                                            # pylint: disable=protected-access
      y_seen, mask, design.astype(np.float32), np.zeros((0, y.shape[0]), np.uint8), [], False, params, draws,
      rq["scale"], rq["shift"], origins, H)
  cnt, seen = lib._placebo_seen(y_seen, mask, origins, H, rq["scale"], rq["shift"])   # pylint: disable=protected-access
  psum.update(n_counted=cnt, seen_sum=seen)
  return lib._placebo_frames(psum, origins, H, ALPHA, rq["observed"],          # pylint: disable=protected-access
                             lib.posterior_processing.model_index(data), n_post,
                             one.summary.loc["cumulative", "rel_effect"])


def _assert_close(got_frame, got_quality, want_frame, want_quality, what):
  assert list(got_frame.columns) == list(lib.PLACEBO_COLUMNS) and got_frame.index.equals(want_frame.index)
  assert len(got_frame) >= 3
  print(what, "largest deviation per column:", (got_frame[NUMERIC] - want_frame[NUMERIC]).abs().max().to_dict())
  np.testing.assert_allclose(got_frame[NUMERIC].to_numpy(np.float64), want_frame[NUMERIC].to_numpy(np.float64), **TOL)
  assert list(got_frame["horizon_end"]) == list(want_frame["horizon_end"])
  assert list(got_frame["significant"]) == list(want_frame["significant"])
  assert list(got_quality.index) == list(lib.PLACEBO_QUALITY_ENTRIES)
  np.testing.assert_allclose(got_quality.to_numpy(), want_quality.to_numpy(), **TOL)


def test_single_fit_on_the_device_route_equals_the_host_summary_and_disturbs_nothing():
  frames = _frames()
  (one, periods), (off, _) = _single(0), _single(0, on=False)
  _assert_close(one.placebo, one.placebo_quality, *_host_frames(one, frames[0], periods), "single fit")
  assert ((one.placebo["pit"] > 0) & (one.placebo["pit"] < 1)).all() and (one.placebo["predicted_sd"] > 0).all()
  assert off.placebo is None and off.placebo_quality is None
  pd.testing.assert_frame_equal(one.series, off.series, check_exact=True)
  pd.testing.assert_frame_equal(one.summary, off.summary, check_exact=True)


def test_batch_frames_equal_the_host_summary_of_every_series_own_fit():
  frames = _frames()
  periods = _periods(frames[0], 0)
  got = ci.fit_causalimpact_batch(frames, *periods, alpha=ALPHA, seed=SEED, shared_streams=True,
                                  placebo=PLACEBO, inference_options=ci.InferenceOptions(**OPTS))
  assert type(got) is ci.CausalImpactBatchAnalysis             # (the one-launch route)
  quality = got.placebo_quality
  assert quality.shape == (3, len(lib.PLACEBO_QUALITY_ENTRIES)) and list(quality.index) == [0, 1, 2]
  for b in range(3):
    one, _ = _single(b)                                         # (shared streams: the same draws)
    want_frame, want_quality = _host_frames(one, frames[b], periods)
    _assert_close(got[b].placebo, got[b].placebo_quality, want_frame, want_quality, f"batch series {b}")
    np.testing.assert_allclose(quality.iloc[b].to_numpy(), want_quality.to_numpy(), **TOL)
  off = ci.fit_causalimpact_batch(frames, *periods, alpha=ALPHA, seed=SEED, shared_streams=True,
                                  inference_options=ci.InferenceOptions(**OPTS))
  assert off.placebo_quality is None and off[1].placebo is None
  pd.testing.assert_frame_equal(off.summary, got.summary, check_exact=True)
  pd.testing.assert_frame_equal(off[1].series, got[1].series, check_exact=True)


def test_panel_frames_equal_the_host_summary_of_every_series_own_fit():
  """Lengths 70, 41 and 64 with their own periods in the ragged launch: every series with the
  horizon and the origins of its own periods, on its own index."""
  frames = _frames(PANEL_LENGTHS)
  got = ci.fit_causalimpact_panel(frames, [_periods(f, b) for b, f in enumerate(frames)], alpha=ALPHA,
                                  seed=SEED, shared_streams=True, placebo=PLACEBO,
                                  inference_options=ci.InferenceOptions(**OPTS))
  assert type(got) is ci.CausalImpactPanelAnalysis
  assert got.placebo_quality.shape == (3, len(lib.PLACEBO_QUALITY_ENTRIES))
  horizons = set()
  for b in range(3):
    one, periods = _single(b, PANEL_LENGTHS, own=True)
    want_frame, want_quality = _host_frames(one, frames[b], periods)
    _assert_close(got[b].placebo, got[b].placebo_quality, want_frame, want_quality, f"panel series {b}")
    np.testing.assert_allclose(got.placebo_quality.iloc[b].to_numpy(), want_quality.to_numpy(), **TOL)
    horizons.add(got.placebo_quality.iloc[b]["horizon"])
  assert len(horizons) > 1


@pytest.mark.parametrize("route", ["two_blocks", "hmc"])
def test_batches_the_device_filter_does_not_take_run_the_numpy_route_inside_the_launch(route):
  """A model with two seasonal blocks (Gibbs) and the one-launch HMC batch: the launch fetches its
  parameter draws and `_placebo_summary_host` forecasts from them.  With shared streams every series
  has the draws of its single fit, which takes the numpy route too: the frames agree."""
  frames = _frames()
  periods = _periods(frames[0], 0)
  kw = dict(alpha=ALPHA, seed=SEED, placebo=PLACEBO)
  if route == "hmc":
    kw["inference_options"] = ci.InferenceOptions(sampler="hmc", num_chains=2, num_results=20, num_warmup_steps=20)
  else:
    kw["inference_options"] = ci.InferenceOptions(**OPTS)
    kw["model_options"] = ci.ModelOptions(seasons=[ci.Seasons(4), ci.Seasons(3)])
  got = ci.fit_causalimpact_batch(frames, *periods, shared_streams=True, **kw)
  assert type(got) is ci.CausalImpactBatchAnalysis             # (one launch, not series by series)
  assert got.placebo_quality.shape == (3, len(lib.PLACEBO_QUALITY_ENTRIES))
  for b in range(3):
    one = ci.fit_causalimpact(frames[b], *periods, **kw)
    _assert_close(got[b].placebo, got[b].placebo_quality, one.placebo, one.placebo_quality, f"{route} series {b}")
    assert (one.placebo["predicted_sd"] > 0).all()
