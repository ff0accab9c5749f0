"""ci_session_summarize_placebo_horizons on the device: the placebo forecasts of every origin at
several horizons from one filter pass -- bit for bit what K calls of ci_session_summarize_placebo
return (the entry this one was built next to, not the code under test), independent of the chunking,
and against numpy written here; then `Placebo(horizons=...)` at package level.

The shapes of tests/test_gpu_placebo.py: T = 70, 2 chains x 37 draws (N = 74: one full wavefront and a
remainder), the steps 11, 12 and 40 missing; origins [3, 4, 11, 35, T_b - 9, -1, -1]: adjacent ones, a
missing one, the last admissible one and unused slots; horizons [1, 2, 9, -1]: h = 1 and h = 2 from
origin 11 count nothing (those rows are 0), h = 9 crosses the gaps, one slot is unused.  Every
comparison with numpy is to rtol 1e-8, atol 1e-8, the project's float64 contract."""
import functools
import math
import re

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _model
from causalimpact import _native
from causalimpact import causalimpact_lib as lib

import test_gpu_placebo as base

pytestmark = pytest.mark.gpu

SCALE, SHIFT = base.SCALE, base.SHIFT
TOL = dict(rtol=1e-8, atol=1e-8)
OUTPUTS = _native.PLACEBO_OUTPUTS
HORIZONS = [1, 2, 9, -1]
HMAX = 9
# no slope and no block, slope alone, slope + 7 seasons, no slope + 2 seasons
MODELS = [(False, ()), (True, ()), (True, ((7, 1),)), (False, ((2, 1),))]
BATCH, RAGGED = (70, 70, 70), (70, 47, 64)
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def _plan(lengths):
  """origins [B, 7] and horizons [B, 4]; in a batch of three the last series has a row of its own
  ([2, 5, -1, -1]: two unused slots, another last horizon)."""
  origins = np.array([base._origins(Tb, HMAX) for Tb in lengths], np.int32)   # pylint: disable=protected-access
  horizons = np.array([HORIZONS] * len(lengths), np.int32)
  if len(lengths) == 3:
    horizons[2] = [2, 5, -1, -1]
  return origins, horizons


def _one_by_one(sess, scale, shift, origins, horizons):
  """The table from K calls of `summarize_placebo`, [B, O, K] per output: column k of the series whose
  slot k is used (the others get a valid horizon and are not read), 0 in the unused horizon slots."""
  B, K = horizons.shape
  want = {k: np.zeros(origins.shape + (K,)) for k in OUTPUTS}
  for k in range(K):
    used = horizons[:, k] > 0
    if not used.any():
      continue
    got = sess.summarize_placebo(scale, shift, origins, np.where(used, horizons[:, k], 1))
    for name in OUTPUTS:
      want[name][used, :, k] = got[name][used]
  return want


def _assert_same_bits(got, want, what):
  for name in OUTPUTS:
    assert got[name].shape == want[name].shape and got[name].dtype == np.float64
    np.testing.assert_array_equal(got[name], want[name], err_msg=f"{what} {name}")


@functools.lru_cache(maxsize=None)
def _fit(lengths, P, has_slope, seasons, ragged=False):
  """One finished session's table, the K single-horizon calls on the same session, its draws and inputs."""
  sess, inp = base._open(list(lengths), P, has_slope, seasons, ragged)        # pylint: disable=protected-access
  try:
    sess.run()
    draws = sess.fetch(base.PARAM_FIELDS)
    origins, horizons = _plan(inp["lengths"])
    scale = np.array([SCALE, 0.5, 2.0]) if ragged else SCALE
    shift = np.array([SHIFT, 4.0, 0.0]) if ragged else SHIFT
    got = sess.summarize_placebo_horizons(scale, shift, origins, horizons)
    want = _one_by_one(sess, scale, shift, origins, horizons)
    some = sess.summarize_placebo_horizons(scale, shift, origins, horizons, want=["spread_mean"])
    per = 3 * origins.shape[1] * horizons.shape[1]
    chunked = sess.summarize_placebo_horizons(scale, shift, origins, horizons, max_rows=per)
    roomy = sess.summarize_placebo_horizons(scale, shift, origins, horizons, max_rows=2 * per + 1)
    with pytest.raises(_native.NativeError, match=f"max_rows must hold the {per} rows of one series"):
      sess.summarize_placebo_horizons(scale, shift, origins, horizons, max_rows=per - 1)
    return dict(got=got, want=want, some=some, chunked=chunked, roomy=roomy, draws=draws, inp=inp,
                origins=origins, horizons=horizons, scale=np.broadcast_to(scale, (len(lengths),)),
                shift=np.broadcast_to(shift, (len(lengths),)), kernel=sess.kernel_name())
  finally:
    sess.close()


# ---- 1. the bit contract against the existing entry -----------------------------------------------

@pytest.mark.parametrize("P", [0, 3])
@pytest.mark.parametrize("has_slope,seasons", MODELS)
def test_a_batch_equals_one_call_per_horizon_bit_for_bit(has_slope, seasons, P):
  run = _fit(BATCH, P, has_slope, seasons)
  _assert_same_bits(run["got"], run["want"], f"batch slope={has_slope} seasons={seasons} P={P}")
  got, origins, horizons = run["got"], run["origins"], run["horizons"]
  for name in OUTPUTS:
    assert (got[name][:, 5:, :] == 0.0).all()                    # the unused origin slots
    assert (got[name][:2, :, 3] == 0.0).all() and (got[name][2, :, 2:] == 0.0).all()   # the unused horizon slots
    assert (got[name][:2, 2, :2] == 0.0).all()                   # h = 1, 2 from the missing origin 11: nothing counted
    assert (got[name][:2, 2, 2] != 0.0).all() and (got[name][:, :2, :2] != 0.0).all()
  assert list(run["some"]) == ["spread_mean"]
  np.testing.assert_array_equal(run["some"]["spread_mean"], got["spread_mean"])
  assert origins.shape == (3, 7) and horizons.shape == (3, 4)


@pytest.mark.parametrize("P", [0, 3])
@pytest.mark.parametrize("has_slope,seasons", MODELS)
def test_a_ragged_session_equals_one_call_per_horizon_bit_for_bit(has_slope, seasons, P):
  run = _fit(RAGGED, P, has_slope, seasons, ragged=True)
  assert "ragged" in run["kernel"] and run["inp"]["lengths"] == list(RAGGED)
  _assert_same_bits(run["got"], run["want"], f"ragged slope={has_slope} seasons={seasons} P={P}")
  assert (run["got"]["pit_mean"][:, :5, 0] != 0.0).sum() == 8    # (origins 3 and 4 everywhere, 35 where it is observed)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("P", [0, 3])
@pytest.mark.parametrize("has_slope,seasons", MODELS)
def test_a_session_made_from_draws_equals_one_call_per_horizon_bit_for_bit(has_slope, seasons, P, dtype):
  """float32: the fit's own draws (and the fit's own table, bit for bit); float64: the same draws and
  data moved off the float32 grid, so the float64 build has something of its own to read."""
  run = _fit(BATCH, P, has_slope, seasons)
  inp, draws = run["inp"], dict(run["draws"])
  y, X = inp["y"], inp["X"]
  if dtype is np.float64:
    rng = np.random.default_rng(7)
    wiggle = lambda a: np.asarray(a, np.float64) * (1.0 + 1e-9 * rng.standard_normal(np.shape(a)))
    draws = {k: wiggle(v) for k, v in draws.items()}
    y, X = wiggle(y), None if X is None else wiggle(X)
  K = len(seasons)
  pb = _native.make_problem(T=inp["T"], P=P, has_slope=has_slope, num_warmup=0, num_results=37, num_chains=2,
                            num_series=3, seed=(5, 9), num_seasons=_model.expand_seasons(seasons, 1)[0])
  if not K:
    draws.pop("seasonal_drift_scales", None)
  if not has_slope:
    draws.pop("slope_scale", None)
  if not P:
    draws.pop("weights", None)
  drawn = _native.DrawsSession(pb, y, inp["mask"], X, inp["sc"] if K else None, _native.make_params(inp["specs"]),
                               draws, dtype=dtype)
  try:
    got = drawn.summarize_placebo_horizons(SCALE, SHIFT, run["origins"], run["horizons"])
    want = _one_by_one(drawn, SCALE, SHIFT, run["origins"], run["horizons"])
  finally:
    drawn.close()
  _assert_same_bits(got, want, f"draws {np.dtype(dtype)} slope={has_slope} seasons={seasons} P={P}")
  if dtype is np.float32:
    _assert_same_bits(got, run["got"], "draws float32 against the fit's session")
  else:
    assert any((got[k] != run["got"][k]).any() for k in OUTPUTS)


# ---- 2. chunking ------------------------------------------------------------------------------------

@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("has_slope,seasons", MODELS)
def test_the_table_does_not_depend_on_where_the_chunks_are_cut(has_slope, seasons, ragged):
  run = _fit(RAGGED if ragged else BATCH, 3, has_slope, seasons, ragged)
  assert run["chunked"]["num_chunks"] == 3 and run["roomy"]["num_chunks"] == 2
  _assert_same_bits(run["chunked"], run["got"], "one series per chunk")
  _assert_same_bits(run["roomy"], run["got"], "two series per chunk")


def test_one_series_whose_rows_exceed_the_scratch_takes_a_buffer_of_the_call():
  """A session of one series: its 3 x 7 x 4 = 84 rows do not fit the scratch's B * T = 70, so the planes
  lie in the call's own buffer -- the same bits as series 0 of the batch (the same stream and draws)."""
  whole = _fit(BATCH, 3, True, ((7, 1),))
  sess, inp = base._open(list(BATCH), 3, True, ((7, 1),), only=0)             # pylint: disable=protected-access
  try:
    sess.run()
    assert 3 * 7 * 4 > inp["T"]
    got = sess.summarize_placebo_horizons(SCALE, SHIFT, whole["origins"][:1], whole["horizons"][:1])
  finally:
    sess.close()
  for name in OUTPUTS:
    np.testing.assert_array_equal(got[name][0], whole["got"][name][0], err_msg=name)


# ---- 3. against numpy written here -------------------------------------------------------------------

def _reference(inp, draws, b, has_slope, seasons, scale, shift, origins, horizons):
  """The definitions of include/causalimpact_amd.h in numpy for series b, all N draws at once with
  dense d x d matrices, the forecast of every origin stopped at each checkpoint: [3, O, K, N]."""
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

  used = [int(h) for h in horizons if h > 0]
  out = np.zeros((3, len(origins), len(horizons), N))
  for t in range(Tb):
    if t in origins:
      i = origins.index(t)
      fa, fP, r = a, Pm, np.zeros((N, d))
      C, V, A, cnt = np.zeros(N), np.zeros(N), 0.0, 0
      for h in range(used[-1]):
        pz = np.einsum("nij,j->ni", fP, Z)
        if not mask[t + h]:
          C, A, cnt = C + (fa @ Z + reg[:, t + h]), A + y[t + h], cnt + 1
          V = V + 2.0 * (r @ Z) + pz @ Z + s_obs ** 2
          r = r + pz
        if h + 1 in used and cnt:
          k = used.index(h + 1)
          out[0, i, k] = C * scale + cnt * shift
          out[1, i, k] = (V + (A - C) ** 2) * scale * scale
          out[2, i, k] = 0.5 * _erfc(-(A - C) / np.sqrt(2.0 * V))
        if h + 1 < used[-1]:
          fa, fP, r = step(t + h, fa, fP, r)
    pz = np.einsum("nij,j->ni", Pm, Z)
    if not mask[t]:
      F = pz @ Z + s_obs ** 2
      v = y[t] - (a @ Z + reg[:, t])
      a = a + pz * (v / F)[:, None]
      Pm = Pm - np.einsum("ni,nj->nij", pz, pz) / F[:, None, None]
    if t + 1 < Tb:
      a, Pm, _ = step(t, a, Pm)
  return out


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("has_slope,seasons", MODELS)
def test_the_table_equals_numpy_on_the_fetched_draws(has_slope, seasons, ragged):
  run = _fit(RAGGED if ragged else BATCH, 3, has_slope, seasons, ragged)
  inp, got = run["inp"], run["got"]
  worst = dict.fromkeys(OUTPUTS, 0.0)
  for b in range(3):
    used = [int(o) for o in run["origins"][b] if o >= 0]
    ref = _reference(inp, run["draws"], b, has_slope, seasons, run["scale"][b], run["shift"][b], used,
                     [int(h) for h in run["horizons"][b]])
    for j, name in enumerate(OUTPUTS):
      worst[name] = max(worst[name], float(np.abs(got[name][b, :len(used)] - ref[j].mean(axis=-1)).max()))
    print(f"slope={has_slope} seasons={seasons} ragged={ragged} series {b}: largest deviation "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for j, name in enumerate(OUTPUTS):
      np.testing.assert_allclose(got[name][b, :len(used)], ref[j].mean(axis=-1), err_msg=f"series {b} {name}", **TOL)
      assert (got[name][b, len(used):] == 0.0).all()


def test_errors_are_reported_before_any_device_work():
  fn = _native.load().ci_session_summarize_placebo_horizons
  sess, _ = base._open([70, 70], 3, False, ())                   # pylint: disable=protected-access
  one, out = np.ones(2), np.zeros((2, 2, 2))
  good = np.array([[3, 9], [3, -1]], np.int32)
  hz = np.array([[2, 5], [5, -1]], np.int32)

  def raw(scale, origins, horizons, K=2):
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = fn(sess._h, ptr(scale), one.ctypes.data, 2, ptr(origins), K, ptr(horizons), out.ctypes.data, None, None)  # pylint: disable=protected-access
    return rc, _native.load().ci_last_error().decode()

  try:
    with pytest.raises(_native.NativeError, match="needs a finished ci_session_run"):
      sess.summarize_placebo_horizons(1.0, 0.0, good, hz)
    sess.run()
    for args in ((None, good, hz), (one, None, hz), (one, good, None)):
      rc, msg = raw(*args)
      assert rc != 0 and "NULL argument" in msg
    for K in (0, 65):
      rc, msg = raw(one, good, hz, K)
      assert rc != 0 and f"max_horizons must be in [1, 64], got {K}" in msg
    for bad, msg in (([[2, 2], [5, -1]], r"horizons\[0\] must be strictly ascending"),
                     ([[2, 5], [-1, 5]], r"horizons\[1\] must be strictly ascending"),
                     ([[2, 5], [0, -1]], r"horizons\[1, 0\] must be at least 1"),
                     ([[2, 5], [-1, -1]], r"horizons\[1\] holds no horizon")):
      rc, text = raw(one, good, np.array(bad, np.int32))           # the C entry's own checks
      assert rc != 0 and re.search(msg, text), text
      with pytest.raises(ValueError, match=msg):                  # and the binding's, before it
        sess.summarize_placebo_horizons(1.0, 0.0, good, bad)
    # the origins are checked with the row's largest horizon: 9 + 62 > 70, 9 + 61 = 70 is the last admissible
    with pytest.raises(_native.NativeError, match=r"origins\[0, 1\] = 9 with horizon 62 reaches beyond the series' 70 steps"):
      sess.summarize_placebo_horizons(1.0, 0.0, good, [[2, 62], [5, -1]])
    got = sess.summarize_placebo_horizons(1.0, 0.0, good, [[2, 61], [5, -1]])
    assert got["predicted_mean"].shape == (2, 2, 2) and (got["predicted_mean"][1, :, 1] == 0.0).all()
  finally:
    sess.close()
  two, _ = base._open([70], 2, False, ((4, 1), (3, 1)))           # pylint: disable=protected-access
  try:
    with pytest.raises(_native.NativeError, match=r"ci_session_summarize_placebo_horizons takes a trend with at most "
                                                  r"one block of 2 to 7 seasons.*\(4, 3\)"):
      two.summarize_placebo_horizons(1.0, 0.0, [3], [2, 5])
  finally:
    two.close()


# ---- 4. package level: Placebo(horizons=...) ---------------------------------------------------------

ALPHA, SEED, OPTS = base.ALPHA, base.SEED, base.OPTS
PLAIN = base.PLACEBO                                              # Placebo(max_origins=6)
SEVERAL = ci.Placebo(max_origins=6, horizons=(2, 5))
NUMERIC = base.NUMERIC
SHARED = [k for k in lib.PLACEBO_QUALITY_ENTRIES if k != "horizon"]


def _assert_identities(one, what):
  """The slice at H is `placebo`, the last row of the profile is `placebo_quality`, exactly; the index,
  the columns and the empirical_p rule."""
  by_h, prof = one.placebo_by_horizon, one.placebo_profile
  H = int(one.placebo_quality["horizon"])
  assert by_h.index.names == ["origin", "horizon"] and list(by_h.columns) == list(lib.PLACEBO_COLUMNS), what
  assert prof.index.name == "horizon" and list(prof.columns) == list(lib.PLACEBO_PROFILE_COLUMNS), what
  assert list(prof.index) == sorted({h for h in (2, 5) if h <= H} | {H}) and len(one.placebo) >= 3, what
  pd.testing.assert_frame_equal(by_h.xs(H, level="horizon"), one.placebo, check_exact=True)
  pd.testing.assert_series_equal(prof.iloc[-1][SHARED], one.placebo_quality[SHARED], check_names=False, check_exact=True)
  n_post = H if not np.isnan(one.placebo_quality["empirical_p"]) else -1
  assert list(prof["empirical_p"].notna()) == [h == n_post for h in prof.index], what
  assert (prof["n_origins"] > 0).all() and (prof["relative_sd"] > 0).all(), what
  at2 = by_h.xs(2, level="horizon")
  assert at2.index.equals(one.placebo.index) and (at2["n_counted"] <= 2).all() and (at2["predicted_sd"] > 0).any(), what


def _assert_close(got, want, what):
  """Two analyses' by-horizon frames and profiles to the float64 contract."""
  a, b = got.placebo_by_horizon, want.placebo_by_horizon
  assert a.index.equals(b.index), what
  print(what, "largest deviation per column:", (a[NUMERIC] - b[NUMERIC]).abs().max().to_dict())
  np.testing.assert_allclose(a[NUMERIC].to_numpy(np.float64), b[NUMERIC].to_numpy(np.float64), err_msg=what, **TOL)
  assert list(a["horizon_end"]) == list(b["horizon_end"]) and list(a["significant"]) == list(b["significant"]), what
  np.testing.assert_allclose(got.placebo_profile.to_numpy(), want.placebo_profile.to_numpy(), err_msg=what, **TOL)


@functools.lru_cache(maxsize=None)
def _single(b, lengths=(70, 70, 70), own=False, **options):
  frames = base._frames(lengths)                                   # pylint: disable=protected-access
  periods = base._periods(frames[b], b) if own else base._periods(frames[0], 0)   # pylint: disable=protected-access
  return ci.fit_causalimpact(frames[b], *periods, alpha=ALPHA, seed=SEED, placebo=SEVERAL,
                             inference_options=ci.InferenceOptions(**dict(OPTS, **options)))


def test_single_fit_identities_nothing_else_differs_and_the_host_route_agrees():
  one = _single(0)
  _assert_identities(one, "single fit")
  plain, _ = base._single(0)                                       # pylint: disable=protected-access
  assert plain.placebo_by_horizon is None and plain.placebo_profile is None
  pd.testing.assert_frame_equal(one.placebo, plain.placebo, check_exact=True)
  pd.testing.assert_series_equal(one.placebo_quality, plain.placebo_quality, check_exact=True)
  pd.testing.assert_frame_equal(one.series, plain.series, check_exact=True)
  pd.testing.assert_frame_equal(one.summary, plain.summary, check_exact=True)
  host = _single(0, summarize_on_device=False)
  _assert_identities(host, "host route")
  _assert_close(host, one, "summarize_on_device=False against the device")


def test_batch_identities_and_one_profile_table():
  frames = base._frames()                                          # pylint: disable=protected-access
  periods = base._periods(frames[0], 0)                            # pylint: disable=protected-access
  got = ci.fit_causalimpact_batch(frames, *periods, alpha=ALPHA, seed=SEED, shared_streams=True, placebo=SEVERAL,
                                  inference_options=ci.InferenceOptions(**OPTS))
  assert type(got) is ci.CausalImpactBatchAnalysis
  prof = got.placebo_profile
  assert prof.index.names == ["series", "horizon"] and list(prof.columns) == list(lib.PLACEBO_PROFILE_COLUMNS)
  for b in range(3):
    _assert_identities(got[b], f"batch series {b}")
    pd.testing.assert_frame_equal(prof.loc[b], got[b].placebo_profile, check_exact=True)
    one = _single(b)                                               # (shared streams: the same draws)
    _assert_close(got[b], one, f"batch series {b} against its single fit")
  plain = ci.fit_causalimpact_batch(frames, *periods, alpha=ALPHA, seed=SEED, shared_streams=True, placebo=PLAIN,
                                    inference_options=ci.InferenceOptions(**OPTS))
  assert plain.placebo_profile is None and plain[1].placebo_by_horizon is None
  pd.testing.assert_frame_equal(plain.placebo_quality, got.placebo_quality, check_exact=True)
  pd.testing.assert_frame_equal(plain[1].placebo, got[1].placebo, check_exact=True)
  host = ci.fit_causalimpact_batch(frames, *periods, alpha=ALPHA, seed=SEED, shared_streams=True, placebo=SEVERAL,
                                   inference_options=ci.InferenceOptions(summarize_on_device=False, **OPTS))
  for b in range(3):
    _assert_close(host[b], got[b], f"batch series {b}, summarize_on_device=False")


def test_panel_keeps_each_series_own_horizons():
  frames = base._frames(base.PANEL_LENGTHS)                        # pylint: disable=protected-access
  periods = [base._periods(f, b) for b, f in enumerate(frames)]    # pylint: disable=protected-access
  got = ci.fit_causalimpact_panel(frames, periods, alpha=ALPHA, seed=SEED, shared_streams=True, placebo=SEVERAL,
                                  inference_options=ci.InferenceOptions(**OPTS))
  assert type(got) is ci.CausalImpactPanelAnalysis
  prof, own = got.placebo_profile, set()
  for b in range(3):
    _assert_identities(got[b], f"panel series {b}")
    H = int(got.placebo_quality.iloc[b]["horizon"])
    own.add(H)
    mine = got[b].placebo_profile
    pd.testing.assert_frame_equal(prof.loc[b].loc[mine.index], mine, check_exact=True)
    others = [h for h in prof.loc[b].index if h not in mine.index]
    assert prof.loc[b].loc[others].isna().all().all()             # NaN rows for the horizons it lacks
    _assert_close(got[b], _single(b, base.PANEL_LENGTHS, own=True), f"panel series {b} against its single fit")
  assert len(own) > 1 and list(prof.loc[0].index) == sorted({2, 5} | own)


def test_two_seasonal_blocks_take_one_call_per_horizon(monkeypatch):
  """Seasons(7) + Seasons(4, num_steps_per_season=7): 1 + 6 + 3 = 10 state components, a block-list model --
  K calls of `summarize_placebo_blocks` with the same origins, and the new entry is not reached."""
  calls = []
  blocks_entry = _native.Session.summarize_placebo_blocks
  def counting(self, scale, shift, origins, horizon, want=None):
    calls.append(np.asarray(horizon).tolist())
    return blocks_entry(self, scale, shift, origins, horizon, want)
  def never(*a, **k):
    raise AssertionError("the one-lane entry was reached")
  monkeypatch.setattr(_native.Session, "summarize_placebo_blocks", counting)
  monkeypatch.setattr(_native.Session, "summarize_placebo_horizons", never)
  frames = base._frames()                                          # pylint: disable=protected-access
  periods = base._periods(frames[0], 0)                            # pylint: disable=protected-access
  kw = dict(alpha=ALPHA, seed=SEED, placebo=SEVERAL,
            model_options=ci.ModelOptions(seasons=[ci.Seasons(7), ci.Seasons(4, num_steps_per_season=7)]))
  one = ci.fit_causalimpact(frames[0], *periods, inference_options=ci.InferenceOptions(**OPTS), **kw)
  _assert_identities(one, "two blocks")
  H = int(one.placebo_quality["horizon"])
  assert calls == [[2], [5], [H]]
  host = ci.fit_causalimpact(frames[0], *periods, inference_options=ci.InferenceOptions(summarize_on_device=False, **OPTS), **kw)
  _assert_close(host, one, "two blocks, summarize_on_device=False")


@pytest.mark.parametrize("route", ["float64", "hmc"])
def test_draws_pooled_on_the_host_go_through_a_draws_session(route, monkeypatch):
  calls = []
  entry = _native.Session.summarize_placebo_horizons
  def counting(self, *a, **k):
    calls.append(type(self).__name__)
    return entry(self, *a, **k)
  monkeypatch.setattr(_native.Session, "summarize_placebo_horizons", counting)
  frames = base._frames()                                          # pylint: disable=protected-access
  periods = base._periods(frames[0], 0)                            # pylint: disable=protected-access
  kw = dict(alpha=ALPHA, seed=SEED, placebo=SEVERAL)
  if route == "hmc":
    opts = dict(sampler="hmc", num_chains=2, num_results=20, num_warmup_steps=20)
  else:
    opts, kw["data_options"] = dict(OPTS), ci.DataOptions(dtype=np.float64)
  one = ci.fit_causalimpact(frames[0], *periods, inference_options=ci.InferenceOptions(**opts), **kw)
  assert calls == ["DrawsSession"]
  _assert_identities(one, route)
  host = ci.fit_causalimpact(frames[0], *periods, inference_options=ci.InferenceOptions(summarize_on_device=False, **opts), **kw)
  assert calls == ["DrawsSession"]                                 # (the numpy twin: no session)
  _assert_close(host, one, f"{route}, summarize_on_device=False")


# ---- 5. off by default ---------------------------------------------------------------------------------

@pytest.mark.parametrize("placebo", [True, ci.Placebo(), ci.Placebo(max_origins=6)])
def test_without_horizons_the_new_entry_is_never_called(placebo, monkeypatch):
  def never(*a, **k):
    raise AssertionError("summarize_placebo_horizons was reached")
  monkeypatch.setattr(_native.Session, "summarize_placebo_horizons", never)
  monkeypatch.setattr(_native.DrawsSession, "summarize_placebo_horizons", never, raising=False)
  frames = base._frames()                                          # pylint: disable=protected-access
  periods = base._periods(frames[0], 0)                            # pylint: disable=protected-access
  kw = dict(alpha=ALPHA, seed=SEED, placebo=placebo, inference_options=ci.InferenceOptions(**OPTS))
  one = ci.fit_causalimpact(frames[0], *periods, **kw)
  assert one.placebo is not None and one.placebo_by_horizon is None and one.placebo_profile is None
  got = ci.fit_causalimpact_batch(frames, *periods, shared_streams=True, **kw)
  assert got.placebo_quality is not None and got.placebo_profile is None and got[0].placebo_profile is None
  with pytest.raises(AssertionError, match="summarize_placebo_horizons was reached"):
    ci.fit_causalimpact(frames[0], *periods, **dict(kw, placebo=SEVERAL))
