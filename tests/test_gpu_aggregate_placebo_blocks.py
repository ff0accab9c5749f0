"""ci_session_pool_placebo_blocks on the device -- the placebo forecasts of POOLED sums for any block
list with a state of at most 64 components: the entry table of ci_session_pool_placebo on the filter of
ci_session_summarize_placebo_blocks, one filter pass per chunk of entries for both pooled terms -- at
session level against numpy (`_placebo_summary_host(per_draw=True)` on the draws fetched from the same
session, `placebo_terms_host`, `pool_placebo_host`, `finish_placebo_host`), bit for bit against the
one-lane entry where both take the model, against the per-series call, across chunk sizes and sessions,
and at package level (`placebo=` with `aggregates=` / `event_aggregates=`) with the numpy filter barred.

The shapes of tests/test_gpu_block_predictions.py: four series, T = 90 (150 for the two wide models),
2 chains x 12 kept draws give N = 24, one case runs N = 70; the steps 11, 12 and 40 are missing and the
post-period (from 0.7 T on) is masked.  An origin row holds five origins -- one right behind the state
dimension, one on the missing step 40, one at T - H -- and two unused slots; H is 1 and 5.  The four
groups of tests/test_gpu_aggregate_placebo.py give 8 entries for 4 series: two chunks, the group of all
four cut by the boundary.  Every comparison with numpy is to rtol 1e-8, atol 1e-8, the project's float64
contract."""
import functools

import numpy as np
import pytest

import causalimpact as ci
from causalimpact import _model
from causalimpact import _native
from causalimpact import causalimpact_lib as lib
from causalimpact import data as cid

import test_gpu_aggregate_placebo as pooled
import test_gpu_block_predictions as blocks
import test_gpu_placebo as base

pytestmark = pytest.mark.gpu

TOL = blocks.TOL
OUTPUTS = blocks.PLAC
GROUPS, SCALES, SHIFTS = pooled.GROUPS, np.array(pooled.SCALES), np.array(pooled.SHIFTS)
MODELS = dict(blocks.MODELS, **{"24 d=24": (False, ((24, 1),), 90)})        # a 32-lane group: MODELS has none
NAMES = ["4x3+3 d=6", "7+4+6 slope d=16", "24 d=24", "34 slope d=35", "63 slope d=64"]
B, SLOTS = 4, 7


def _plan(T, has_slope, seasons, H, num_series=B):
  """origins [B, 7]: right behind the state dimension, a neighbour, the missing step 40, one late in
  the pre-period, T - H (its window lies in the masked post-period: nothing counted), two unused."""
  first = max(blocks._state_dim(has_slope, seasons) + 2, 13)                  # pylint: disable=protected-access
  pre = int(0.7 * T)
  rows = []
  for b in range(num_series):
    row = sorted({first, first + 4 + b, 40, pre - 7 - b, T - H})
    assert len(row) == 5
    rows.append(row + [-1, -1])
  return np.asarray(rows, np.int32)


def _entry_terms(inp, draws, b, has_slope, scale, shift, origins, H):
  """(s, v [O, N], seen_sum [O]) of one entry: series b of the session from `origins` with horizon H."""
  pool = lambda a: a[b].reshape((a.shape[1] * a.shape[2],) + a.shape[3:]).astype(np.float64)
  got = lib._placebo_summary_host(                                            # pylint: disable=protected-access
      inp["y"][b], inp["mask"][b], inp["X"][b], inp["sc"], inp["num_seasons"], has_slope, inp["specs"][b],
      {k: pool(draws[k]) for k in blocks.PARAM_FIELDS}, scale, shift, origins, H, per_draw=True)
  s, v = _native.placebo_terms_host(got["C"], got["V"], got["cnt"], scale, shift)
  _, seen = lib._placebo_seen(inp["y"][b], inp["mask"][b], origins, H, scale, shift)   # pylint: disable=protected-access
  return s, v, np.nan_to_num(seen)


def _reference(inp, draws, has_slope, scales, shifts, csr, origins, H):
  """(acc [G, O, 2, N], seen [G, O], means) in numpy; origins [B, O]: every entry takes its series' row."""
  offsets, members, weights = csr
  G = offsets.size - 1
  own = {b: _entry_terms(inp, draws, b, has_slope, scales[b], shifts[b], origins[b], H) for b in sorted(set(members))}
  terms = [own[int(b)] for b in members]
  acc = _native.pool_placebo_host(np.stack([t[0] for t in terms]), np.stack([t[1] for t in terms]), csr)
  seen = np.zeros((G, origins.shape[1]))
  for g in range(G):
    for k in range(offsets[g], offsets[g + 1]):
      seen[g] = seen[g] + weights[k] * terms[k][2]
  return acc, seen, _native.finish_placebo_host(acc, seen)


@functools.lru_cache(maxsize=None)
def _run(name, H, S=12):
  """One session of four series of a model: the numpy reference on its draws, the per-series call
  before and after, the pooled call with and without `seen` and with the chunk sizes 1, 3 and B."""
  has_slope, seasons, T = MODELS[name]
  sess, inp = blocks._open(B, T, has_slope, seasons, S=S)                      # pylint: disable=protected-access
  origins = _plan(T, has_slope, seasons, H)
  try:
    sess.run()
    draws = sess.fetch(blocks.PARAM_FIELDS)
    csr = _native.groups_csr(GROUPS, B)
    acc, seen, means = _reference(inp, draws, has_slope, SCALES, SHIFTS, csr, origins, H)
    before = sess.summarize_placebo_blocks(SCALES, SHIFTS, origins, H)
    got = sess.pool_placebo_blocks(SCALES, SHIFTS, GROUPS, origins, H, seen=seen)
    bare = sess.pool_placebo_blocks(SCALES, SHIFTS, GROUPS, origins, H)
    cut = {c: sess.pool_placebo_blocks(SCALES, SHIFTS, GROUPS, origins, H, seen=seen, chunk_entries=c) for c in (1, 3, B)}
    after = sess.summarize_placebo_blocks(SCALES, SHIFTS, origins, H)
    return dict(got=got, bare=bare, cut=cut, acc=acc, seen=seen, means=means, before=before, after=after, inp=inp,
                origins=origins, kernel=sess.kernel_name())
  finally:
    sess.close()


# ---- 1. numpy ----------------------------------------------------------------------------------------

def _check_against_numpy(name, H, S=12):
  r = _run(name, H, S)
  got, N = r["got"], 2 * S
  assert got["acc"].shape == (len(GROUPS), SLOTS, 2, N) and got["pit_mean"].shape == (len(GROUPS), SLOTS)
  pooled._compare(got, r["acc"], r["means"], f"{name} [{r['kernel']}] H={H} N={N}")   # pylint: disable=protected-access
  assert sorted(r["bare"]) == ["acc"]
  np.testing.assert_array_equal(r["bare"]["acc"], got["acc"])
  # slots that read zero: the unused ones, and the windows that count nothing
  assert (got["acc"][:, 5:] == 0.0).all() and all((got[k][:, 5:] == 0.0).all() for k in OUTPUTS)
  mask = r["inp"]["mask"]
  per_series = np.array([[(~mask[b, o:o + H]).sum() for o in r["origins"][b][:5]] for b in range(B)])
  counted = np.array([per_series[sorted(g)].sum(axis=0) for g in GROUPS])       # member-steps, [G, 5]
  assert ((got["acc"][:, :5, 1] == 0.0).all(axis=2) == (counted == 0)).all()
  assert ((got["acc"][:, :5, 1] > 0.0).all(axis=2) == (counted > 0)).all()
  for k in OUTPUTS:
    assert ((got[k][:, :5] == 0.0) == (counted == 0)).all()
  assert (counted[:, 4] == 0).all() and (counted > 0).any()                     # (T - H: the masked post-period)
  if H == 1:
    at40 = [list(r["origins"][b]).index(40) for b in range(B)]
    assert len(set(at40)) == 1 and (counted[:, at40[0]] == 0).all() and (got["acc"][:, at40[0]] == 0.0).all()
  pit = got["pit_mean"][:, :5][counted > 0]
  assert ((pit > 0.0) & (pit < 1.0)).all()


@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("name", NAMES)
def test_pooled_sums_and_means_equal_numpy_on_the_fetched_draws(name, H):
  _check_against_numpy(name, H)


def test_seventy_draws_fill_wavefronts_with_a_remainder():
  """N = 70 over groups of 16 lanes: seventeen wavefronts of 4 filters and one of 2."""
  _check_against_numpy("7+4+6 slope d=16", 5, S=35)


# ---- 2. the one-lane entry -----------------------------------------------------------------------------

@pytest.mark.parametrize("has_slope,seasons", [(False, ()), (True, ()), (True, ((7, 1),)), (False, ((2, 1),))])
def test_models_both_families_take_pool_the_same_bits_as_the_one_lane_entry(has_slope, seasons):
  sess, _ = blocks._open(B, 90, has_slope, seasons)                            # pylint: disable=protected-access
  try:
    sess.run()
    for H in (1, 5):
      origins = _plan(90, has_slope, seasons, H)
      seen = 50.0 + np.arange(len(GROUPS) * SLOTS, dtype=np.float64).reshape(len(GROUPS), SLOTS)
      old = sess.pool_placebo(SCALES, SHIFTS, GROUPS, origins, H, seen=seen)
      new = sess.pool_placebo_blocks(SCALES, SHIFTS, GROUPS, origins, H, seen=seen)
      gap = {k: float((np.abs(new[k] - old[k]) / np.maximum(np.abs(old[k]), 1e-300)).max()) for k in old}
      print(f"slope={has_slope} seasons={seasons} H={H}: largest relative gap to the one-lane entry {gap}")
      assert (old["acc"][:, :4, 1] > 0.0).any()
      np.testing.assert_array_equal(new["acc"], old["acc"])
      for k in OUTPUTS:
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)
  finally:
    sess.close()


# ---- 3. one pass equals two ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["4x3+3 d=6", "34 slope d=35"])
def test_a_group_of_one_member_is_the_per_series_call(name):
  """Group 0 is {0: 1.0}: its S and U planes come out of the single pass.  The row means of S are
  `summarize_placebo_blocks`'s predicted_mean of series 0 bit for bit (SUM, then comp_row_stats in
  both); the row means of U agree with spread_mean - e^2 of the per-series call to the float64
  contract (e is formed on the data scale here, in the sampler's units there)."""
  r = _run(name, 5)
  np.testing.assert_array_equal(r["got"]["predicted_mean"][0], r["before"]["predicted_mean"][0])
  S, U = r["got"]["acc"][0, :, 0], r["got"]["acc"][0, :, 1]
  e2 = np.where(U != 0.0, (r["seen"][0][:, None] - S) ** 2, 0.0).mean(axis=1)
  want = r["before"]["spread_mean"][0] - e2
  print(f"{name}: largest deviation of the U plane's row means", float(np.abs(U.mean(axis=1) - want).max()))
  np.testing.assert_allclose(U.mean(axis=1), want, **TOL)
  assert (U.mean(axis=1)[:4] > 0.0).all()
  np.testing.assert_allclose(r["got"]["spread_mean"][0], r["before"]["spread_mean"][0], **TOL)
  np.testing.assert_allclose(r["got"]["pit_mean"][0], r["before"]["pit_mean"][0], **TOL)


# ---- 4. cutting ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["7+4+6 slope d=16", "63 slope d=64"])
def test_the_result_does_not_depend_on_where_the_entries_are_cut(name):
  r = _run(name, 5)
  for c, cut in r["cut"].items():
    for k, v in r["got"].items():
      np.testing.assert_array_equal(cut[k], v, err_msg=f"chunk_entries={c} {k}")


def test_a_batch_cut_into_sessions_continues_the_sum_bit_for_bit():
  """Three series in one session, and as single-series sessions (matching stream keys) chained
  through `init`: the same bits; and once more with `init` and `out` the same buffer."""
  has_slope, seasons, T = MODELS["7+4+6 slope d=16"]
  H = 5
  groups = ({0: 1.0, 1: 0.5, 2: 2.0}, {1: 1.0, 2: -1.0})
  origins = _plan(T, has_slope, seasons, H, 3)
  scales, shifts = SCALES[:3].copy(), SHIFTS[:3].copy()
  sess, _ = blocks._open(3, T, has_slope, seasons)                             # pylint: disable=protected-access
  try:
    sess.run()
    whole = sess.pool_placebo_blocks(scales, shifts, groups, origins, H)["acc"]
    again = sess.pool_placebo_blocks(scales, shifts, groups, origins, H, init=whole)["acc"]
    buf = whole.copy()
    csr = _native.groups_csr(groups, 3)
    org = np.ascontiguousarray(origins[csr[1]], dtype=np.int32)
    hz = np.array([H, H], np.int32)
    rc = _native.load().ci_session_pool_placebo_blocks(
        sess._h, scales.ctypes.data, shifts.ctypes.data, 2, csr[0].ctypes.data, csr[1].ctypes.data,  # pylint: disable=protected-access
        csr[2].ctypes.data, SLOTS, org.ctypes.data, hz.ctypes.data, buf.ctypes.data, buf.ctypes.data, None, None, None, None)
    assert rc == 0
    np.testing.assert_array_equal(buf, again)
    assert not np.array_equal(again, whole)
  finally:
    sess.close()
  acc = None
  for b in range(3):
    one, _ = blocks._open(3, T, has_slope, seasons, only=b)                    # pylint: disable=protected-access
    try:
      one.run()
      own = [{0: g[b]} if b in g else {} for g in groups]
      acc = one.pool_placebo_blocks(scales[b], shifts[b], own, origins[b:b + 1], H, init=acc)["acc"]
    finally:
      one.close()
  np.testing.assert_array_equal(acc, whole)


# ---- 5. the per-series call is undisturbed ---------------------------------------------------------------

@pytest.mark.parametrize("name", ["4x3+3 d=6", "63 slope d=64"])
def test_the_per_series_call_returns_the_same_before_and_after(name):
  r = _run(name, 5)
  for k in OUTPUTS:
    np.testing.assert_array_equal(r["before"][k], r["after"][k])


# ---- 6. errors before any device work --------------------------------------------------------------------

def test_errors_are_reported_before_any_device_work():
  L = _native.load()
  sess, _ = blocks._open(2, 90, True, ((4, 1), (3, 1)))                        # pylint: disable=protected-access
  good = np.array([[13, 19], [13, -1]], np.int32)
  groups = ({0: 1.0, 1: 2.0}, {1: 1.0})
  try:
    with pytest.raises(_native.NativeError, match="ci_session_pool_placebo_blocks needs a finished ci_session_run"):
      sess.pool_placebo_blocks(1.0, 0.0, groups, good, 5)
    sess.run()
    with pytest.raises(_native.NativeError, match=r"group 1: the horizon must be at least 1, got 0"):
      sess.pool_placebo_blocks(1.0, 0.0, groups, good, [5, 0])
    for bad in ([[19, 13], [13, -1]], [[13, 13], [13, -1]]):                    # descending, repeated
      with pytest.raises(_native.NativeError, match=r"group 0, entry 0 \(member 0\): the origins must be strictly "
                                                    r"ascending .* \(slot 1 holds 13\)"):
        sess.pool_placebo_blocks(1.0, 0.0, groups, bad, 5)
    with pytest.raises(_native.NativeError, match=r"group 0, entry 1 \(member 1\): slot 0 must hold a step or -1"):
      sess.pool_placebo_blocks(1.0, 0.0, groups, [[13, 19], [-2, -1]], 5)
    with pytest.raises(_native.NativeError, match=r"group 0, entry 0 \(member 0\): the origin 86 of slot 1 with horizon 5 "
                                                  r"reaches beyond the series' 90 steps"):
      sess.pool_placebo_blocks(1.0, 0.0, groups, [[13, 86], [13, -1]], 5)
    for c in (0, 3):
      with pytest.raises(_native.NativeError, match=rf"chunk_entries must be in \[1, 2\] \(the session's series\), got {c}"):
        sess.pool_placebo_blocks(1.0, 0.0, groups, good, 5, chunk_entries=c)
    # the means without `seen`, through the raw call
    one, off = np.ones(2), np.array([0, 2], np.int32)
    members, weights = np.array([0, 1], np.int32), np.ones(2)
    org, hz = np.array([[13, 19], [13, 19]], np.int32), np.array([5], np.int32)
    out, means = np.zeros((1, 2, 2, 24)), np.zeros((1, 2))
    ptr = lambda a: None if a is None else a.ctypes.data

    def raw(seen=None, mean=None, origins=org):
      rc = L.ci_session_pool_placebo_blocks(
          sess._h, one.ctypes.data, one.ctypes.data, 1, off.ctypes.data, members.ctypes.data,  # pylint: disable=protected-access
          weights.ctypes.data, 2, ptr(origins), hz.ctypes.data, None, out.ctypes.data, ptr(seen), None, None, ptr(mean))
      return rc, L.ci_last_error().decode()

    rc, msg = raw(mean=means)
    assert rc != 0 and "need `seen`" in msg
    rc, msg = raw(origins=None)
    assert rc != 0 and "NULL argument" in msg
    rc, msg = raw(seen=means, mean=means)
    assert rc == 0, msg
    got = sess.pool_placebo_blocks(1.0, 0.0, groups, [[13, 85], [13, -1]], 5)["acc"]   # 85 + 5 = 90: the last admissible
    assert got.shape == (2, 2, 2, 24) and (got[1, 1] == 0.0).all() and (got[:, 0, 1] > 0.0).all()
    assert (got[0, 1] == 0.0).all()                     # (its window lies in the masked post-period: nothing counted)
  finally:
    sess.close()
  big, _ = blocks._open(1, 150, True, ((64, 1),))                               # d = 65  pylint: disable=protected-access
  try:
    with pytest.raises(_native.NativeError, match=r"ci_session_pool_placebo_blocks takes a state of at most 64 "
                                                  r"components, this session has 65 with the blocks \(64\)"):
      big.pool_placebo_blocks(1.0, 0.0, [{0: 1.0}], [[70]], 5)
  finally:
    big.close()
  pb = _native.make_problem(T=90, P=3, has_slope=0, num_warmup=3, num_results=12, num_chains=2, num_series=2, seed=(5, 9))
  series = [blocks._series(T, 3, 61 + T, False, ()) for T in (90, 70)]           # pylint: disable=protected-access
  pad = lambda a, fill: np.concatenate([a, np.full((90 - a.shape[0],) + a.shape[1:], fill, a.dtype)])
  rag = _native.Session.ragged(pb, [90, 70], np.stack([pad(s[0], np.nan) for s in series]),
                               np.stack([pad(s[1], True) for s in series]), np.stack([pad(s[2], 7.5) for s in series]),
                               _native.make_params([s[3] for s in series]))
  try:
    rag.run()
    with pytest.raises(_native.NativeError, match=r"ci_session_pool_placebo_blocks takes no ragged session.*"
                                                  r"ci_session_pool_placebo$"):
      rag.pool_placebo_blocks(1.0, 0.0, [{0: 1.0, 1: 1.0}], [[13], [13]], 5)
    assert rag.pool_placebo(1.0, 0.0, [{0: 1.0, 1: 1.0}], [[13], [13]], 5)["acc"].shape == (1, 1, 2, 24)
  finally:
    rag.close()


# ---- 7., 8. package level: placebo= with aggregates= / event_aggregates= -----------------------------------

ALPHA, SEED, OPTS = pooled.ALPHA, pooled.SEED, pooled.OPTS
PLACEBO = ci.Placebo(max_origins=5)
AGGREGATES = pooled.AGGREGATES
TWO = [ci.Seasons(4), ci.Seasons(3)]
_ENTRY_HOST = lib._placebo_entry_host                                          # pylint: disable=protected-access


def _barred(*args, **kwargs):
  raise AssertionError("the launch filtered a pooled placebo entry in numpy")


def _member_entry(b, frame, periods, origins, H):
  """`lib._placebo_entry_host` of series b from its OWN fit of the two-block model (the single fit on
  the key of series b draws what the batch draws for it), for the origins and the horizon of a group."""
  one = ci.fit_causalimpact(frame, *periods, alpha=ALPHA, seed=_native.series_stream_key((0, SEED), b),
                            model_options=ci.ModelOptions(seasons=TWO), inference_options=ci.InferenceOptions(**OPTS))
  data = cid.CausalImpactData(frame, *periods, dtype=np.float32)
  n_after = data.model_after_pre_data.shape[0]
  y = np.concatenate([np.asarray(data.outcome_ts.time_series, np.float64), np.full(n_after, np.nan)])
  mask = np.concatenate([np.asarray(data.outcome_ts.is_missing, bool), np.ones(n_after, bool)])
  design = np.asarray(data.feature_ts.values, np.float64)
  params = _model.series_params(y, mask, design, num_seasonal_blocks=len(TWO),
                                outcome_sd=float(np.nanstd(y[:y.shape[0] - n_after], ddof=1)))
  num_seasons, sc = _model.expand_seasons(TWO, y.shape[0])
  ps = one.posterior_samples
  N = np.asarray(ps.level_scale).shape[0]
  draws = dict(observation_noise_scale=np.asarray(ps.observation_noise_scale), level_scale=np.asarray(ps.level_scale),
               slope_scale=np.zeros(N), seasonal_drift_scales=np.asarray(ps.seasonal_drift_scales),
               weights=np.asarray(ps.weights))
  rq = lib._device_summary_request(data, ALPHA)                               # pylint: disable=protected-access
  inputs = lib.SeriesInputs(y, mask, design, sc, num_seasons, False, params)
  return _ENTRY_HOST(inputs, draws, rq["scale"], rq["shift"], rq["observed"], origins, H)


def test_batch_pooled_placebo_of_a_two_block_model_is_filtered_on_the_device(monkeypatch):
  """On the parent the launch pools such a model in numpy (`lib._placebo_entry_host`): barred here."""
  from causalimpact import batch                                               # pylint: disable=import-outside-toplevel
  frames = base._frames()                                                      # pylint: disable=protected-access
  periods = base._periods(frames[0], 0)                                        # pylint: disable=protected-access
  kw = dict(alpha=ALPHA, seed=SEED, model_options=ci.ModelOptions(seasons=TWO),
            inference_options=ci.InferenceOptions(**OPTS))
  with monkeypatch.context() as m:
    m.setattr(lib, "_placebo_entry_host", _barred)
    got = ci.fit_causalimpact_batch(frames, *periods, aggregates=AGGREGATES, placebo=PLACEBO, **kw)
  assert type(got) is ci.CausalImpactBatchAnalysis             # (the one-launch route)
  names, csr = batch.aggregate_groups(AGGREGATES, range(3))
  prep = got._prep                                                             # pylint: disable=protected-access
  n_post = int(np.count_nonzero(prep.flags & 2))
  H, origins = lib.placebo_plan(PLACEBO, prep.num_pre, n_post, 1)
  pp = batch.batch_placebo_pool_plan(csr, origins, H, n_post, prep.index[prep.model_rows])
  assert len(origins) == 5 and got.aggregates["all"].placebo.index.equals(got[0].placebo.index)
  monkeypatch.setattr(pooled, "_member_entry", _member_entry)
  pooled._assert_pooled(got, pooled._host_aggregate_frames(got, pp, names, frames, [periods] * 3), names,   # pylint: disable=protected-access
                        "two-block batch")
  pooled._assert_rest_unchanged(got, ci.fit_causalimpact_batch(frames, *periods, aggregates=AGGREGATES, **kw),   # pylint: disable=protected-access
                                ci.fit_causalimpact_batch(frames, *periods, placebo=PLACEBO, **kw), names)


def test_panel_pooled_placebo_of_a_two_block_model_is_filtered_on_the_device(monkeypatch):
  """Two lengths: one ordinary session per length, each through the block-model entry."""
  from causalimpact import batch                                               # pylint: disable=import-outside-toplevel
  frames = base._frames((70, 64))                                              # pylint: disable=protected-access
  periods = [base._periods(f, b) for b, f in enumerate(frames)]               # pylint: disable=protected-access
  aggregates = {"all": "all", "pair": {0: 1.0, 1: 0.5}}
  kw = dict(alpha=ALPHA, seed=SEED, model_options=ci.ModelOptions(seasons=TWO),
            inference_options=ci.InferenceOptions(**OPTS))
  with monkeypatch.context() as m:
    m.setattr(lib, "_placebo_entry_host", _barred)
    got = ci.fit_causalimpact_panel(frames, periods, event_aggregates=aggregates, placebo=PLACEBO, **kw)
  assert type(got) is ci.CausalImpactPanelAnalysis
  names, csr = batch.aggregate_groups(aggregates, range(2))
  prep = got._prep                                                             # pylint: disable=protected-access
  pp = batch.event_placebo_pool_plan(PLACEBO, batch.event_plan(names, csr, prep, "y"), 1)
  assert (pp.columns >= 0).any(axis=1).all()
  monkeypatch.setattr(pooled, "_member_entry", _member_entry)
  pooled._assert_pooled(got, pooled._host_aggregate_frames(got, pp, names, frames, periods), names,   # pylint: disable=protected-access
                        "two-block panel")
