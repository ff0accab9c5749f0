"""ci_session_pool_placebo_horizons[_blocks] on the device: the pooled placebo forecasts of every group
at several horizons from one filter pass -- bit for bit what K calls of ci_session_pool_placebo[_blocks]
return on the same session (the entry this one was built next to, not the code under test), whatever the
chunking, the session's kind and the cut of a batch into sessions, and against numpy written from the
fetched draws (`_placebo_summary_host(per_draw=True)` per horizon, `pool_placebo_host`,
`finish_placebo_host`); then `Placebo(horizons=...)` with `aggregates=` / `event_aggregates=` at package
level.

The shapes of tests/test_gpu_aggregate_placebo.py and tests/test_gpu_placebo_horizons.py: four series,
T = 70 (133 with a block of 7 seasons), 2 chains x 37 draws (N = 74: a full wavefront and a remainder),
the steps 11, 12 and 40 missing; origins [3, 4, 11, 35, T_b - 9, -1, -1]; the four GROUPS of the former
(8 entries); horizons [1, 2, 9, -1], the last group on a row of its own, [2, 5, -1, -1].  h = 1 and 2 from
origin 11 count nothing: those rows are 0, their neighbours are not.  Every comparison with numpy is to
rtol 1e-8, atol 1e-8, the project's float64 contract."""
import functools

import numpy as np
import pytest

from causalimpact import _model
from causalimpact import _native
from causalimpact import causalimpact_lib as lib

import test_gpu_aggregate_placebo as pooled
import test_gpu_aggregate_placebo_blocks as pooled_blocks
import test_gpu_block_predictions as blocks
import test_gpu_placebo as base

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-8, atol=1e-8)
OUTPUTS = _native.PLACEBO_OUTPUTS
GROUPS = pooled.GROUPS
SCALES, SHIFTS = np.array(pooled.SCALES), np.array(pooled.SHIFTS)
HORIZONS, OWN_ROW, HMAX = [1, 2, 9, -1], [2, 5, -1, -1], 9
# no slope and no block, slope alone, slope + 7 seasons, no slope + 2 seasons
MODELS = [(False, ()), (True, ()), (True, ((7, 1),)), (False, ((2, 1),))]
RAGGED = (70, 47, 64, 70)
G, SLOTS, K, N = len(GROUPS), 7, 4, 74


def _lengths(seasons):
  return (133,) * 4 if seasons == ((7, 1),) else (70,) * 4


def _table(last=OWN_ROW, row=None):
  """horizons [G, K]: the last group has a row of its own."""
  hz = np.array([HORIZONS if row is None else row] * G, np.int32)
  hz[G - 1] = last
  return hz


def _origins(lengths, hmax=HMAX):
  return np.array([base._origins(Tb, hmax) for Tb in lengths], np.int32)      # pylint: disable=protected-access


def _k_calls(sess, origins, hz, init=None, seen=None, entry="pool_placebo", groups=GROUPS, scales=SCALES, shifts=SHIFTS):
  """The result from K calls of `pool_placebo` (`pool_placebo_blocks`) on the same session: column k of
  the groups whose slot k is used (the others get a valid horizon and are not read); an unused slot
  keeps `init` and has means of 0."""
  n_groups, width = hz.shape
  O, n = origins.shape[1], sess.pb.num_chains * sess.pb.num_results
  acc = np.zeros((n_groups, O, width, 2, n)) if init is None else np.array(init, np.float64)
  out = {"acc": acc}
  if seen is not None:
    out.update({name: np.zeros((n_groups, O, width)) for name in OUTPUTS})
  for k in range(width):
    used = hz[:, k] > 0
    if not used.any():
      continue
    got = getattr(sess, entry)(scales, shifts, groups, origins, np.where(used, hz[:, k], 1),
                               init=None if init is None else np.ascontiguousarray(init[:, :, k]),
                               seen=None if seen is None else np.ascontiguousarray(seen[:, :, k]))
    acc[used, :, k] = got["acc"][used]
    for name in OUTPUTS if seen is not None else ():
      out[name][used, :, k] = got[name][used]
  return out


def _assert_same_bits(got, want, what):
  for name in want:
    assert got[name].shape == want[name].shape and got[name].dtype == np.float64, f"{what} {name}"
    np.testing.assert_array_equal(got[name], want[name], err_msg=f"{what} {name}")


def _numpy(series_terms, seen_of, csr, origins, hz, draws=N):
  """(acc [G, O, K, 2, N], seen [G, O, K], means) in numpy.  series_terms(b, h) -> (s, v [O, N]) of series
  b at horizon h from origins[b]; seen_of(b, row) -> seen_sum [O, K] of series b for a horizon row."""
  offsets, members, weights = csr
  n_groups, width = hz.shape
  E, O = int(offsets[-1]), origins.shape[1]
  sums, variances = np.zeros((E, O, width, draws)), np.zeros((E, O, width, draws))
  seen = np.zeros((n_groups, O, width))
  for g in range(n_groups):
    for e in range(offsets[g], offsets[g + 1]):
      b = int(members[e])
      for k, h in enumerate(int(h) for h in hz[g]):
        if h > 0:
          sums[e, :, k], variances[e, :, k] = series_terms(b, h)
      seen[g] = seen[g] + weights[e] * np.nan_to_num(seen_of(b, hz[g]))
  acc = _native.pool_placebo_horizons_host(sums, variances, csr)
  return acc, seen, _native.finish_placebo_horizons_host(acc, seen)


def _compare(got, acc, means, what):
  worst = {"acc": float(np.abs(got["acc"] - acc).max()), **{k: float(np.abs(got[k] - means[k]).max()) for k in OUTPUTS}}
  print(f"{what}: largest deviation from numpy " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
  np.testing.assert_allclose(got["acc"], acc, err_msg=f"{what} acc", **TOL)
  for k in OUTPUTS:
    np.testing.assert_allclose(got[k], means[k], err_msg=f"{what} {k}", **TOL)


@functools.lru_cache(maxsize=None)
def _run(lengths, P, has_slope, seasons, ragged=False):
  """One finished session of four series: the numpy reference on its draws, the K single-horizon calls,
  the one-pass call with and without `seen` and with chunks of 1 and 3 entries, and the per-series
  entries before and after."""
  sess, inp = base._open(list(lengths), P, has_slope, seasons, ragged)        # pylint: disable=protected-access
  try:
    sess.run()
    draws = sess.fetch(base.PARAM_FIELDS)
    origins, hz = _origins(inp["lengths"]), _table()
    csr = _native.groups_csr(GROUPS, 4)

    @functools.lru_cache(maxsize=None)
    def series_terms(b, h):
      s, v, _, _ = pooled._entry_terms(inp, draws, b, has_slope, seasons, SCALES[b], SHIFTS[b], origins[b], h)   # pylint: disable=protected-access
      return s, v

    def seen_of(b, row):
      Tb = inp["lengths"][b]
      return lib._placebo_seen(inp["y"][b, :Tb], inp["mask"][b, :Tb], origins[b], HMAX, SCALES[b], SHIFTS[b],   # pylint: disable=protected-access
                               horizons=row)[1]

    acc, seen, means = _numpy(series_terms, seen_of, csr, origins, hz)
    per_series = np.array([HORIZONS] * 4, np.int32)
    before = (sess.summarize_placebo(SCALES, SHIFTS, origins, HMAX),
              sess.summarize_placebo_horizons(SCALES, SHIFTS, origins, per_series))
    want = _k_calls(sess, origins, hz, seen=seen)
    got = sess.pool_placebo_horizons(SCALES, SHIFTS, GROUPS, origins, hz, seen=seen)
    bare = sess.pool_placebo_horizons(SCALES, SHIFTS, GROUPS, origins, hz)
    cut = {c: sess.pool_placebo_horizons(SCALES, SHIFTS, GROUPS, origins, hz, seen=seen, chunk_entries=c) for c in (1, 3)}
    after = (sess.summarize_placebo(SCALES, SHIFTS, origins, HMAX),
             sess.summarize_placebo_horizons(SCALES, SHIFTS, origins, per_series))
    return dict(got=got, want=want, bare=bare, cut=cut, acc=acc, seen=seen, means=means, before=before, after=after,
                draws=draws, inp=inp, origins=origins, hz=hz, kernel=sess.kernel_name())
  finally:
    sess.close()


def _assert_zero_rows_and_their_neighbours(acc):
  """acc [G, O, K, 2, N]: what counts nothing reads 0 and what lies next to it does not, so that no
  comparison passes on zeros."""
  assert (acc[:, 5:] == 0.0).all()                                 # the unused origin slots
  assert (acc[:G - 1, :, 3] == 0.0).all() and (acc[G - 1, :, 2:] == 0.0).all()   # the unused horizon slots
  assert (acc[:G - 1, 2, :2] == 0.0).all() and (acc[G - 1, 2, 0] == 0.0).all()   # h = 1, 2 from the missing origin 11
  assert (acc[:G - 1, 2, 2, 1] > 0.0).all() and (acc[G - 1, 2, 1, 1] > 0.0).all()   # h = 9 (5) from it
  assert (acc[:, :2, :2, 1] > 0.0).all() and (acc[:, :2, :2, 0] != 0.0).all()    # h = 1, 2 from the origins 3 and 4


# ---- 1. the bit contract against the existing entry, and numpy ------------------------------------------

@pytest.mark.parametrize("P", [0, 3])
@pytest.mark.parametrize("has_slope,seasons", MODELS)
def test_one_pass_equals_one_call_per_horizon_bit_for_bit_and_numpy(has_slope, seasons, P):
  r = _run(_lengths(seasons), P, has_slope, seasons)
  what = f"slope={has_slope} seasons={seasons} P={P}"
  got = r["got"]
  assert got["acc"].shape == (G, SLOTS, K, 2, N) and got["pit_mean"].shape == (G, SLOTS, K)
  _assert_same_bits(got, r["want"], what)
  _assert_zero_rows_and_their_neighbours(got["acc"])
  for name in OUTPUTS:
    assert ((got[name] == 0.0) == (got["acc"][:, :, :, 1] == 0.0).all(axis=-1)).all(), name
  _compare(got, r["acc"], r["means"], what)
  # without `seen` there are no means and the accumulators are the same bits
  assert sorted(r["bare"]) == ["acc"]
  np.testing.assert_array_equal(r["bare"]["acc"], got["acc"])


@pytest.mark.parametrize("has_slope,seasons", MODELS)
def test_the_result_does_not_depend_on_where_the_entries_are_cut(has_slope, seasons):
  r = _run(_lengths(seasons), 3, has_slope, seasons)
  assert r["cut"][1]["num_chunks"] == 8 and r["cut"][3]["num_chunks"] == 3   # (3: the group of all four is cut)
  for c, cut in r["cut"].items():
    _assert_same_bits(cut, r["got"], f"chunk_entries={c}")


@pytest.mark.parametrize("has_slope,seasons", MODELS)
def test_a_ragged_session_equals_one_call_per_horizon_bit_for_bit_and_numpy(has_slope, seasons):
  r = _run(RAGGED, 3, has_slope, seasons, ragged=True)
  assert "ragged" in r["kernel"] and r["inp"]["lengths"] == list(RAGGED)
  _assert_same_bits(r["got"], r["want"], f"ragged slope={has_slope} seasons={seasons}")
  _assert_zero_rows_and_their_neighbours(r["got"]["acc"])
  _compare(r["got"], r["acc"], r["means"], f"ragged slope={has_slope} seasons={seasons}")
  for c, cut in r["cut"].items():
    _assert_same_bits(cut, r["got"], f"ragged chunk_entries={c}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("P", [0, 3])
@pytest.mark.parametrize("has_slope,seasons", MODELS)
def test_a_session_made_from_draws_equals_one_call_per_horizon_bit_for_bit(has_slope, seasons, P, dtype):
  """float32: the fit's own draws (and the fit's own result, bit for bit); float64: the same draws and
  data moved off the float32 grid, so the float64 build has something of its own to read."""
  r = _run(_lengths(seasons), P, has_slope, seasons)
  inp, draws = r["inp"], dict(r["draws"])
  y, X = inp["y"], inp["X"]
  if dtype is np.float64:
    rng = np.random.default_rng(7)
    wiggle = lambda a: np.asarray(a, np.float64) * (1.0 + 1e-9 * rng.standard_normal(np.shape(a)))
    draws = {k: wiggle(v) for k, v in draws.items()}
    y, X = wiggle(y), None if X is None else wiggle(X)
  blocks_ = len(seasons)
  pb = _native.make_problem(T=inp["T"], P=P, has_slope=has_slope, num_warmup=0, num_results=37, num_chains=2,
                            num_series=4, seed=(5, 9), num_seasons=_model.expand_seasons(seasons, 1)[0])
  if not blocks_:
    draws.pop("seasonal_drift_scales", None)
  if not has_slope:
    draws.pop("slope_scale", None)
  if not P:
    draws.pop("weights", None)
  drawn = _native.DrawsSession(pb, y, inp["mask"], X, inp["sc"] if blocks_ else None, _native.make_params(inp["specs"]),
                               draws, dtype=dtype)
  try:
    got = drawn.pool_placebo_horizons(SCALES, SHIFTS, GROUPS, r["origins"], r["hz"], seen=r["seen"])
    want = _k_calls(drawn, r["origins"], r["hz"], seen=r["seen"])
  finally:
    drawn.close()
  _assert_same_bits(got, want, f"draws {np.dtype(dtype)} slope={has_slope} seasons={seasons} P={P}")
  _assert_zero_rows_and_their_neighbours(got["acc"])
  if dtype is np.float32:
    _assert_same_bits(got, r["got"], "draws float32 against the fit's session")
  else:
    assert (got["acc"] != r["got"]["acc"]).any()


def _open_part(lengths, P, has_slope, seasons, which):
  """The session of the series `which` (consecutive) of the batch of `base._open`, on their stream keys."""
  series = [base._series(T, P, 40 + 7 * b + P, has_slope, seasons) for b, T in enumerate(lengths)]   # pylint: disable=protected-access
  T = max(lengths)
  pb = _native.make_problem(T=T, P=P, has_slope=has_slope, num_warmup=3, num_results=37, num_chains=2,
                            num_series=len(which), seed=(5, 9), series_offset=which[0],
                            num_seasons=_model.expand_seasons(seasons, 1)[0])
  y = base._pad([series[b][0] for b in which], T, np.nan)                      # pylint: disable=protected-access
  mask = base._pad([series[b][1] for b in which], T, True)                     # pylint: disable=protected-access
  X = None if P == 0 else base._pad([series[b][2] for b in which], T, 7.5)     # pylint: disable=protected-access
  return _native.Session(pb, y, mask, X, _model.expand_seasons(seasons, T)[1],
                         _native.make_params([series[b][3] for b in which]))


@pytest.mark.parametrize("has_slope,seasons", [MODELS[1], MODELS[2]], ids=["trend", "seasonal"])
def test_two_sessions_of_two_series_each_hand_the_sum_on_bit_for_bit(has_slope, seasons):
  lengths = _lengths(seasons)
  r = _run(lengths, 3, has_slope, seasons)
  acc = None
  for which in ([0, 1], [2, 3]):
    part = _open_part(lengths, 3, has_slope, seasons, which)
    try:
      part.run()
      own = [{b - which[0]: w for b, w in g.items() if b in which} for g in GROUPS]
      res = part.pool_placebo_horizons(SCALES[which], SHIFTS[which], own, r["origins"][which], r["hz"], init=acc,
                                       seen=r["seen"])
      acc = res["acc"]
    finally:
      part.close()
  _assert_same_bits(res, r["got"], "two sessions chained through init")


@pytest.mark.parametrize("has_slope,seasons", [MODELS[1], MODELS[2]], ids=["trend", "seasonal"])
def test_the_per_series_entries_return_the_same_before_and_after(has_slope, seasons):
  r = _run(_lengths(seasons), 3, has_slope, seasons)
  for before, after in zip(r["before"], r["after"]):
    for name in OUTPUTS:
      np.testing.assert_array_equal(before[name], after[name])
      assert (before[name] != 0.0).any()
  # group 0 is {0: 1.0}: S is SUM of series 0, so its row means are the per-series table's bit for bit
  np.testing.assert_array_equal(r["got"]["predicted_mean"][0], r["before"][1]["predicted_mean"][0])
  np.testing.assert_allclose(r["got"]["pit_mean"][0], r["before"][1]["pit_mean"][0], **TOL)


def test_one_entry_whose_rows_exceed_the_scratch_takes_a_buffer_of_the_call():
  """A session of one series: an entry's 2 x 7 x 6 = 84 rows do not fit the scratch's B * T = 70, so a
  chunk's planes lie in the call's own buffer -- the same bits as K calls on the same session, one entry
  per chunk or both.  (The two refusals by name -- accumulators, or one entry, beyond CI_PATHS_MAX_BYTES
  = 1 GiB -- need 2 O K N doubles beyond that and are not reached at the sizes of a test.)"""
  sess, inp = base._open(list(_lengths(())), 3, True, (), only=0)             # pylint: disable=protected-access
  groups = ({0: 1.0}, {0: -0.5})
  hz = np.array([[1, 2, 3, 5, 9, -1], [2, 5, -1, -1, -1, -1]], np.int32)
  origins = _origins([70])
  seen = 50.0 + np.arange(2 * SLOTS * 6, dtype=np.float64).reshape(2, SLOTS, 6)
  try:
    sess.run()
    assert 2 * SLOTS * hz.shape[1] > inp["T"] * 1
    want = _k_calls(sess, origins, hz, seen=seen, groups=groups, scales=SCALES[0], shifts=SHIFTS[0])
    got = sess.pool_placebo_horizons(SCALES[0], SHIFTS[0], groups, origins, hz, seen=seen)
    cut = sess.pool_placebo_horizons(SCALES[0], SHIFTS[0], groups, origins, hz, seen=seen, chunk_entries=1)
  finally:
    sess.close()
  assert cut["num_chunks"] == 2
  _assert_same_bits(got, want, "the call's own buffer")
  _assert_same_bits(cut, got, "the call's own buffer, one entry per chunk")
  assert (got["acc"][0, :2, :5, 1] > 0.0).all() and (got["acc"][0, 2, :2] == 0.0).all() and (got["acc"][0, 2, 2:5, 1] > 0.0).all()
  np.testing.assert_array_equal(got["acc"][1, :, 0, 1], 0.25 * got["acc"][0, :, 1, 1])   # (h = 2 at the weight -0.5)


@pytest.mark.parametrize("with_init", [False, True], ids=["from zero", "from init"])
def test_the_horizon_slots_in_column_chunks_give_the_same_bits(with_init):
  """`lib.pool_placebo_horizon_columns` with room for two of the four columns per call: the second call
  holds [9, -1] for three groups and no used slot of the last group, which takes no part in it."""
  lengths = _lengths(())
  r = _run(lengths, 3, True, ())
  groups = [dict(g) for g in GROUPS]
  rows = [{b: r["origins"][b] for b in g} for g in GROUPS]
  init = None if not with_init else np.random.default_rng(2).normal(size=(G, SLOTS, K, 2, N))
  per_column = G * SLOTS * 2 * N * 8
  calls = []
  sess, _ = base._open(list(lengths), 3, True, ())                             # pylint: disable=protected-access
  try:
    sess.run()
    entry = sess.pool_placebo_horizons
    def counting(scale, shift, here, origins, table, *a, **k):
      calls.append((np.asarray(table).tolist(), [len(g) for g in here]))
      return entry(scale, shift, here, origins, table, *a, **k)
    sess.pool_placebo_horizons = counting
    whole = lib.pool_placebo_horizon_columns(sess, False, SCALES, SHIFTS, groups, rows, r["hz"], init)
    assert len(calls) == 1
    cut = lib.pool_placebo_horizon_columns(sess, False, SCALES, SHIFTS, groups, rows, r["hz"], init,
                                           max_bytes=2 * per_column + 1)
    single = lib.pool_placebo_horizon_columns(sess, False, SCALES, SHIFTS, groups, rows, r["hz"], init, one_pass=False)
  finally:
    del sess.pool_placebo_horizons
    sess.close()
  assert calls[1:] == [([[1, 2], [1, 2], [1, 2], [2, 5]], [1, 2, 4, 1]), ([[9, -1], [9, -1], [9, -1], [1, -1]], [1, 2, 4, 0])]
  np.testing.assert_array_equal(cut, whole)
  np.testing.assert_array_equal(single, whole)
  if with_init:
    np.testing.assert_array_equal(whole[G - 1, :, 2:], init[G - 1, :, 2:])     # the unused slots keep `init`
    assert (whole[:, :2, :2] != init[:, :2, :2]).all()
  else:
    np.testing.assert_array_equal(whole, r["got"]["acc"])
    _assert_zero_rows_and_their_neighbours(cut)


# ---- 2. the block entry ---------------------------------------------------------------------------------

BLOCK_ROW, BLOCK_OWN = [1, 2, 5, -1], [2, 5, -1, -1]


@functools.lru_cache(maxsize=None)
def _run_blocks(name):
  has_slope, seasons, T = pooled_blocks.MODELS[name]
  sess, inp = blocks._open(4, T, has_slope, seasons)                          # pylint: disable=protected-access
  origins = pooled_blocks._plan(T, has_slope, seasons, 5)                     # pylint: disable=protected-access
  hz = _table(BLOCK_OWN, BLOCK_ROW)
  try:
    sess.run()
    draws = sess.fetch(blocks.PARAM_FIELDS)
    csr = _native.groups_csr(GROUPS, 4)

    @functools.lru_cache(maxsize=None)
    def series_terms(b, h):
      return pooled_blocks._entry_terms(inp, draws, b, has_slope, SCALES[b], SHIFTS[b], origins[b], h)[:2]   # pylint: disable=protected-access

    def seen_of(b, row):
      return lib._placebo_seen(inp["y"][b], inp["mask"][b], origins[b], 5, SCALES[b], SHIFTS[b], horizons=row)[1]   # pylint: disable=protected-access

    acc, seen, means = _numpy(series_terms, seen_of, csr, origins, hz, draws=24)
    want = _k_calls(sess, origins, hz, seen=seen, entry="pool_placebo_blocks")
    got = sess.pool_placebo_horizons(SCALES, SHIFTS, GROUPS, origins, hz, seen=seen, blocks=True)
    cut = {c: sess.pool_placebo_horizons(SCALES, SHIFTS, GROUPS, origins, hz, seen=seen, blocks=True, chunk_entries=c)
           for c in (1, 3)}
    return dict(got=got, want=want, cut=cut, acc=acc, means=means, origins=origins, kernel=sess.kernel_name())
  finally:
    sess.close()


@pytest.mark.parametrize("name", pooled_blocks.NAMES)
def test_the_block_entry_equals_one_call_per_horizon_bit_for_bit_and_numpy(name):
  r = _run_blocks(name)
  got = r["got"]
  assert got["acc"].shape == (G, SLOTS, K, 2, 24)
  _assert_same_bits(got, r["want"], name)
  for c, cut in r["cut"].items():
    _assert_same_bits(cut, got, f"{name} chunk_entries={c}")
  _compare(got, r["acc"], r["means"], f"{name} [{r['kernel']}]")
  acc = got["acc"]
  at40 = list(r["origins"][0]).index(40)
  assert (acc[:, 5:] == 0.0).all() and (acc[:G - 1, :, 3] == 0.0).all() and (acc[G - 1, :, 2:] == 0.0).all()
  assert (acc[:G - 1, at40, 0] == 0.0).all() and (acc[:G - 1, at40, 1:3, 1] > 0.0).all()   # h = 1 from the missing step 40
  assert (acc[:, 4] == 0.0).all()                                    # T - 5: the masked post-period
  first = 1 if at40 == 0 else 0                                      # the origin right behind the state dimension
  assert (acc[:G - 1, first, :3, 1] > 0.0).all() and (acc[G - 1, first, :2, 1] > 0.0).all()


@pytest.mark.parametrize("has_slope,seasons", MODELS)
def test_models_both_families_take_agree_bit_for_bit(has_slope, seasons):
  sess, _ = blocks._open(4, 90, has_slope, seasons)                            # pylint: disable=protected-access
  try:
    sess.run()
    origins = pooled_blocks._plan(90, has_slope, seasons, 5)                  # pylint: disable=protected-access
    hz = _table(BLOCK_OWN, BLOCK_ROW)
    seen = 50.0 + np.arange(G * SLOTS * K, dtype=np.float64).reshape(G, SLOTS, K)
    one_lane = sess.pool_placebo_horizons(SCALES, SHIFTS, GROUPS, origins, hz, seen=seen)
    group = sess.pool_placebo_horizons(SCALES, SHIFTS, GROUPS, origins, hz, seen=seen, blocks=True)
  finally:
    sess.close()
  assert (one_lane["acc"][:, :4, :2, 1] > 0.0).any()
  _assert_same_bits(group, one_lane, f"slope={has_slope} seasons={seasons}")


# ---- 3. refusals ----------------------------------------------------------------------------------------

def test_errors_name_the_group_entry_or_slot_before_any_device_work():
  fn = _native.load().ci_session_pool_placebo_horizons
  sess, _ = base._open([70, 70], 3, False, ())                                 # pylint: disable=protected-access
  good = np.array([[3, 9], [3, -1]], np.int32)
  groups = ({0: 1.0, 1: 2.0}, {1: 1.0})
  hz = np.array([[2, 5], [5, -1]], np.int32)
  try:
    with pytest.raises(_native.NativeError, match="needs a finished ci_session_run"):
      sess.pool_placebo_horizons(1.0, 0.0, groups, good, hz)
    sess.run()
    # the binding's checks, before the library is reached
    for bad, msg in (([[2, 2], [5, -1]], r"horizons\[0\] must be strictly ascending"),
                     ([[2, 5], [-1, 5]], r"horizons\[1\] must be strictly ascending"),
                     ([[2, 5], [0, -1]], r"horizons\[1, 0\] must be at least 1"),
                     ([[2, 5], [-1, -1]], r"horizons\[1\] holds no horizon: every group needs at least one")):
      with pytest.raises(ValueError, match=msg):
        sess.pool_placebo_horizons(1.0, 0.0, groups, good, bad)
    with pytest.raises(ValueError, match=r"`horizons` must be \[2, K\] or \[K\]"):
      sess.pool_placebo_horizons(1.0, 0.0, groups, good, np.ones((3, 2), np.int32))
    with pytest.raises(ValueError, match=r"`horizons` must have 1 to 64 slots per group, got 65"):
      sess.pool_placebo_horizons(1.0, 0.0, groups, good, np.arange(1, 66))
    with pytest.raises(ValueError, match=r"`init` must be \[2, 2, 2, 2, 74\]"):
      sess.pool_placebo_horizons(1.0, 0.0, groups, good, hz, init=np.zeros((2, 2, 2, 74)))
    with pytest.raises(ValueError, match=r"`seen` must be \[2, 2, 2\]"):
      sess.pool_placebo_horizons(1.0, 0.0, groups, good, hz, seen=np.zeros((2, 2)))
    # the C entry's own checks, through the raw call
    one, off = np.ones(2), np.array([0, 2, 3], np.int32)
    members, weights = np.array([0, 1, 1], np.int32), np.ones(3)
    org = np.array([[3, 9], [3, -1], [3, -1]], np.int32)
    out, means = np.zeros((2, 2, 2, 2, 74)), np.zeros((2, 2, 2))
    ptr = lambda a: None if a is None else a.ctypes.data

    def raw(horizons=hz, width=2, O=2, seen=None, mean=None, origins=org, members=members):
      rc = fn(sess._h, one.ctypes.data, one.ctypes.data, 2, off.ctypes.data, members.ctypes.data,  # pylint: disable=protected-access
              weights.ctypes.data, O, ptr(origins), width, ptr(horizons), None, out.ctypes.data, ptr(seen), None, None,
              ptr(mean))
      return rc, _native.load().ci_last_error().decode()

    for kw in (dict(horizons=None), dict(origins=None)):
      rc, msg = raw(**kw)
      assert rc != 0 and "NULL argument" in msg
    for width in (0, 65):
      rc, msg = raw(width=width)
      assert rc != 0 and f"max_horizons must be in [1, 64], got {width}" in msg
    for bad, text in (([[2, 2], [5, -1]], "horizons[0] must be strictly ascending"),
                      ([[2, 5], [0, -1]], "horizons[1, 0] must be at least 1"),
                      ([[2, 5], [-1, -1]], "horizons[1] holds no horizon: every group needs at least one")):
      rc, msg = raw(horizons=np.array(bad, np.int32))
      assert rc != 0 and text in msg, msg
    rc, msg = raw(members=np.array([1, 0, 1], np.int32))
    assert rc != 0 and "group 0: members must be strictly ascending (0 after 1)" in msg
    rc, msg = raw(mean=means)
    assert rc != 0 and "need `seen`" in msg
    for O in (0, 71):
      rc, msg = raw(O=O)
      assert rc != 0 and f"max_origins must be in [1, 70], got {O}" in msg
    rc, msg = raw(seen=means, mean=means)
    assert rc == 0, msg
    # the origins are checked with the group's largest horizon: 9 + 62 > 70, 9 + 61 = 70 is the last admissible
    with pytest.raises(_native.NativeError, match=r"group 0, entry 0 \(member 0\): the origin 9 of slot 1 with horizon 62 "
                                                  r"reaches beyond the series' 70 steps"):
      sess.pool_placebo_horizons(1.0, 0.0, groups, good, [[2, 62], [5, -1]])
    with pytest.raises(_native.NativeError, match=r"group 1, entry 2 \(member 1\): the origins must be strictly ascending"):
      sess.pool_placebo_horizons(1.0, 0.0, groups, [{0: [3, 9], 1: [3, 9]}, {1: [-1, 3]}], hz)
    got = sess.pool_placebo_horizons(1.0, 0.0, groups, good, [[2, 61], [5, -1]])["acc"]
    assert got.shape == (2, 2, 2, 2, 74) and (got[1, :, 1] == 0.0).all() and (got[:, 0, 0, 1] > 0.0).all()
    with pytest.raises(_native.NativeError, match="chunk_entries must be at least 1, got 0"):
      sess.pool_placebo_horizons(1.0, 0.0, groups, good, hz, chunk_entries=0)
  finally:
    sess.close()
  two, _ = base._open([70], 2, False, ((4, 1), (3, 1)))                         # pylint: disable=protected-access
  try:
    with pytest.raises(_native.NativeError, match=r"ci_session_pool_placebo_horizons takes a trend with at most "
                                                  r"one block of 2 to 7 seasons.*\(4, 3\)"):
      two.pool_placebo_horizons(1.0, 0.0, [{0: 1.0}], [[3]], [2, 5])
  finally:
    two.close()
  ragged, _ = base._open([70, 41], 3, False, (), ragged=True)                  # pylint: disable=protected-access
  try:
    ragged.run()
    with pytest.raises(_native.NativeError, match="ci_session_pool_placebo_horizons_blocks takes no ragged session"):
      ragged.pool_placebo_horizons(1.0, 0.0, [{0: 1.0}], [[3], [3]], [2, 5], blocks=True)
  finally:
    ragged.close()


# ---- 4. package level: Placebo(horizons=...) with aggregates= / event_aggregates= -------------------------

import pandas as pd                                                 # pylint: disable=wrong-import-position

import causalimpact as ci                                           # pylint: disable=wrong-import-position
from causalimpact import batch                                      # pylint: disable=wrong-import-position

import test_aggregate_placebo_horizons as host                      # pylint: disable=wrong-import-position

ALPHA, SEED, OPTS = base.ALPHA, base.SEED, base.OPTS
PLAIN = ci.Placebo(max_origins=6)
SEVERAL = ci.Placebo(max_origins=6, horizons=(2, 5))
AGGREGATES = {"all": "all", "pair": {0: 1.0, 2: 0.5}, "one": {1: 1.0}}
NUMERIC = base.NUMERIC


def _route(route):
  kw = dict(alpha=ALPHA, seed=SEED, inference_options=ci.InferenceOptions(**OPTS))
  if route == "two_blocks":
    kw["model_options"] = ci.ModelOptions(seasons=[ci.Seasons(4), ci.Seasons(3)])
  elif route == "float64":
    kw["data_options"] = ci.DataOptions(dtype=np.float64)
  elif route == "hmc":
    kw["inference_options"] = ci.InferenceOptions(sampler="hmc", num_chains=2, num_results=20, num_warmup_steps=20)
  return kw


def _counting(monkeypatch):
  """The filter passes of the one-pass entry (calls with an entry to filter) by the kind of session;
  `pool_placebo` and `pool_placebo_blocks` are barred."""
  passes = []
  entry = _native.Session.pool_placebo_horizons

  def counting(self, scale, shift, groups, *a, **k):
    if any(len(g) for g in groups):
      passes.append(type(self).__name__)
    return entry(self, scale, shift, groups, *a, **k)

  def never(*a, **k):
    raise AssertionError("the one-horizon pooled entry was reached")
  monkeypatch.setattr(_native.Session, "pool_placebo_horizons", counting)
  monkeypatch.setattr(_native.Session, "pool_placebo", never)
  monkeypatch.setattr(_native.Session, "pool_placebo_blocks", never)
  return passes


def _assert_close(got, want, what):
  """Two aggregates' by-horizon frames and profiles to the float64 contract."""
  a, b = got.placebo_by_horizon, want.placebo_by_horizon
  assert a.index.equals(b.index), what
  print(what, "largest deviation per column:", (a[NUMERIC] - b[NUMERIC]).abs().max().to_dict())
  np.testing.assert_allclose(a[NUMERIC].to_numpy(np.float64), b[NUMERIC].to_numpy(np.float64), err_msg=what, **TOL)
  assert list(a["horizon_end"]) == list(b["horizon_end"]) and list(a["significant"]) == list(b["significant"]), what
  np.testing.assert_allclose(got.placebo_profile.to_numpy(), want.placebo_profile.to_numpy(), err_msg=what, **TOL)


@pytest.mark.parametrize("route", ["gibbs", "two_blocks", "float64", "hmc"])
def test_batch_aggregates_gain_the_horizon_frames_from_one_pass_per_launch(route, monkeypatch):
  frames = base._frames()                                                      # pylint: disable=protected-access
  periods = base._periods(frames[0], 0)                                        # pylint: disable=protected-access
  kw = _route(route)
  plain = ci.fit_causalimpact_batch(frames, *periods, aggregates=AGGREGATES, placebo=PLAIN, **kw)
  with monkeypatch.context() as patch:
    passes = _counting(patch)
    got = ci.fit_causalimpact_batch(frames, *periods, aggregates=AGGREGATES, placebo=SEVERAL, **kw)
  one_launch = route != "float64"
  assert (type(got) is ci.CausalImpactBatchAnalysis) == one_launch
  # one launch: one filter pass; series by series: one per entry of the group table (3 + 2 + 1), each on a draws session
  assert passes == {"gibbs": ["Session"], "two_blocks": ["Session"], "hmc": ["DrawsSession"],
                    "float64": ["DrawsSession"] * 6}[route]
  host._assert_rest_equal(got, plain, list(AGGREGATES))                        # pylint: disable=protected-access
  prof = got.aggregate_placebo_profile
  assert prof.index.names == ["aggregate", "horizon"] and plain.aggregate_placebo_profile is None
  for name in AGGREGATES:
    host._assert_identities(got.aggregates[name], plain.aggregates[name], (2, 5), f"{route} {name!r}")   # pylint: disable=protected-access
    pd.testing.assert_frame_equal(prof.loc[name], got.aggregates[name].placebo_profile, check_exact=True)
  # a group of one member at weight 1 has that member's own columns
  own, one = got[1].placebo_by_horizon, got.aggregates["one"].placebo_by_horizon
  assert own.index.equals(one.index) and list(own["horizon_end"]) == list(one["horizon_end"])
  if route in ("gibbs", "two_blocks"):
    # S of the group is SUM of the member and both row means are the device's, taken in the launch's own session:
    # the same bits.  The other routes take one of the two means elsewhere (the series-by-series route finishes
    # the pooled sums in numpy, the member's table on the device): another order of addition, the float64 contract.
    np.testing.assert_array_equal(one["predicted"], own["predicted"])
  print(f"{route}: a group of one member against the member's own table:", (one[NUMERIC] - own[NUMERIC]).abs().max().to_dict())
  np.testing.assert_allclose(one[NUMERIC].to_numpy(np.float64), own[NUMERIC].to_numpy(np.float64), **TOL)
  assert list(one["significant"]) == list(own["significant"])
  numpy_kw = dict(kw, inference_options=ci.InferenceOptions(**dict(
      kw["inference_options"].__dict__, summarize_on_device=False)))
  on_host = ci.fit_causalimpact_batch(frames, *periods, aggregates=AGGREGATES, placebo=SEVERAL, **numpy_kw)
  for name in AGGREGATES:
    _assert_close(on_host.aggregates[name], got.aggregates[name], f"{route} {name!r}, summarize_on_device=False")


def test_every_listed_horizon_alone_gives_its_slice_on_the_device():
  frames = base._frames()                                                      # pylint: disable=protected-access
  periods = base._periods(frames[0], 0)                                        # pylint: disable=protected-access
  kw = _route("gibbs")
  got = ci.fit_causalimpact_batch(frames, *periods, aggregates=AGGREGATES,
                                  placebo=ci.Placebo(max_origins=64, horizons=(2, 5)), **kw)
  H = int(got.aggregate_placebo_quality.loc["all", "horizon"])
  for h in (2, 5):
    alone = ci.fit_causalimpact_batch(frames, *periods, aggregates=AGGREGATES,
                                      placebo=ci.Placebo(horizon=h, min_history=H, max_origins=64), **kw)
    for name in AGGREGATES:
      want = alone.aggregates[name].placebo
      want = want.loc[want.index.intersection(got.aggregates[name].placebo.index)]
      assert len(want) == len(got.aggregates[name].placebo) >= 3
      pd.testing.assert_frame_equal(got.aggregates[name].placebo_by_horizon.xs(h, level="horizon").loc[want.index], want,
                                    check_exact=True)


def test_every_listed_horizon_alone_gives_its_slice_of_a_panels_event_aggregates():
  frames = base._frames(base.PANEL_LENGTHS)                                    # pylint: disable=protected-access
  periods = [base._periods(f, b) for b, f in enumerate(frames)]               # pylint: disable=protected-access
  kw = _route("gibbs")
  got = ci.fit_causalimpact_panel(frames, periods, event_aggregates=AGGREGATES,
                                  placebo=ci.Placebo(max_origins=64, horizons=(2, 5)), **kw)
  first = int(got.aggregate_placebo_quality["horizon"].max())       # (the latest first origin of the groups)
  for h in (2, 5):
    alone = ci.fit_causalimpact_panel(frames, periods, event_aggregates=AGGREGATES,
                                      placebo=ci.Placebo(horizon=h, min_history=first, max_origins=64), **kw)
    for name in AGGREGATES:
      want = alone.aggregates[name].placebo
      want = want.loc[want.index.intersection(got.aggregates[name].placebo.index)]
      assert len(want) >= 2, name                                  # (the origins both plans admit)
      pd.testing.assert_frame_equal(got.aggregates[name].placebo_by_horizon.xs(h, level="horizon").loc[want.index], want,
                                    check_exact=True)


def test_panel_event_aggregates_keep_every_groups_own_horizons(monkeypatch):
  frames = base._frames(base.PANEL_LENGTHS)                                    # pylint: disable=protected-access
  periods = [base._periods(f, b) for b, f in enumerate(frames)]               # pylint: disable=protected-access
  kw = _route("gibbs")
  several = ci.Placebo(max_origins=6, horizons=(2, 5, 9))
  plain = ci.fit_causalimpact_panel(frames, periods, event_aggregates=AGGREGATES, placebo=PLAIN, **kw)
  with monkeypatch.context() as patch:
    passes = _counting(patch)
    got = ci.fit_causalimpact_panel(frames, periods, event_aggregates=AGGREGATES, placebo=several, **kw)
  assert type(got) is ci.CausalImpactPanelAnalysis and passes and set(passes) == {"Session"}
  host._assert_rest_equal(got, plain, list(AGGREGATES))                        # pylint: disable=protected-access
  own = {name: int(got.aggregate_placebo_quality.loc[name, "horizon"]) for name in AGGREGATES}
  assert len(set(own.values())) >= 2                                # (the groups have horizons of their own)
  prof = got.aggregate_placebo_profile
  union = sorted({h for H in own.values() for h in (2, 5, 9) if h <= H} | set(own.values()))
  assert list(prof.index) == [(name, h) for name in AGGREGATES for h in union]
  for name in AGGREGATES:
    one = got.aggregates[name]
    host._assert_identities(one, plain.aggregates[name], (2, 5, 9), f"panel {name!r}")   # pylint: disable=protected-access
    mine = list(one.placebo_profile.index)
    pd.testing.assert_frame_equal(prof.loc[name].loc[mine], one.placebo_profile, check_exact=True)
    others = [h for h in union if h not in mine]
    assert prof.loc[name].loc[others].isna().all().all()             # NaN rows for the horizons it lacks
    assert (one.placebo_by_horizon.index.get_level_values("origin") < 0).all()   # event time: before the start
  assert any(len(got.aggregates[name].placebo_profile) < len(union) for name in AGGREGATES)
  on_host = ci.fit_causalimpact_panel(frames, periods, event_aggregates=AGGREGATES, placebo=several, **dict(
      kw, inference_options=ci.InferenceOptions(summarize_on_device=False, **OPTS)))
  for name in AGGREGATES:
    _assert_close(on_host.aggregates[name], got.aggregates[name], f"panel {name!r}, summarize_on_device=False")


def test_a_library_without_the_block_entry_takes_one_call_per_horizon_the_same_bits(monkeypatch):
  """The fallback the package keeps for a library without ci_session_pool_placebo_horizons_blocks: K calls
  of `pool_placebo_blocks` -- the definition -- give the frames of the one-pass entry exactly."""
  frames = base._frames()                                                      # pylint: disable=protected-access
  periods = base._periods(frames[0], 0)                                        # pylint: disable=protected-access
  kw = _route("two_blocks")
  got = ci.fit_causalimpact_batch(frames, *periods, aggregates=AGGREGATES, placebo=SEVERAL, **kw)
  calls = []
  single = _native.Session.pool_placebo_blocks

  def counting(self, scale, shift, groups, origins, horizon, *a, **k):
    if any(len(g) for g in groups):
      calls.append(sorted(set(np.asarray(horizon).tolist())))
    return single(self, scale, shift, groups, origins, horizon, *a, **k)
  monkeypatch.setattr(_native.Session, "pool_placebo_blocks", counting)
  monkeypatch.setattr(lib, "pool_placebo_horizons_available", lambda blocks: False)
  old = ci.fit_causalimpact_batch(frames, *periods, aggregates=AGGREGATES, placebo=SEVERAL, **kw)
  H = int(got.aggregate_placebo_quality.loc["all", "horizon"])
  assert calls == [[2], [5], [H]]
  for name in AGGREGATES:
    pd.testing.assert_frame_equal(old.aggregates[name].placebo_by_horizon, got.aggregates[name].placebo_by_horizon,
                                  check_exact=True)
    pd.testing.assert_frame_equal(old.aggregates[name].placebo_profile, got.aggregates[name].placebo_profile,
                                  check_exact=True)


@pytest.mark.parametrize("placebo", [True, ci.Placebo(), PLAIN])
def test_without_horizons_the_new_entry_is_never_reached(placebo, monkeypatch):
  def never(*a, **k):
    raise AssertionError("pool_placebo_horizons was reached")
  monkeypatch.setattr(_native.Session, "pool_placebo_horizons", never)
  frames = base._frames()                                                      # pylint: disable=protected-access
  periods = base._periods(frames[0], 0)                                        # pylint: disable=protected-access
  kw = _route("gibbs")
  got = ci.fit_causalimpact_batch(frames, *periods, aggregates=AGGREGATES, placebo=placebo, **kw)
  assert got.aggregate_placebo_quality is not None and got.aggregate_placebo_profile is None
  assert got.aggregates["all"].placebo is not None and got.aggregates["all"].placebo_by_horizon is None
  several = ci.fit_causalimpact_batch(frames, *periods, placebo=SEVERAL, **kw)   # (horizons without aggregates)
  assert several.placebo_profile is not None and several.aggregate_placebo_profile is None
  with pytest.raises(AssertionError, match="pool_placebo_horizons was reached"):
    ci.fit_causalimpact_batch(frames, *periods, aggregates=AGGREGATES, placebo=SEVERAL, **kw)
