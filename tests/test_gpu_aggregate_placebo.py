"""ci_session_pool_placebo on the device -- the placebo forecasts of POOLED sums: the members'
forecasts added draw by draw with the group's weights, their predictive variances with the squared
weights -- at session level against numpy (`_placebo_summary_host(per_draw=True)` on the parameter
draws fetched from the same session, pooled by `_native.pool_placebo_host` and finished by
`_native.finish_placebo_host`), and at package level (`placebo=` with `aggregates=` /
`event_aggregates=`) against the same host twin fed with every member's own fit.

The shapes of tests/test_gpu_placebo.py: T = 70, C = 2 and S = 37 give N = 74 draws (one full
wavefront of lanes and a remainder); the steps 11, 12 and 40 are missing; the origin rows are
[3, 4, 11, 35, T - H, -1, -1] with H 1 and 9.  Every comparison with numpy is to rtol 1e-8,
atol 1e-8, the project's float64 contract (tests/test_gpu_float64.py)."""
import functools

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _native
from causalimpact import causalimpact_lib as lib

import test_gpu_placebo as base

pytestmark = pytest.mark.gpu

TOL = base.TOL
OUTPUTS = base.OUTPUTS
SCALES, SHIFTS = (3.7, 0.5, 2.0, 1.3), (-12.25, 4.0, 0.0, 7.5)
# {0}, {0: 1.0, 2: 0.5}, all four, and series 1 once more: 8 entries for 4 series, so two chunks of
# entries are taken and the group of all four is cut by the chunk boundary
GROUPS = ({0: 1.0}, {0: 1.0, 2: 0.5}, {0: 1.0, 1: -0.75, 2: 2.0, 3: 0.3}, {1: 1.5})


def _host_draws(draws, b):
  pool = lambda a: a[b].reshape((a.shape[1] * a.shape[2],) + a.shape[3:]).astype(np.float64)
  return {k: pool(draws[k]) for k in base.PARAM_FIELDS}


def _entry_terms(inp, draws, b, has_slope, seasons, scale, shift, origins, H):
  """(s, v [O, N], n_counted, seen_sum [O]) of one entry: series b from `origins` with horizon H."""
  Tb = inp["lengths"][b]
  X = None if inp["X"] is None else inp["X"][b, :Tb]
  got = lib._placebo_summary_host(                                            # pylint: disable=protected-access
      inp["y"][b, :Tb], inp["mask"][b, :Tb], X, inp["sc"], [s[0] for s in seasons], has_slope, inp["specs"][b],
      _host_draws(draws, b), scale, shift, origins, H, per_draw=True)
  s, v = _native.placebo_terms_host(got["C"], got["V"], got["cnt"], scale, shift)
  cnt, seen = lib._placebo_seen(inp["y"][b, :Tb], inp["mask"][b, :Tb], origins, H, scale, shift)  # pylint: disable=protected-access
  return s, v, cnt, np.nan_to_num(seen)


def _reference(inp, draws, has_slope, seasons, scales, shifts, csr, origins, horizons):
  """(acc [G, O, 2, N], seen [G, O], means) in numpy; origins [K, O], horizons [G]."""
  offsets, members, weights = csr
  G = offsets.size - 1
  terms = [_entry_terms(inp, draws, int(members[k]), has_slope, seasons, scales[members[k]], shifts[members[k]],
                        origins[k], int(horizons[g]))
           for g in range(G) for k in range(offsets[g], offsets[g + 1])]
  acc = _native.pool_placebo_host(np.stack([t[0] for t in terms]), np.stack([t[1] for t in terms]), csr)
  seen = np.zeros((G, origins.shape[1]))
  for g in range(G):
    for k in range(offsets[g], offsets[g + 1]):
      seen[g] = seen[g] + weights[k] * terms[k][3]
  return acc, seen, _native.finish_placebo_host(acc, seen)


def _compare(got, acc, means, what):
  worst = {"S": float(np.abs(got["acc"][:, :, 0] - acc[:, :, 0]).max()),
           "U": float(np.abs(got["acc"][:, :, 1] - acc[:, :, 1]).max()),
           **{k: float(np.abs(got[k] - means[k]).max()) for k in OUTPUTS}}
  print(f"{what}: largest deviation " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
  np.testing.assert_allclose(got["acc"], acc, err_msg=f"{what} acc", **TOL)
  for k in OUTPUTS:
    np.testing.assert_allclose(got[k], means[k], err_msg=f"{what} {k}", **TOL)


@functools.lru_cache(maxsize=None)
def _run(lengths, P, has_slope, seasons, H):
  """One session of four series: its draws, `summarize_placebo` before and after the pooled call,
  and the pooled call with `seen`."""
  sess, inp = base._open(list(lengths), P, has_slope, seasons)                 # pylint: disable=protected-access
  try:
    sess.run()
    draws = sess.fetch(base.PARAM_FIELDS)
    scales, shifts = np.array(SCALES[:len(lengths)]), np.array(SHIFTS[:len(lengths)])
    origins, horizon = base._plan(inp["lengths"], H)                           # pylint: disable=protected-access
    csr = _native.groups_csr(GROUPS, len(lengths))
    acc, seen, means = _reference(inp, draws, has_slope, seasons, scales, shifts, csr, origins[csr[1]],
                                  [H] * len(GROUPS))
    before = sess.summarize_placebo(scales, shifts, origins, horizon)
    got = sess.pool_placebo(scales, shifts, GROUPS, origins, H, seen=seen)
    bare = sess.pool_placebo(scales, shifts, GROUPS, origins, H)
    after = sess.summarize_placebo(scales, shifts, origins, horizon)
    return dict(got=got, bare=bare, acc=acc, seen=seen, means=means, before=before, after=after, inp=inp,
                origins=origins)
  finally:
    sess.close()


CASES = [((70,) * 4, P, slope, (), H) for P in (0, 5) for slope in (False, True) for H in (1, 9)] + [
    ((133,) * 4, 3, False, ((7, 1),), H) for H in (1, 9)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"T{c[0][0]}-P{c[1]}-slope{int(c[2])}-ns{c[3][0][0] if c[3] else 0}-H{c[4]}")
def test_pooled_sums_and_means_equal_numpy_on_the_fetched_draws(case):
  r = _run(*case)
  got, H = r["got"], case[4]
  N = 74
  assert got["acc"].shape == (len(GROUPS), 7, 2, N) and got["pit_mean"].shape == (len(GROUPS), 7)
  _compare(got, r["acc"], r["means"], f"case {case[1:]}")
  # without `seen` there are no means and the accumulators are the same bits
  assert sorted(r["bare"]) == ["acc"]
  np.testing.assert_array_equal(r["bare"]["acc"], got["acc"])
  # slots that read zero: the unused ones, and the windows that count nothing (origin 11 with H = 1)
  assert (got["acc"][:, 5:] == 0.0).all() and all((got[k][:, 5:] == 0.0).all() for k in OUTPUTS)
  mask = r["inp"]["mask"]
  per_series = np.array([[(~mask[b, o:o + H]).sum() for o in r["origins"][b][:5]] for b in range(4)])
  counted = np.array([per_series[sorted(g)].sum(axis=0) for g in GROUPS])       # member-steps, [G, 5]
  assert ((got["acc"][:, :5, 1] == 0.0).all(axis=2) == (counted == 0)).all()
  assert ((got["acc"][:, :5, 1] > 0.0).all(axis=2) == (counted > 0)).all()
  for k in OUTPUTS:
    assert ((got[k][:, :5] == 0.0) == (counted == 0)).all()
  assert (counted == 0).any() and (counted > 0).any()
  if H == 1:
    assert (counted[:, 2] == 0).all() and (got["acc"][:, 2] == 0.0).all()
  pit = got["pit_mean"][:, :5][counted > 0]
  assert ((pit > 0.0) & (pit < 1.0)).all()


@pytest.mark.parametrize("case", [CASES[3], CASES[-1]], ids=["trend", "seasonal"])
def test_a_group_of_one_member_is_the_per_series_call(case):
  """Group 0 is {0: 1.0}: S is SUM of series 0, so its row means are `summarize_placebo`'s
  predicted_mean bit for bit; pit_mean agrees to the float64 contract (e is formed on the data scale)."""
  r = _run(*case)
  np.testing.assert_array_equal(r["got"]["predicted_mean"][0], r["before"]["predicted_mean"][0])
  print("single-member pit_mean deviation:", float(np.abs(r["got"]["pit_mean"][0] - r["before"]["pit_mean"][0]).max()))
  np.testing.assert_allclose(r["got"]["pit_mean"][0], r["before"]["pit_mean"][0], **TOL)
  np.testing.assert_allclose(r["got"]["spread_mean"][0], r["before"]["spread_mean"][0], **TOL)


@pytest.mark.parametrize("case", [CASES[3], CASES[-1]], ids=["trend", "seasonal"])
def test_the_per_series_call_returns_the_same_before_and_after(case):
  r = _run(*case)
  for k in OUTPUTS:
    np.testing.assert_array_equal(r["before"][k], r["after"][k])


def test_a_batch_cut_into_sessions_continues_the_sum_bit_for_bit():
  """Three series in one session, and as single-series sessions (matching stream keys) chained
  through `init`: the same bits; and once more with `init` and `out` the same buffer."""
  lengths, P, H = [70, 70, 70], 5, 9
  groups = ({0: 1.0, 1: 0.5, 2: 2.0}, {1: 1.0, 2: -1.0})
  scales, shifts = np.array(SCALES[:3]), np.array(SHIFTS[:3])
  origins, _ = base._plan(lengths, H)                                         # pylint: disable=protected-access
  sess, _ = base._open(lengths, P, True, ())                                   # pylint: disable=protected-access
  try:
    sess.run()
    whole = sess.pool_placebo(scales, shifts, groups, origins, H)["acc"]
    # init == out: the raw call on one buffer, from the whole sum as the initial value
    again = sess.pool_placebo(scales, shifts, groups, origins, H, init=whole)["acc"]
    buf = whole.copy()
    csr = _native.groups_csr(groups, 3)
    org = np.ascontiguousarray(origins[csr[1]], dtype=np.int32)
    hz = np.array([H, H], np.int32)
    rc = _native.load().ci_session_pool_placebo(
        sess._h, scales.ctypes.data, shifts.ctypes.data, 2, csr[0].ctypes.data, csr[1].ctypes.data,  # pylint: disable=protected-access
        csr[2].ctypes.data, 7, org.ctypes.data, hz.ctypes.data, buf.ctypes.data, buf.ctypes.data, None, None, None, None)
    assert rc == 0
    np.testing.assert_array_equal(buf, again)
    assert not np.array_equal(again, whole)
  finally:
    sess.close()
  acc = None
  for b in range(3):
    one, _ = base._open(lengths, P, True, (), only=b)                           # pylint: disable=protected-access
    try:
      one.run()
      own = [{0: g[b]} if b in g else {} for g in groups]
      acc = one.pool_placebo(scales[b], shifts[b], own, origins[b:b + 1], H, init=acc)["acc"]
    finally:
      one.close()
  np.testing.assert_array_equal(acc, whole)


@pytest.mark.parametrize("seasons", [(), ((7, 1),)], ids=["trend", "seasonal"])
def test_ragged_sessions_take_every_entrys_own_origins_and_every_groups_horizon(seasons):
  """Lengths 70, 41 and 64 in one launch; the origins of an entry are event-time columns shifted by
  the member's own first step, the two groups have different horizons and origin counts."""
  lengths = (70, 41, 64)
  sess, inp = base._open(list(lengths), 3, False, seasons, ragged=True)        # pylint: disable=protected-access
  try:
    sess.run()
    assert "ragged" in sess.kernel_name()
    draws = sess.fetch(base.PARAM_FIELDS)
    scales, shifts = np.array(SCALES[:3]), np.array(SHIFTS[:3])
    groups = ({0: 1.0, 1: 0.5, 2: 2.0}, {0: -1.0, 2: 1.0})
    columns, first = ([3, 4, 9, 20], [3, 11, 30]), ({0: 20, 1: 2, 2: 10}, {0: 5, 2: 0})
    horizons = [5, 9]
    per_group = [{b: np.array(columns[g]) + first[g][b] for b in groups[g]} for g in range(2)]
    csr = _native.groups_csr(groups, 3)
    origins = np.full((5, 4), -1, np.int32)
    k = 0
    for g in range(2):
      for b in sorted(groups[g]):
        origins[k, :len(columns[g])] = per_group[g][b]
        k += 1
    acc, seen, means = _reference(inp, draws, False, seasons, scales, shifts, csr, origins, horizons)
    got = sess.pool_placebo(scales, shifts, groups, per_group, horizons, seen=seen)
    assert got["acc"].shape == (2, 4, 2, 74)
    _compare(got, acc, means, f"ragged seasons={seasons}")
    assert (got["acc"][1, 3] == 0.0).all() and (got["acc"][:, :3, 1] > 0.0).all()
    # member 1 has 41 steps: column 20 from its step 16 with horizon 5 ends at its last step ...
    per_group[0][1] = np.array(columns[0]) + 16
    assert sess.pool_placebo(scales, shifts, groups, per_group, horizons)["acc"].shape == (2, 4, 2, 74)
    # ... and one step later reaches beyond it
    per_group[0][1] = np.array(columns[0]) + 17
    with pytest.raises(_native.NativeError, match=r"group 0, entry 1 \(member 1\): the origin 37 of slot 3 with horizon 5 "
                                                  r"reaches beyond the series' 41 steps"):
      sess.pool_placebo(scales, shifts, groups, per_group, horizons)
  finally:
    sess.close()


def test_errors_are_reported_before_any_device_work():
  fn = _native.load().ci_session_pool_placebo
  sess, _ = base._open([70, 70], 3, False, ())                                 # pylint: disable=protected-access
  good = np.array([[3, 9], [3, -1]], np.int32)
  groups = ({0: 1.0, 1: 2.0}, {1: 1.0})
  try:
    with pytest.raises(_native.NativeError, match="needs a finished ci_session_run"):
      sess.pool_placebo(1.0, 0.0, groups, good, 5)
    sess.run()
    with pytest.raises(_native.NativeError, match=r"group 1: the horizon must be at least 1, got 0"):
      sess.pool_placebo(1.0, 0.0, groups, good, [5, 0])
    for bad in ([[9, 3], [3, -1]], [[3, 3], [3, -1]]):                        # descending, repeated
      with pytest.raises(_native.NativeError, match=r"group 0, entry 0 \(member 0\): the origins must be strictly "
                                                    r"ascending .* \(slot 1 holds 3\)"):
        sess.pool_placebo(1.0, 0.0, groups, bad, 5)
    with pytest.raises(_native.NativeError, match=r"group 1, entry 2 \(member 1\): the origins must be strictly ascending"):
      sess.pool_placebo(1.0, 0.0, groups, [{0: [3, 9], 1: [3, 9]}, {1: [-1, 3]}], 5)
    with pytest.raises(_native.NativeError, match=r"group 0, entry 1 \(member 1\): slot 0 must hold a step or -1"):
      sess.pool_placebo(1.0, 0.0, groups, [[3, 9], [-2, -1]], 5)
    with pytest.raises(_native.NativeError, match=r"group 0, entry 0 \(member 0\): the origin 66 of slot 1 with horizon 5 "
                                                  r"reaches beyond the series' 70 steps"):
      sess.pool_placebo(1.0, 0.0, groups, [[3, 66], [3, -1]], 5)
    # the group table: members not ascending, through the raw call (`groups_csr` sorts them)
    one, off = np.ones(2), np.array([0, 2], np.int32)
    members, weights = np.array([1, 0], np.int32), np.ones(2)
    org, hz = np.array([[3, 9], [3, 9]], np.int32), np.array([5], np.int32)
    out, means = np.zeros((1, 2, 2, 74)), np.zeros((1, 2))
    ptr = lambda a: None if a is None else a.ctypes.data

    def raw(members, O=2, seen=None, mean=None, origins=org):
      rc = fn(sess._h, one.ctypes.data, one.ctypes.data, 1, off.ctypes.data, members.ctypes.data,  # pylint: disable=protected-access
              weights.ctypes.data, O, ptr(origins), hz.ctypes.data, None, out.ctypes.data, ptr(seen), None, None, ptr(mean))
      return rc, _native.load().ci_last_error().decode()

    rc, msg = raw(members)
    assert rc != 0 and "group 0: members must be strictly ascending (0 after 1)" in msg
    members = np.array([0, 1], np.int32)
    rc, msg = raw(members, mean=means)
    assert rc != 0 and "need `seen`" in msg
    rc, msg = raw(members, origins=None)
    assert rc != 0 and "NULL argument" in msg
    for O in (0, 71):
      rc, msg = raw(members, O)
      assert rc != 0 and f"max_origins must be in [1, 70], got {O}" in msg
    rc, msg = raw(members, seen=means, mean=means)
    assert rc == 0, msg
    with pytest.raises(ValueError, match=r"`init` must be \[2, 2, 2, 74\]"):
      sess.pool_placebo(1.0, 0.0, groups, good, 5, init=np.zeros((2, 2, 74)))
    with pytest.raises(ValueError, match=r"`seen` must be \[2, 2\]"):
      sess.pool_placebo(1.0, 0.0, groups, good, 5, seen=np.zeros(2))
    got = sess.pool_placebo(1.0, 0.0, groups, [[3, 65], [3, -1]], 5)["acc"]      # 65 + 5 = 70: the last admissible
    assert got.shape == (2, 2, 2, 74) and (got[1, 1] == 0.0).all() and (got[:, 0, 1] > 0.0).all()
    assert (got[0, 1] == 0.0).all()                     # (its window lies in the masked post-period: nothing counted)
  finally:
    sess.close()
  two, _ = base._open([70], 2, False, ((4, 1), (3, 1)))                         # pylint: disable=protected-access
  try:
    with pytest.raises(_native.NativeError, match=r"ci_session_pool_placebo takes a trend with at most "
                                                  r"one block of 2 to 7 seasons.*\(4, 3\)"):
      two.pool_placebo(1.0, 0.0, [{0: 1.0}], [[3]], 5)
  finally:
    two.close()


# ---- package level: placebo= with aggregates= / event_aggregates= ----------------------------------

ALPHA, SEED, OPTS = base.ALPHA, base.SEED, base.OPTS
PLACEBO = ci.Placebo(max_origins=5)
AGGREGATES = {"all": "all", "pair": {0: 1.0, 2: 0.5}}
NUMERIC = base.NUMERIC


def _member_entry(b, frame, periods, origins, H):
  """`lib._placebo_entry_host` of series b from its OWN fit (the single fit on the key of series b
  draws what the batch draws for it), for the origins and the horizon of a group."""
  from causalimpact import _model, data as cid                                  # pylint: disable=import-outside-toplevel
  one = ci.fit_causalimpact(frame, *periods, alpha=ALPHA, seed=_native.series_stream_key((0, SEED), b),
                            inference_options=ci.InferenceOptions(**OPTS))
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
  inputs = lib.SeriesInputs(y, mask, design, np.zeros((0, y.shape[0]), np.uint8), (), False, params)
  return lib._placebo_entry_host(inputs, draws, rq["scale"], rq["shift"], rq["observed"], origins, H)   # pylint: disable=protected-access


def _host_aggregate_frames(got, pp, names, frames, periods):
  """{name: (placebo, placebo_quality)} by the host twin from every member's own fit."""
  offsets, members, weights = pp.csr
  entries = {}
  for g in range(len(names)):
    for k in range(offsets[g], offsets[g + 1]):
      b = int(members[k])
      entries[k] = _member_entry(b, frames[b], periods[b], pp.origins[k], int(pp.horizon[g]))
  acc = _native.pool_placebo_host(np.stack([entries[k]["s"] for k in sorted(entries)]),
                                  np.stack([entries[k]["v"] for k in sorted(entries)]), pp.csr)
  pooled = {c: np.zeros(pp.columns.shape) for c in ("seen_sum", "actual", "n_counted")}
  for g in range(len(names)):
    for k in range(offsets[g], offsets[g + 1]):
      pooled["seen_sum"][g] = pooled["seen_sum"][g] + weights[k] * entries[k]["seen_sum"]
      pooled["actual"][g] = pooled["actual"][g] + weights[k] * entries[k]["actual"]
      pooled["n_counted"][g] = pooled["n_counted"][g] + entries[k]["n_counted"]
  means = _native.finish_placebo_host(acc, pooled["seen_sum"])
  out = {}
  for g, name in enumerate(names):
    psum = dict({c: v[g] for c, v in means.items()}, n_counted=pooled["n_counted"][g], seen_sum=pooled["seen_sum"][g])
    out[name] = lib._aggregate_placebo_frames(                                # pylint: disable=protected-access
        psum, pooled["actual"][g], pp.columns[g], int(pp.horizon[g]), ALPHA, pp.labels[g], int(pp.n_post[g]),
        got.aggregates[name].summary.loc["cumulative", "rel_effect"])
  return out


def _assert_pooled(got, want, names, what):
  quality = got.aggregate_placebo_quality
  assert list(quality.index) == list(names) and list(quality.columns) == list(lib.PLACEBO_QUALITY_ENTRIES)
  for name in names:
    frame, row = got.aggregates[name].placebo, got.aggregates[name].placebo_quality
    base._assert_close(frame, row, *want[name], f"{what} {name!r}")            # pylint: disable=protected-access
    np.testing.assert_allclose(quality.loc[name].to_numpy(), want[name][1].to_numpy(), **TOL)
    assert ((frame["pit"] > 0) & (frame["pit"] < 1)).all() and (frame["predicted_sd"] > 0).all()


def _assert_rest_unchanged(got, without_placebo, without_aggregates, names):
  assert without_placebo.aggregate_placebo_quality is None and without_aggregates.aggregate_placebo_quality is None
  assert all(without_placebo.aggregates[name].placebo is None for name in names)
  pd.testing.assert_frame_equal(got.summary, without_placebo.summary, check_exact=True)
  pd.testing.assert_frame_equal(got.aggregate_summary, without_placebo.aggregate_summary, check_exact=True)
  pd.testing.assert_frame_equal(got.placebo_quality, without_aggregates.placebo_quality, check_exact=True)
  for name in names:
    pd.testing.assert_frame_equal(got.aggregates[name].series, without_placebo.aggregates[name].series, check_exact=True)
    pd.testing.assert_frame_equal(got.aggregates[name].summary, without_placebo.aggregates[name].summary, check_exact=True)
  for b in range(len(got)):
    pd.testing.assert_frame_equal(got[b].series, without_placebo[b].series, check_exact=True)
    pd.testing.assert_frame_equal(got[b].placebo, without_aggregates[b].placebo, check_exact=True)


def test_batch_pooled_placebo_equals_the_host_twin_on_every_members_own_fit():
  from causalimpact import batch                                               # pylint: disable=import-outside-toplevel
  frames = base._frames()                                                      # pylint: disable=protected-access
  periods = base._periods(frames[0], 0)                                        # pylint: disable=protected-access
  kw = dict(alpha=ALPHA, seed=SEED, inference_options=ci.InferenceOptions(**OPTS))
  got = ci.fit_causalimpact_batch(frames, *periods, aggregates=AGGREGATES, placebo=PLACEBO, **kw)
  assert type(got) is ci.CausalImpactBatchAnalysis             # (the one-launch route)
  names, csr = batch.aggregate_groups(AGGREGATES, range(3))
  own = got[0].placebo
  prep = got._prep                                                             # pylint: disable=protected-access
  n_post = int(np.count_nonzero(prep.flags & 2))
  H, origins = lib.placebo_plan(PLACEBO, prep.num_pre, n_post, 1)
  pp = batch.batch_placebo_pool_plan(csr, origins, H, n_post, prep.index[prep.model_rows])
  assert len(origins) == 5 and got.aggregates["all"].placebo.index.equals(own.index)
  _assert_pooled(got, _host_aggregate_frames(got, pp, names, frames, [periods] * 3), names, "batch")
  _assert_rest_unchanged(got, ci.fit_causalimpact_batch(frames, *periods, aggregates=AGGREGATES, **kw),
                         ci.fit_causalimpact_batch(frames, *periods, placebo=PLACEBO, **kw), names)


def test_panel_pooled_placebo_equals_the_host_twin_in_event_time():
  from causalimpact import batch                                               # pylint: disable=import-outside-toplevel
  frames = base._frames(base.PANEL_LENGTHS)                                    # pylint: disable=protected-access
  periods = [base._periods(f, b) for b, f in enumerate(frames)]               # pylint: disable=protected-access
  kw = dict(alpha=ALPHA, seed=SEED, inference_options=ci.InferenceOptions(**OPTS))
  got = ci.fit_causalimpact_panel(frames, periods, event_aggregates=AGGREGATES, placebo=PLACEBO, **kw)
  assert type(got) is ci.CausalImpactPanelAnalysis
  names, csr = batch.aggregate_groups(AGGREGATES, range(3))
  prep = got._prep                                                             # pylint: disable=protected-access
  pp = batch.event_placebo_pool_plan(PLACEBO, batch.event_plan(names, csr, prep, "y"), 1)
  assert len(set(pp.horizon)) == 2 and (pp.columns >= 0).any(axis=1).all()   # (two groups, two horizons)
  for g, name in enumerate(names):
    assert got.aggregates[name].placebo.index.name == "origin" and (got.aggregates[name].placebo.index < 0).all()
    for k in range(csr[0][g], csr[0][g + 1]):                                   # inside every member's own pre-period
      assert pp.origins[k].max() + pp.horizon[g] <= prep.num_pre[csr[1][k]]
  _assert_pooled(got, _host_aggregate_frames(got, pp, names, frames, periods), names, "panel")
  _assert_rest_unchanged(got, ci.fit_causalimpact_panel(frames, periods, event_aggregates=AGGREGATES, **kw),
                         ci.fit_causalimpact_panel(frames, periods, placebo=PLACEBO, **kw), names)


@pytest.mark.parametrize("route", ["two_blocks", "hmc"])
def test_batches_the_device_filter_does_not_take_pool_in_numpy_inside_the_launch(route):
  """Two seasonal blocks (Gibbs) and the one-launch HMC batch: the launch fetches its parameter draws
  and the host twin pools the members' forecasts.  The pooled forecast is the weighted sum of the
  members' forecasts, which the same launch filtered in numpy for every series."""
  frames = base._frames()                                                      # pylint: disable=protected-access
  periods = base._periods(frames[0], 0)                                        # pylint: disable=protected-access
  kw = dict(alpha=ALPHA, seed=SEED, placebo=PLACEBO, aggregates=AGGREGATES)
  if route == "hmc":
    kw["inference_options"] = ci.InferenceOptions(sampler="hmc", num_chains=2, num_results=20, num_warmup_steps=20)
  else:
    kw["inference_options"] = ci.InferenceOptions(**OPTS)
    kw["model_options"] = ci.ModelOptions(seasons=[ci.Seasons(4), ci.Seasons(3)])
  got = ci.fit_causalimpact_batch(frames, *periods, **kw)
  assert type(got) is ci.CausalImpactBatchAnalysis             # (one launch, not series by series)
  assert list(got.aggregate_placebo_quality.index) == list(AGGREGATES)
  for name, members in (("all", {0: 1.0, 1: 1.0, 2: 1.0}), ("pair", AGGREGATES["pair"])):
    frame = got.aggregates[name].placebo
    assert list(frame.columns) == list(lib.PLACEBO_COLUMNS) and frame.index.equals(got[0].placebo.index)
    assert len(frame) >= 3 and got.aggregate_placebo_quality.loc[name, "n_origins"] == len(frame)
    for column, weight in (("predicted", lambda w: w), ("actual", lambda w: w), ("n_counted", lambda w: 1.0)):
      want = sum(weight(w) * got[b].placebo[column].to_numpy() for b, w in members.items())
      np.testing.assert_allclose(frame[column], want, err_msg=f"{route} {name} {column}", **TOL)
    assert ((frame["pit"] > 0) & (frame["pit"] < 1)).all() and (frame["predicted_sd"] > 0).all()
    # independent members: the pooled variance is below the square of the summed sds and above 0
    sds = sum(abs(w) * got[b].placebo["predicted_sd"].to_numpy() for b, w in members.items())
    assert (frame["predicted_sd"] < sds).all()
