"""Event-time aggregates of a panel on the device: ci_session_pool_event_trajectories
(csrc/ci_pool.h) against the numpy loop of its definition on ragged trend sessions (stride 47,
N*T odd: the offset of a row from the 16-byte grid changes with the draw) and ragged seasonal
sessions (stride a multiple of 4), the running sum chained over sessions, the argument checks that
need a session, and `fit_causalimpact_panel(event_aggregates=...)` on every route against the host
arithmetic on numpy-pooled draws.  3 chains x 27 draws, 10 warm-up steps, one covariate."""
import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _model
from causalimpact import _native
from causalimpact import batch
from causalimpact import causalimpact_lib as lib
from causalimpact import data as cid

pytestmark = pytest.mark.gpu

CHAINS, DRAWS, WARMUP = 3, 27, 10
N = CHAINS * DRAWS
ALPHA, SEED = 0.05, (5, 11)
WEEKLY = ci.ModelOptions(seasons=[ci.Seasons(num_seasons=7)])


def _options(**kw):
  return ci.InferenceOptions(num_results=DRAWS, num_chains=CHAINS, num_warmup_steps=WARMUP, **kw)


def _frame(num_rows, seed, start=None, missing=None):
  """One covariate; the outcome steps up by 1 from row `start` on."""
  rng = np.random.default_rng(seed)
  x = rng.normal(size=num_rows)
  y = (1.5 * x + 10.0 + 3.0 * seed + np.cumsum(0.1 * rng.normal(size=num_rows))
       + 0.3 * rng.normal(size=num_rows))
  if start is not None:
    y[start:] += 1.0
  if missing is not None:
    y[missing] = np.nan
  return pd.DataFrame({"y": y, "x0": x})


def _assert_frames_equal(a: pd.DataFrame, b: pd.DataFrame, rtol=1e-10):
  """The comparison of tests/test_gpu_aggregates.py for device against host frames."""
  assert list(a.columns) == list(b.columns) and list(a.index) == list(b.index)
  for c in a.columns:
    if a[c].dtype.kind in "fc":
      np.testing.assert_allclose(a[c].to_numpy(float), b[c].to_numpy(float), rtol=rtol,
                                 atol=1e-12, equal_nan=True, err_msg=str(c))
    else:
      assert (a[c] == b[c]).all(), c


def _assert_values_identical(a: pd.DataFrame, b: pd.DataFrame):
  """Every numeric column array_equal (NaN == NaN), every other column equal, whatever the index."""
  assert list(a.columns) == list(b.columns) and len(a) == len(b)
  for c in a.columns:
    if a[c].dtype.kind in "fc":
      np.testing.assert_array_equal(a[c].to_numpy(float), b[c].to_numpy(float), err_msg=str(c))
    else:
      assert (a[c].to_numpy() == b[c].to_numpy()).all(), c


def _loop(traj, scale, shift, groups, stride, init=None):
  """The definition: per group, over the members ascending, acc = acc + w * (traj[first : first +
  width] * scale + shift), every operation rounded on its own in float64; 0.0 beyond the width."""
  out = np.zeros((len(groups), traj.shape[1], stride))
  for g, (group, width) in enumerate(groups):
    if init is not None:
      out[g, :, :width] = init[g, :, :width]
    for b in sorted(group):
      w, first = group[b]
      value = traj[b, :, first:first + width].astype(np.float64) * np.float64(scale[b]) + np.float64(shift[b])
      out[g, :, :width] = out[g, :, :width] + np.float64(w) * value
  return out


class _Panel:
  """A panel as `fit_causalimpact_panel` prepares it, and sessions over some of its positions built
  the way `batch._run_launch` builds them."""

  def __init__(self, frames, periods, model_options=None):
    self.frames, self.periods = frames, periods
    self.model_options = model_options or ci.ModelOptions()
    self.prep = batch.prepare_panel(frames, periods)
    y = batch._sampler_outcome(self.prep, ci.DataOptions())
    with np.errstate(invalid="ignore"):
      pre_sd = [np.nanstd(y[b, :nb], ddof=1) for b, nb in enumerate(self.prep.num_pre)]
    self.fit = batch._new_fit(self.prep, y, self.prep.lengths, pre_sd, ALPHA, SEED, self.model_options,
                              _options(), False)

  def session(self, ids, kind):
    """(session not yet run, stride): a ragged or ragged seasonal session over the positions `ids`."""
    f, ids = self.fit, np.asarray(ids, np.int64)
    T = int(f.lengths[ids].max())
    stride = (T + 3) & ~3 if kind == "ragged_seasonal" else T

    def rows(a, fill):
      a = a[ids, :T]
      return np.concatenate([a, np.full((len(ids), stride - T) + a.shape[2:], fill, a.dtype)], axis=1)

    num_seasons, season_change = _model.expand_seasons(self.model_options.seasons, stride)
    design = rows(f.design, 0.0)
    pb = _native.make_problem(T=stride, P=design.shape[2], has_slope=False, num_seasons=num_seasons,
                              num_warmup=WARMUP, num_results=DRAWS, num_chains=CHAINS,
                              num_series=len(ids), seed=f.seed, device=0)
    sess = _native.Session.ragged(pb, f.lengths[ids], rows(f.y, np.nan), rows(f.mask, True), design,
                                  _native.make_params([f.params[b] for b in ids]), series_ids=ids,
                                  season_change=season_change if kind == "ragged_seasonal" else None)
    return sess, stride


def _trajectories(sess):
  pb = sess.pb
  return sess.fetch(["posterior_trajectories"])["posterior_trajectories"].reshape(pb.num_series, N, pb.T)


# ---- the entry point against its numpy loop ----------------------------------------------------------
# five series of a ragged trend session of stride 47; the groups of tests/test_gpu_aggregates.py and a
# sixth, every member with a first step of its own: all residues mod 4, widths 1, 3, 4, 5, 9 and 47,
# series 0 from step 0 (the first float of the buffer), series 4 up to step 47 (the last one)
TREND_LENGTHS = [47, 40, 47, 33, 47]
TREND_GROUPS = [({0: (1.0, 0), 1: (1.0, 1), 2: (1.0, 2), 3: (1.0, 3), 4: (1.0, 38)}, 9),
                ({0: (0.5, 5), 3: (-2.0, 6)}, 1),
                ({2: (1.0, 7)}, 3),
                ({1: (1.0, 10), 2: (0.25, 11), 3: (1.0, 13)}, 4),
                ({2: (1.0, 3), 3: (3.0, 1), 4: (1.0, 42)}, 5),
                ({0: (1.0, 0), 1: (1.0, 0), 2: (1.0, 0), 3: (1.0, 0), 4: (1.0, 0)}, 47)]
# the ragged seasonal session: stride 92; one group whose first steps are all multiples of 4 (with the
# stride a multiple of 4 every quad is then aligned) among groups that are not
WEEKLY_LENGTHS = [60, 75, 90, 66, 81]
WEEKLY_GROUPS = [({0: (1.0, 0), 1: (1.0, 13), 2: (1.0, 30), 3: (1.0, 7), 4: (1.0, 83)}, 9),
                 ({0: (0.5, 5), 3: (-2.0, 6)}, 1),
                 ({2: (1.0, 7)}, 3),
                 ({1: (1.0, 10), 2: (0.25, 11), 3: (1.0, 13)}, 4),
                 ({2: (1.0, 3), 3: (3.0, 1), 4: (1.0, 87)}, 5),
                 ({0: (1.0, 0), 1: (1.0, 0), 2: (1.0, 0), 3: (1.0, 0), 4: (1.0, 0)}, 92)]
ALIGNED_GROUPS = [({0: (1.0, 0), 1: (1.0, 12), 2: (1.0, 28), 3: (1.0, 8), 4: (1.0, 80)}, 12),
                  ({1: (0.5, 4), 4: (-2.0, 40)}, 7)]


def _panel_of(lengths, model_options=None):
  frames = [_frame(T, b, start=T - 12) for b, T in enumerate(lengths)]
  periods = [((0, T - 13), (T - 12, T - 1)) for T in lengths]
  return _Panel(frames, periods, model_options)


@pytest.fixture(scope="module")
def trend():
  """(panel, trajectories [5, N, 47], scale, shift, {name: pooled}) of one ragged trend session."""
  panel = _panel_of(TREND_LENGTHS)
  f = panel.fit
  sess, stride = panel.session(range(5), "ragged")
  assert stride == 47 and (N * stride) % 2 == 1
  try:
    sess.run()
    traj = _trajectories(sess)
    rng = np.random.default_rng(7)
    init = rng.normal(size=(len(TREND_GROUPS), N, 47)) * 50.0
    wide_init = rng.normal(size=(len(TREND_GROUPS), N, 50)) * 50.0
    for g, (_, width) in enumerate(TREND_GROUPS):           # beyond the width init is never looked at
      init[g, :, width:] = np.nan
      wide_init[g, :, width:] = np.nan
    got = dict(
        plain=sess.pool_event_trajectories(f.scale, f.shift, TREND_GROUPS),
        continued=sess.pool_event_trajectories(f.scale, f.shift, TREND_GROUPS, init),
        wide=sess.pool_event_trajectories(f.scale, f.shift, TREND_GROUPS, wide_init, out_stride=50),
        narrow=sess.pool_event_trajectories(f.scale, f.shift, TREND_GROUPS[1:5]),
        full=sess.pool_event_trajectories(f.scale, f.shift, [({b: (w, 0) for b, (w, _) in g.items()}, 47)
                                                             for g, _ in TREND_GROUPS]),
        whole=sess.pool_trajectories(f.scale, f.shift, [{b: w for b, (w, _) in g.items()}
                                                        for g, _ in TREND_GROUPS]),
        init=init, wide_init=wide_init)
  finally:
    sess.close()
  return panel, traj, got


def test_event_pool_equals_the_numpy_loop_on_rows_off_the_vector_grid(trend):
  panel, traj, got = trend
  f = panel.fit
  assert [w for _, w in TREND_GROUPS] == [9, 1, 3, 4, 5, 47]
  assert {first % 4 for g, _ in TREND_GROUPS for _, first in g.values()} == {0, 1, 2, 3}
  assert got["plain"].shape == (6, N, 47) and got["plain"].dtype == np.float64
  np.testing.assert_array_equal(got["plain"], _loop(traj, f.scale, f.shift, TREND_GROUPS, 47))
  np.testing.assert_array_equal(got["continued"], _loop(traj, f.scale, f.shift, TREND_GROUPS, 47, got["init"]))
  assert not np.array_equal(got["plain"], got["continued"])
  # rows longer than the widest group, and than the session's stride: 0.0 beyond a width, with init too
  np.testing.assert_array_equal(got["wide"], _loop(traj, f.scale, f.shift, TREND_GROUPS, 50, got["wide_init"]))
  for name in ("plain", "continued", "wide"):
    for g, (_, width) in enumerate(TREND_GROUPS):
      assert (got[name][g, :, width:] == 0.0).all(), (name, g)
  # out_stride defaults to the widest group: 5 columns here
  assert got["narrow"].shape == (4, N, 5)
  np.testing.assert_array_equal(got["narrow"], _loop(traj, f.scale, f.shift, TREND_GROUPS[1:5], 5))


def test_full_width_from_step_zero_is_pool_trajectories_bit_for_bit(trend):
  _, _, got = trend
  np.testing.assert_array_equal(got["full"], got["whole"])


@pytest.fixture(scope="module")
def weekly():
  """The same on a ragged seasonal session (stride 92), cut in two for the chain: positions 0, 2, 4
  and positions 1, 3."""
  panel = _panel_of(WEEKLY_LENGTHS, WEEKLY)
  f = panel.fit
  sess, stride = panel.session(range(5), "ragged_seasonal")
  assert stride == 92
  try:
    sess.run()
    traj = _trajectories(sess)
    init = np.random.default_rng(8).normal(size=(len(WEEKLY_GROUPS), N, 92)) * 50.0
    got = dict(
        plain=sess.pool_event_trajectories(f.scale, f.shift, WEEKLY_GROUPS),
        continued=sess.pool_event_trajectories(f.scale, f.shift, WEEKLY_GROUPS, init),
        aligned=sess.pool_event_trajectories(f.scale, f.shift, ALIGNED_GROUPS),
        full=sess.pool_event_trajectories(f.scale, f.shift, [({b: (w, 0) for b, (w, _) in g.items()}, 92)
                                                             for g, _ in WEEKLY_GROUPS]),
        whole=sess.pool_trajectories(f.scale, f.shift, [{b: w for b, (w, _) in g.items()}
                                                        for g, _ in WEEKLY_GROUPS]),
        init=init)
  finally:
    sess.close()
  return panel, traj, got


def test_event_pool_equals_the_numpy_loop_on_aligned_rows(weekly):
  panel, traj, got = weekly
  f = panel.fit
  np.testing.assert_array_equal(got["plain"], _loop(traj, f.scale, f.shift, WEEKLY_GROUPS, 92))
  np.testing.assert_array_equal(got["continued"], _loop(traj, f.scale, f.shift, WEEKLY_GROUPS, 92, got["init"]))
  assert all(first % 4 == 0 for g, _ in ALIGNED_GROUPS for _, first in g.values())
  np.testing.assert_array_equal(got["aligned"], _loop(traj, f.scale, f.shift, ALIGNED_GROUPS, 12))
  np.testing.assert_array_equal(got["full"], got["whole"])


# ---- groups of more members than one chunk of loads ---------------------------------------------------
# 15 series of 17 steps in one ragged trend session (stride 17, N*T odd).  The kernel adds the members
# of a group in chunks of 8, 4, 2 and 1: 15 = 8 + 4 + 2 + 1 and 9 = 8 + 1.  The first steps cover all
# residues mod 4; the group of 15 starts at the first float of the buffer (series 0 from step 0) and
# ends at the last one (series 14 up to step 17): the quads that go element by element.  Widths 9 and
# 6 in rows of 14 columns.
MANY_GROUPS = [({b: ((-1.0) ** b * (0.25 + 0.5 * b), f)
                 for b, f in enumerate([0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 1, 2, 3, 5, 8])}, 9),
               ({b: (3.0 - b, f) for b, f in zip((0, 2, 3, 5, 6, 8, 9, 11, 12), (3, 0, 1, 2, 7, 6, 5, 4, 11))}, 6)]
# ... and 15 series of 20 steps, every first step and the width a multiple of 4: the aligned build
MANY_ALIGNED_GROUPS = [({b: (0.5 * b - 3.0, 4 * (b % 4)) for b in range(15)}, 8)]


@pytest.fixture(scope="module")
def many():
  """Per session (trajectories, scale, shift, {name: pooled}): 15 series of 17 steps, 15 of 20."""
  out = []
  for T, groups, stride in ((17, MANY_GROUPS, 14), (20, MANY_ALIGNED_GROUPS, None)):
    panel = _panel_of([T] * 15)
    f = panel.fit
    sess, session_stride = panel.session(range(15), "ragged")
    assert session_stride == T
    try:
      sess.run()
      traj = _trajectories(sess)
      init = np.random.default_rng(9).normal(size=(len(groups), N, stride or groups[0][1])) * 50.0
      for g, (_, width) in enumerate(groups):               # beyond the width init is never looked at
        init[g, :, width:] = np.nan
      got = dict(plain=sess.pool_event_trajectories(f.scale, f.shift, groups, out_stride=stride),
                 continued=sess.pool_event_trajectories(f.scale, f.shift, groups, init, out_stride=stride),
                 init=init)
    finally:
      sess.close()
    out.append((traj, f.scale, f.shift, got))
  return out


@pytest.mark.parametrize("with_init", [False, True])
def test_event_groups_of_15_and_9_members_equal_the_numpy_loop(many, with_init):
  traj, scale, shift, got = many[0]
  assert [len(g) for g, _ in MANY_GROUPS] == [15, 9] and traj.shape == (15, N, 17)
  for group, width in MANY_GROUPS:
    assert {first % 4 for _, first in group.values()} == {0, 1, 2, 3} and width % 4 != 0
  assert MANY_GROUPS[0][0][0][1] == 0 and MANY_GROUPS[0][0][14][1] + MANY_GROUPS[0][1] == 17
  want = _loop(traj, scale, shift, MANY_GROUPS, 14, got["init"] if with_init else None)
  np.testing.assert_array_equal(got["continued" if with_init else "plain"], want)


@pytest.mark.parametrize("with_init", [False, True])
def test_event_group_of_15_members_equals_the_numpy_loop_on_aligned_rows(many, with_init):
  traj, scale, shift, got = many[1]
  group, width = MANY_ALIGNED_GROUPS[0]
  assert len(group) == 15 and traj.shape[2] % 4 == 0 and width % 4 == 0
  assert all(first % 4 == 0 for _, first in group.values())
  want = _loop(traj, scale, shift, MANY_ALIGNED_GROUPS, 8, got["init"] if with_init else None)
  np.testing.assert_array_equal(got["continued" if with_init else "plain"], want)


def _cut_groups(groups, ids):
  place = {b: i for i, b in enumerate(ids)}
  return [({place[b]: wf for b, wf in group.items() if b in place}, width) for group, width in groups]


def test_running_sum_chained_over_two_sessions_equals_the_loop_over_both(weekly):
  """Positions 0, 2, 4, then positions 1, 3 fed the first part's output: the loop over both sessions'
  trajectories in that order.  A group without a member in the second session passes through it.
  The argument checks that need a session are made on the second one."""
  panel, _, _ = weekly
  f = panel.fit
  groups = WEEKLY_GROUPS[:5]
  want, acc = None, None
  for k, ids in enumerate(([0, 2, 4], [1, 3])):
    sess, stride = panel.session(ids, "ragged_seasonal")
    assert stride == (92, 76)[k]
    try:
      cut = _cut_groups(groups, ids)
      if k == 1:
        assert cut[2] == ({}, 3)
        with pytest.raises(_native.NativeError, match="needs a finished ci_session_run"):
          sess.pool_event_trajectories(f.scale[ids], f.shift[ids], cut, acc, out_stride=92)
      sess.run()
      acc = sess.pool_event_trajectories(f.scale[ids], f.shift[ids], cut, acc, out_stride=92)
      want = _loop(_trajectories(sess), f.scale[ids], f.shift[ids], cut, 92, want)
      if k == 1:
        np.testing.assert_array_equal(acc[2], before[2])
        _check_refusals(sess, stride)
      before = acc.copy()
    finally:
      sess.close()
  np.testing.assert_array_equal(acc, want)


def _check_refusals(sess, T):
  """Straight through ctypes (the binding would not build these tables): a session of two series."""
  L = _native.load()
  two, out = np.ones(2), np.zeros((1, N, T))

  def call(offsets, members, weights, first, width, out_stride=T, num_groups=1):
    arrays = [np.asarray(offsets, np.int32), np.asarray(members, np.int32), np.asarray(weights, np.float64),
              np.asarray(first, np.int32), np.asarray(width, np.int32)]
    o, m, w, f, wd = [a.ctypes.data for a in arrays]
    rc = L.ci_session_pool_event_trajectories(sess._h, two.ctypes.data, two.ctypes.data, num_groups, o, m,
                                              w, f, wd, out_stride, None, out.ctypes.data)
    return rc, L.ci_last_error()

  for args, message in [(([0, 1], [0], [1.0], [0], [0]), b"width 0 outside [1, out_stride"),
                        (([0, 1], [0], [1.0], [0], [T]), b"outside [1, out_stride = 5]"),
                        (([0, 1], [0], [1.0], [-1], [4]), b"is negative"),
                        (([0, 1], [1], [1.0], [T - 3], [4]), b"ends beyond the session's"),
                        (([0, 2], [0, 1], [1.0, 1.0], [0, 1], [T]), b"ends beyond the session's"),
                        # ... and what ci_session_pool_trajectories checks
                        (([1, 2], [0, 1], [1.0, 1.0], [0, 0], [4]), b"offsets[0] must be 0"),
                        (([0, 1], [2], [1.0], [0], [4]), b"out of range"),
                        (([0, 2], [1, 0], [1.0, 1.0], [0, 0], [4]), b"strictly ascending"),
                        (([0, 1], [0], [np.nan], [0], [4]), b"not finite")]:
    kw = dict(out_stride=5) if b"out_stride = 5" in message else {}
    rc, error = call(*args, **kw)
    assert rc != 0 and message in error, (args, error)
  rc, error = call([0, 0], [0], [1.0], [0], [T + 1], out_stride=T + 1)        # a group without a member too
  assert rc != 0 and b"exceeds the session's" in error
  rc, error = call([0], [0], [1.0], [0], [4], num_groups=0)
  assert rc != 0 and b"num_groups must be >= 1" in error
  off, mem, one = np.array([0, 1], np.int32), np.zeros(1, np.int32), np.ones(1, np.int32)
  for first, width in ((None, one.ctypes.data), (mem.ctypes.data, None)):
    rc = L.ci_session_pool_event_trajectories(sess._h, two.ctypes.data, two.ctypes.data, 1, off.ctypes.data,
                                              mem.ctypes.data, two.ctypes.data, first, width, T, None,
                                              out.ctypes.data)
    assert rc != 0 and b"NULL argument" in L.ci_last_error()


# ---- the public call ----------------------------------------------------------------------------------
class _Spy:
  """Records every `Session.pool_event_trajectories` of a fit with the trajectories of its session."""

  def __init__(self, monkeypatch):
    self.calls = []
    real = _native.Session.pool_event_trajectories

    def spy(sess, scale, shift, groups, init=None, out_stride=None):
      out = real(sess, scale, shift, groups, init, out_stride)
      self.calls.append(dict(traj=_trajectories(sess), scale=np.array(scale), shift=np.array(shift),
                             groups=groups, init=None if init is None else init.copy(), out=out.copy(),
                             stride=out_stride))
      return out

    monkeypatch.setattr(_native.Session, "pool_event_trajectories", spy)

  def assert_every_step_is_the_loop(self):
    assert self.calls
    for call in self.calls:
      np.testing.assert_array_equal(call["out"], _loop(call["traj"], call["scale"], call["shift"],
                                                       call["groups"], call["stride"], call["init"]))


def _host_frames(res, frames, periods, members, order, traj_of, prep):
  """(series, summary) of one aggregate by the host arithmetic (`_compute_impact` on numpy-pooled
  draws): members {position: weight} added in `order`; traj_of[b] the data-scale draws [N, T_b] of
  series b."""
  axis = batch.event_axes(prep, _native.groups_csr([members], len(frames)))[0]
  first = dict(zip(sorted(b for b, w in members.items() if w != 0.0), axis.first))
  W = axis.width
  pooled, outcome, mean = np.zeros((N, W)), np.zeros(W), np.zeros(W)
  for b in order:
    if members.get(b, 0.0) == 0.0:
      continue
    w, f, Tb = members[b], first[b], int(prep.lengths[b])
    d = cid.CausalImpactData(frames[b], *periods[b])
    own_mean = np.ravel(d.outcome_scaler.inverse_transform(res._means[b, :Tb].astype(np.float64)))
    model_outcome = frames[b]["y"].to_numpy()[prep.model_rows[b]]
    pooled = pooled + w * traj_of[b][:, f:f + W]
    outcome = outcome + w * model_outcome[f:f + W]
    mean = mean + w * own_mean[f:f + W]
  index = pd.Index(np.arange(-axis.L, axis.H), name="event_time")
  ci_data = cid.CausalImpactData(pd.DataFrame({"y": outcome}, index=index),
                                 (0, axis.L - axis.gap - 1), (axis.L, axis.L + axis.Hwin - 1),
                                 standardize_data=False)
  assert ci_data.pre_period == (-axis.L, -1 - axis.gap) and ci_data.post_period == (0, axis.Hwin - 1)
  return lib._compute_impact(mean, pooled, ci_data, ALPHA)


def _data_scale_draws(spy_calls, launches, prep):
  """{position: [N, T_b] float64 data-scale draws} from the sessions the spy saw, one per launch."""
  assert len(spy_calls) == len(launches)
  out = {}
  for call, (_, _, ids) in zip(spy_calls, launches):
    for i, b in enumerate(ids):
      Tb = int(prep.lengths[b])
      out[b] = call["traj"][i, :, :Tb].astype(np.float64) * prep.outcome_sd[b] + prep.outcome_mean[b]
  return out


# six series in two steps-per-thread classes (five of 40..60 steps, position 2 of 300), every one with
# its own periods; position 1 leaves a gap of 3 between pre-period and start and drops 4 rows in
# front, position 4 misses an outcome value inside its window
API_NAMES = ["n", "s", "long", "e", "w", "c"]
API_FRAMES = [_frame(48, 0, 36), _frame(60, 1, 45), _frame(300, 2, 270), _frame(40, 3, 28),
              _frame(55, 4, 40, missing=44), _frame(52, 5, 38)]
API_PERIODS = [((0, 35), (36, 47)), ((4, 41), (45, 56)), ((0, 269), (270, 289)), ((0, 27), (28, 39)),
               ((0, 39), (40, 51)), ((0, 37), (38, 49))]
API_AGGREGATES = {"total": "all", "mix": {"n": 0.5, "long": -2.0, "w": 1.5}, "one": ["s"]}
API_MEMBERS = [{b: 1.0 for b in range(6)}, {0: 0.5, 2: -2.0, 4: 1.5}, {1: 1.0}]


def _fit_api(frames=API_FRAMES, periods=API_PERIODS, names=API_NAMES, aggregates=API_AGGREGATES, devices=(0,),
             **kw):
  return ci.fit_causalimpact_panel(frames, periods, alpha=ALPHA, seed=SEED, names=names,
                                   inference_options=_options(devices=list(devices)),
                                   event_aggregates=aggregates, **kw)


@pytest.fixture(scope="module")
def api():
  with pytest.MonkeyPatch.context() as patch:
    spy = _Spy(patch)
    res = _fit_api()
  return res, spy


def test_api_frames_equal_the_host_arithmetic_in_class_then_position_order(api):
  res, spy = api
  prep = batch.prepare_panel(API_FRAMES, API_PERIODS)
  route = batch.panel_route(float64=False, standardize_data=True, sampler="gibbs", num_seasonal_blocks=0,
                            P=2, lengths=prep.lengths)
  assert route == dict(route="ragged", groups=[(1, [0, 1, 3, 4, 5]), (2, [2])])
  launches = batch.panel_launches(route, [0])
  spy.assert_every_step_is_the_loop()
  assert spy.calls[1]["init"] is not None and len(spy.calls[1]["groups"]) == 2    # "one" passes through
  draws = _data_scale_draws(spy.calls, launches, prep)
  assert list(res.aggregates) == list(API_AGGREGATES)
  for name, members in zip(API_AGGREGATES, API_MEMBERS):
    series, summary = _host_frames(res, API_FRAMES, API_PERIODS, members, [0, 1, 3, 4, 5, 2], draws, prep)
    got = res.aggregates[name]
    assert got.series.index.name == "event_time" and got.posterior_samples is None
    _assert_frames_equal(got.series, series)
    _assert_frames_equal(got.summary, summary)
    _assert_frames_equal(res.aggregate_summary.loc[name], summary)
    assert np.isfinite(got.series["posterior_mean"].to_numpy()).all()
  assert list(res.aggregate_summary.index) == [(a, r) for a in API_AGGREGATES for r in ("average", "cumulative")]
  assert list(res.aggregate_summary.columns) == list(res.summary.columns)
  # total: L = 28 (position 3), the gap of position 1, windows of 12, H = 12
  total = res.aggregates["total"].series
  assert list(total.index) == list(range(-28, 12))
  assert ci.plot(res.aggregates["total"]) is not None    # an integer index is nothing new to the plots


def test_api_does_not_depend_on_the_split_over_devices(api):
  res, _ = api
  two = _fit_api(devices=(0, 0))
  for name in API_AGGREGATES:
    pd.testing.assert_frame_equal(res.aggregates[name].series, two.aggregates[name].series, check_exact=True)
    pd.testing.assert_frame_equal(res.aggregates[name].summary, two.aggregates[name].summary, check_exact=True)
  pd.testing.assert_frame_equal(res.aggregate_summary, two.aggregate_summary, check_exact=True)
  pd.testing.assert_frame_equal(res.summary, two.summary, check_exact=True)


def test_api_group_of_one_series_is_that_series(api):
  res, _ = api
  own = res[1]
  got = res.aggregates["one"]
  steps = 60 - 4                                         # the rows from its pre-period on
  assert len(got.series) == steps and list(got.series.index) == list(range(-41, 15))
  # ... every column but the four period marks, which are on the event axis: the series' own, shifted
  # by its treatment start (row 45 of its frame)
  marks = ["pre_period_start", "pre_period_end", "post_period_start", "post_period_end"]
  _assert_values_identical(got.series.drop(columns=marks), own.series.iloc[-steps:].drop(columns=marks))
  np.testing.assert_array_equal(got.series[marks].to_numpy(), own.series.iloc[-steps:][marks].to_numpy() - 45)
  assert got.series[marks].iloc[0].tolist() == [-41, -4, 0, 11]
  _assert_values_identical(got.summary, own.summary)
  _assert_values_identical(res.aggregate_summary.loc["one"], own.summary)


def test_api_without_event_aggregates_nothing_changes(api):
  res, _ = api
  none = _fit_api(aggregates=None)
  plain = ci.fit_causalimpact_panel(API_FRAMES, API_PERIODS, alpha=ALPHA, seed=SEED, names=API_NAMES,
                                    inference_options=_options(devices=[0]))
  assert none.aggregates is None and none.aggregate_summary is None
  assert plain.aggregates is None and plain.aggregate_summary is None
  pd.testing.assert_frame_equal(none.summary, plain.summary, check_exact=True)
  pd.testing.assert_frame_equal(res.summary, plain.summary, check_exact=True)     # ... nor with them
  for b in range(6):
    pd.testing.assert_frame_equal(none[b].series, plain[b].series, check_exact=True)
    pd.testing.assert_frame_equal(res[b].series, plain[b].series, check_exact=True)
    pd.testing.assert_frame_equal(res[b].summary, plain[b].summary, check_exact=True)


# ---- the other routes ---------------------------------------------------------------------------------
ROUTE_LENGTHS = {"ragged_seasonal": [60, 75, 90, 66], "equal_length": [60, 60, 72, 60]}
ROUTE_MODELS = {"ragged_seasonal": WEEKLY,
                "equal_length": ci.ModelOptions(seasons=[ci.Seasons(num_seasons=7), ci.Seasons(num_seasons=4)])}


@pytest.mark.parametrize("route", ["ragged_seasonal", "equal_length"])
def test_api_on_the_other_one_launch_routes(route, monkeypatch):
  lengths, model = ROUTE_LENGTHS[route], ROUTE_MODELS[route]
  frames = [_frame(T, 10 + b, start=T - 14 - b) for b, T in enumerate(lengths)]
  periods = [((0, T - 15 - b), (T - 14 - b, T - 3)) for b, T in enumerate(lengths)]
  names = ["a", "b", "c", "d"]
  aggregates = {"total": "all", "mix": {"a": 0.5, "c": -2.0, "d": 1.0}}
  members = [{b: 1.0 for b in range(4)}, {0: 0.5, 2: -2.0, 3: 1.0}]
  prep = batch.prepare_panel(frames, periods)
  routed = batch.panel_route(float64=False, standardize_data=True, sampler="gibbs",
                             num_seasonal_blocks=len(model.seasons), P=2, lengths=prep.lengths,
                             num_seasons=_model.expand_seasons(model.seasons, 1)[0])
  assert routed["route"] == route
  launches = batch.panel_launches(routed, [0])
  order = [b for _, _, ids in launches for b in ids]
  assert order == ([0, 1, 2, 3] if route == "ragged_seasonal" else [0, 1, 3, 2])
  spy = _Spy(monkeypatch)
  res = _fit_api(frames, periods, names, aggregates, model_options=model)
  spy.assert_every_step_is_the_loop()
  draws = _data_scale_draws(spy.calls, launches, prep)
  for name, group in zip(aggregates, members):
    series, summary = _host_frames(res, frames, periods, group, order, draws, prep)
    _assert_frames_equal(res.aggregates[name].series, series)
    _assert_frames_equal(res.aggregates[name].summary, summary)


def test_float64_panel_pools_on_the_per_series_route():
  """Three series, float64: fitted series by series, the windows added in numpy in position order."""
  frames = [_frame(48, 20, 36), _frame(60, 21, 45), _frame(40, 22, 28)]
  periods = [((0, 35), (36, 47)), ((4, 41), (45, 56)), ((0, 27), (28, 39))]
  names = ["n", "s", "e"]
  aggregates = {"total": "all", "one": ["s"], "mix": {"n": 0.5, "e": -2.0}}
  kw = dict(alpha=ALPHA, seed=SEED, names=names, data_options=ci.DataOptions(dtype=np.float64),
            inference_options=_options())
  res = ci.fit_causalimpact_panel(frames, periods, event_aggregates=aggregates, **kw)
  assert isinstance(res, batch.PerSeriesBatchAnalysis) and list(res.aggregates) == list(aggregates)
  plain = ci.fit_causalimpact_panel(frames, periods, **kw)
  assert plain.aggregates is None and plain.aggregate_summary is None
  _assert_frames_equal(res.summary, plain.summary)
  own = res[1]
  assert list(res.aggregates["one"].series.index) == list(range(-41, 15))
  marks = ["pre_period_start", "pre_period_end", "post_period_start", "post_period_end"]
  _assert_frames_equal(res.aggregates["one"].series.drop(columns=marks).reset_index(drop=True),
                       own.series.iloc[-56:].drop(columns=marks).reset_index(drop=True))
  assert res.aggregates["one"].series[marks].iloc[0].tolist() == [-41, -4, 0, 11]
  _assert_frames_equal(res.aggregates["one"].summary, own.summary)
  # the total against the host arithmetic on the three single fits' trajectories
  sunk = []
  for b in range(3):
    lib.fit_causalimpact(frames[b], *periods[b], seed=_native.series_stream_key(SEED, b), alpha=ALPHA,
                         data_options=ci.DataOptions(dtype=np.float64), inference_options=_options(),
                         _trajectory_sink=lambda *a: sunk.append(a))
  prep = batch.prepare_panel(frames, periods)
  axis = batch.event_axes(prep, _native.groups_csr([[0, 1, 2]], 3))[0]
  assert (axis.L, axis.gap, axis.Hwin, axis.H, axis.first.tolist()) == (28, 3, 12, 12, [8, 13, 0])
  W = axis.width
  draws, mean, outcome = np.zeros((N, W)), np.zeros(W), np.zeros(W)
  for b, (pm, tr, scale, shift) in enumerate(sunk):
    f = int(axis.first[b])
    assert tr.dtype == np.float64 and tr.shape == (N, prep.lengths[b])
    draws = draws + 1.0 * (tr * scale + shift)[:, f:f + W]
    mean = mean + 1.0 * (np.ravel(pm) * scale + shift)[f:f + W]
    outcome = outcome + 1.0 * frames[b]["y"].to_numpy()[prep.model_rows[b]][f:f + W]
  ci_data = cid.CausalImpactData(pd.DataFrame({"y": outcome}, index=axis.index), (0, 24), (28, 39),
                                 standardize_data=False)
  series, summary = lib._compute_impact(mean, draws, ci_data, ALPHA)
  _assert_frames_equal(res.aggregates["total"].series, series)
  _assert_frames_equal(res.aggregates["total"].summary, summary)
