"""Event-time aggregates of a panel (`fit_causalimpact_panel(event_aggregates=...)`), the parts that
need no GPU: the event axes of a hand-made panel, the pooled rows, the numpy accumulator of the
per-series route, the chain of pool steps over launches whose positions interleave, the refusals of
the public call ahead of any device work, and the C-ABI entry point
ci_session_pool_event_trajectories: declared, bound and exported with one signature, NULL arguments
refused before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _native
from causalimpact import batch
from causalimpact import causalimpact_lib as lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["a", "b", "c", "d"]


def _frame(num_rows, seed):
  rng = np.random.default_rng(seed)
  x = rng.normal(size=num_rows)
  y = 1.5 * x + 10.0 + seed + np.cumsum(0.1 * rng.normal(size=num_rows)) + 0.3 * rng.normal(size=num_rows)
  return pd.DataFrame({"y": y, "x": x})


# series        rows   pre-period   post-period   model steps  start  gap  window  steps from start
#   a            40     0..29        30..39          40         30     0     10        10
#   b            50     5..34        37..46          45         32     2     10        13   (gap 2, tail 3)
#   c            45     0..19        20..25          45         20     0      6        25   (short window)
#   d            30     0..11        12..29          30         12     0     18        18
FRAMES = [_frame(40, 0), _frame(50, 1), _frame(45, 2), _frame(30, 3)]
PERIODS = [((0, 29), (30, 39)), ((5, 34), (37, 46)), ((0, 19), (20, 25)), ((0, 11), (12, 29))]


# ---- the event axes --------------------------------------------------------------------------------
def test_event_axes_of_a_hand_made_panel():
  prep = batch.prepare_panel(FRAMES, PERIODS, names=NAMES)
  np.testing.assert_array_equal(prep.lengths, [40, 45, 45, 30])
  np.testing.assert_array_equal(prep.num_pre, [30, 30, 20, 12])
  _, csr = batch.aggregate_groups({"all": "all", "ab": {"b": 2.0, "a": 1.0, "d": 0.0}, "c": ["c"],
                                   "bd": ["d", "b"]}, NAMES)
  axes = batch.event_axes(prep, csr)
  got = [(x.L, x.gap, x.Hwin, x.H, x.first.tolist()) for x in axes]
  assert got == [(12, 2, 6, 10, [18, 20, 8, 0]),      # all: d has the fewest steps in front, a behind
                 (30, 2, 10, 10, [0, 2]),             # d has weight 0: it does not shape the axis
                 (20, 0, 6, 25, [0]),                 # one series: its own steps
                 (12, 2, 10, 13, [20, 0])]
  assert [x.width for x in axes] == [22, 40, 45, 25]
  for x, m in zip(axes, ([0, 1, 2, 3], [0, 1], [2], [1, 3])):      # every window inside its series
    assert x.first.dtype == np.int32
    assert (x.first >= 0).all() and (x.first + x.width <= prep.lengths[m]).all()
  one = axes[0]
  assert one.index.name == "event_time" and one.index.tolist() == list(range(-12, 10))
  np.testing.assert_array_equal(one.flags, [0] * 12 + [3] * 6 + [1] * 4)
  # a group of one series gets that series' own flags
  np.testing.assert_array_equal(axes[2].flags, prep.flags[2, :45])


def test_event_plan_pools_outcome_and_observed_over_the_shifted_windows():
  frames = [f.copy() for f in FRAMES]
  frames[2].iloc[22, 0] = np.nan                        # c misses a value at its tau = 2
  prep = batch.prepare_panel(frames, PERIODS, names=NAMES)
  names, csr = batch.aggregate_groups({"all": "all", "mix": {"a": 0.5, "c": -2.0}}, NAMES)
  plan = batch.event_plan(names, csr, prep, "y")
  assert plan.names == ["all", "mix"] and plan.stride == 30          # the widest group
  y = [f["y"].to_numpy() for f in frames]
  model = [y[0], y[1][5:], y[2], y[3]]                  # b drops the rows before its pre-period
  want = ((0.0 + 1.0 * model[0][18:40]) + 1.0 * model[1][20:42]) + 1.0 * model[2][8:30]
  want = want + 1.0 * model[3][0:22]
  data = plan.data[0]
  np.testing.assert_array_equal(data.data["y"].to_numpy(), want)
  assert data.data.index.name == "event_time"
  assert (data.pre_period, data.post_period) == ((-12, -3), (0, 5))
  assert not data.standardize_data
  observed = plan.observed[0]
  tau = np.arange(-12, 10)
  nan_at = set(tau[np.isnan(observed)])
  assert nan_at == {-2, -1, 2, 6, 7, 8, 9}              # b's gap, c's missing value, c's tail
  np.testing.assert_array_equal(observed[~np.isnan(observed)], want[~np.isnan(observed)])
  # mix: a and c only -- L = 20, no gap, the window of c, what a has behind its start
  mix = plan.axes[1]
  assert (mix.L, mix.gap, mix.Hwin, mix.H, mix.first.tolist()) == (20, 0, 6, 10, [10, 0])
  np.testing.assert_array_equal(plan.data[1].data["y"].to_numpy(),
                                (0.0 + 0.5 * model[0][10:40]) + -2.0 * model[2][0:30])


# ---- the numpy definition and the accumulator of the per-series route -------------------------------
def _event_loop(traj, scale, shift, groups, stride, init=None):
  """The definition, element by element: groups = [({series: (weight, first)}, width)], the members
  of a group in ascending order."""
  N = traj[0].shape[0]
  out = np.zeros((len(groups), N, stride))
  for g, (group, width) in enumerate(groups):
    for n in range(N):
      for c in range(width):
        acc = 0.0 if init is None else float(init[g, n, c])
        for b in sorted(group):
          w, first = group[b]
          value = float(traj[b][n, first + c]) * float(scale[b]) + float(shift[b])
          acc = acc + w * value
        out[g, n, c] = acc
  return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_event_host_pool_equals_an_explicit_loop_bit_for_bit(dtype):
  rng = np.random.default_rng(2)
  lengths, N = [9, 12, 7, 10], 5
  traj = [rng.normal(size=(N, T)).astype(dtype) for T in lengths]
  pm = [rng.normal(size=T).astype(dtype) for T in lengths]
  scale, shift = rng.uniform(0.5, 30.0, 4), rng.normal(size=4) * 100.0
  groups = [({0: (1.0, 2), 1: (1.0, 5), 2: (1.0, 0), 3: (1.0, 3)}, 7), ({0: (0.5, 0), 3: (-2.0, 1)}, 9),
            ({2: (1.0, 1)}, 4)]
  csr = _native.groups_csr([{b: w for b, (w, _) in g.items()} for g, _ in groups], 4)
  axes = [batch.EventAxis(L=1, gap=0, Hwin=1, H=width - 1,
                          first=np.array([g[b][1] for b in sorted(g)], np.int32)) for g, width in groups]
  pool = batch.HostPool(csr, axes)
  assert pool.stride == 9
  for b in range(4):
    pool.add(b, pm[b], traj[b], scale[b], shift[b])
  want = _event_loop(traj, scale, shift, groups, 9)
  np.testing.assert_array_equal(pool.pooled, want)
  assert (pool.pooled[0, :, 7:] == 0.0).all() and (pool.pooled[2, :, 4:] == 0.0).all()
  for b in range(4):
    np.testing.assert_array_equal(pool.means[b], pm[b].astype(np.float64) * scale[b] + shift[b])
  # `_native.pool_event_host` is the same definition on a padded [B, N, T] block, `init` continued
  block = np.zeros((4, N, 12), dtype)
  for b, T in enumerate(lengths):
    block[b, :, :T] = traj[b]
  np.testing.assert_array_equal(_native.pool_event_host(block, scale, shift, groups), want)
  init = rng.normal(size=(3, N, 11))
  got = _native.pool_event_host(block, scale, shift, groups, init, out_stride=11)
  np.testing.assert_array_equal(got, _event_loop(traj, scale, shift, groups, 11, init))
  assert (got[2, :, 4:] == 0.0).all()                                  # also where init is not
  with pytest.raises(ValueError, match="leaves"):
    _native.pool_event_host(block, scale, shift, [({1: (1.0, 6)}, 7)])
  with pytest.raises(ValueError, match="every width must be in"):
    _native.pool_event_host(block, scale, shift, groups, out_stride=8)


def test_event_groups_csr_keeps_first_next_to_its_member():
  offsets, members, weights, first, width = _native.event_groups_csr(
      [({3: (1.0, 7), 1: (2.0, 5), 2: (0.0, 9)}, 4), ({}, 2), ({0: (-1.0, 0)}, 6)], 5)
  np.testing.assert_array_equal(offsets, [0, 2, 2, 3])
  np.testing.assert_array_equal(members, [1, 3, 0])
  np.testing.assert_array_equal(weights, [2.0, 1.0, -1.0])
  np.testing.assert_array_equal(first, [5, 7, 0])                      # zero weight: left out with its first
  np.testing.assert_array_equal(width, [4, 2, 6])
  assert first.dtype == np.int32 and width.dtype == np.int32


# ---- the chain of pool steps over the launches of a panel -------------------------------------------
class _FakePanel:
  """Five series in two length classes whose positions interleave: class 1 holds 0, 2, 4 (12 steps),
  class 2 holds 1, 3 (20 steps).  Values of very different magnitude, so that the order of addition
  shows in the last bits."""

  def __init__(self):
    rng = np.random.default_rng(5)
    self.lengths = [12, 20, 12, 20, 12]
    self.N = 3
    self.traj = [(rng.normal(size=(self.N, T)) * 10.0 ** rng.integers(-3, 4)).astype(np.float32)
                 for T in self.lengths]
    self.scale, self.shift = rng.uniform(1, 2, 5), rng.normal(size=5)
    self.groups = [({0: (1.0, 2), 1: (1.0, 9), 2: (1.0, 0), 3: (1.0, 4), 4: (1.0, 1)}, 10),
                   ({0: (0.5, 0), 3: (-2.0, 8)}, 12), ({2: (1.0, 3)}, 6), ({1: (1.0, 0), 3: (0.25, 0)}, 20)]
    self.csr = _native.groups_csr([{b: w for b, (w, _) in g.items()} for g, _ in self.groups], 5)
    self.axes = [batch.EventAxis(L=1, gap=0, Hwin=1, H=width - 1,
                                 first=np.array([g[b][1] for b in sorted(g)], np.int32))
                 for g, width in self.groups]

  def pool_of(self, launch, seen=None):
    """What a ragged session over the positions of `launch` would compute, in numpy."""
    ids = list(launch[2])
    T = max(self.lengths[b] for b in ids)
    block = np.zeros((len(ids), self.N, T), np.float32)
    for i, b in enumerate(ids):
      block[i, :, :self.lengths[b]] = self.traj[b]

    def pool(groups, init):
      if seen is not None:
        seen.append((tuple(ids), [sorted(group) for group, _ in groups]))
      return _native.pool_event_host(block, self.scale[ids], self.shift[ids], groups, init, out_stride=20)
    return pool

  def want(self, order):
    """The sums with the members added in `order`."""
    out = np.zeros((len(self.groups), self.N, 20))
    for g, (group, width) in enumerate(self.groups):
      for b in order:
        if b in group:
          w, first = group[b]
          value = self.traj[b][:, first:first + width].astype(np.float64) * self.scale[b] + self.shift[b]
          out[g, :, :width] = out[g, :, :width] + w * value
    return out


def test_panel_chain_adds_in_class_then_position_order():
  panel = _FakePanel()
  want = panel.want([0, 2, 4, 1, 3])
  assert not np.array_equal(want, panel.want([0, 1, 2, 3, 4]))        # not plain position order
  cuts = [([(0, 1, [0, 2, 4]), (0, 2, [1, 3])], ((0, 2, 4), [[0, 1, 2], [0], [1]])),
          ([(0, 1, [0, 2]), (1, 1, [4]), (0, 2, [1]), (1, 2, [3])], ((0, 2), [[0, 1], [0], [1]]))]
  for launches, first_step in cuts:
    chain = batch._PoolChain(launches, panel.csr, panel.axes)
    assert chain.stride == 20
    seen = []
    for launch in launches:
      chain.step(launch, panel.pool_of(launch, seen))
    np.testing.assert_array_equal(chain.result(), want)
    # only the groups with a member in a launch went to its pool step, by place within the launch
    assert seen[0] == first_step
    # side by side on two devices, every device its launches in list order
    chain = batch._PoolChain(launches, panel.csr, panel.axes)
    lib.map_by_device(chain.guarded(lambda launch: chain.step(launch, panel.pool_of(launch))), launches)
    np.testing.assert_array_equal(chain.result(), want)


def test_panel_chain_passes_a_group_without_a_member_through():
  panel = _FakePanel()
  launches = [(0, 1, [0, 2, 4]), (0, 2, [1, 3])]
  chain = batch._PoolChain(launches, panel.csr, panel.axes)
  assert chain.groups_of([1, 3]) == [({0: (1.0, 9), 1: (1.0, 4)}, 10), ({1: (-2.0, 8)}, 12), ({}, 6),
                                     ({0: (1.0, 0), 1: (0.25, 0)}, 20)]
  chain.step(launches[0], panel.pool_of(launches[0]))
  first = chain._futures[0].result()
  assert (first[3] == 0.0).all()                          # no member in the first launch: still zero
  chain.step(launches[1], panel.pool_of(launches[1]))
  np.testing.assert_array_equal(chain.result()[2], first[2])           # untouched by the second launch
  assert (chain.result()[3] != 0.0).any()


def test_panel_chain_failure_fails_every_later_launch():
  panel = _FakePanel()
  launches = [(0, 1, [0, 2]), (1, 1, [4]), (0, 2, [1]), (1, 2, [3])]
  chain = batch._PoolChain(launches, panel.csr, panel.axes)

  def run(launch):
    if launch[2] == [0, 2]:
      raise RuntimeError("the fit of the first launch failed")
    chain.step(launch, panel.pool_of(launch))

  with pytest.raises(RuntimeError, match="first launch failed"):
    lib.map_by_device(chain.guarded(run), launches)
  for future in chain._futures:
    with pytest.raises(RuntimeError, match="first launch failed"):
      future.result(timeout=0)
  with pytest.raises(RuntimeError, match="first launch failed"):
    chain.result()
  # a pool step that fails does the same
  chain = batch._PoolChain(launches, panel.csr, panel.axes)
  chain.step(launches[0], panel.pool_of(launches[0]))

  def broken(groups, init):
    raise _native.NativeError("the pool step failed")

  with pytest.raises(_native.NativeError, match="pool step failed"):
    chain.step(launches[1], broken)
  with pytest.raises(_native.NativeError, match="pool step failed"):
    chain.step(launches[2], panel.pool_of(launches[2]))
  assert chain._futures[0].result() is not None        # what was done before the failure stays done


# ---- the public call refuses before any device work -------------------------------------------------
def test_fit_refuses_bad_event_aggregates_before_any_device_work():
  kw = dict(names=NAMES)
  with pytest.raises(ValueError, match="event_aggregates.*shared_streams=True.*perfectly correlated.*joint posterior"):
    ci.fit_causalimpact_panel(FRAMES, PERIODS, event_aggregates={"total": "all"}, shared_streams=True, **kw)
  with pytest.raises(ValueError, match="unknown series 'nowhere'"):
    ci.fit_causalimpact_panel(FRAMES, PERIODS, event_aggregates={"g": ["nowhere"]}, **kw)
  with pytest.raises(ValueError, match="listed twice"):
    ci.fit_causalimpact_panel(FRAMES, PERIODS, event_aggregates={"g": ["c", "c"]}, **kw)
  with pytest.raises(ValueError, match="is empty"):
    ci.fit_causalimpact_panel(FRAMES, PERIODS, event_aggregates={"g": []}, **kw)
  with pytest.raises(ValueError, match="is empty"):
    ci.fit_causalimpact_panel(FRAMES, PERIODS, event_aggregates={"g": {"a": 0.0}}, **kw)
  with pytest.raises(ValueError, match="not finite"):
    ci.fit_causalimpact_panel(FRAMES, PERIODS, event_aggregates={"g": {"a": np.inf}}, **kw)
  # bad data is not looked at before the groups are: the refusal comes ahead of data preparation
  with pytest.raises(ValueError, match="unknown series 'nowhere'"):
    ci.fit_causalimpact_panel(FRAMES, [PERIODS[0]] * 3 + [((0, 1), (2, 3))],
                              event_aggregates={"g": ["nowhere"]}, **kw)


@pytest.mark.parametrize("options", [{}, dict(data_options=ci.DataOptions(dtype=np.float64))])
def test_fit_refuses_an_axis_with_too_few_pre_period_steps_and_names_the_aggregate(options):
  """d has 4 pre-period steps and b a gap of 2: their common axis keeps 2 steps in front of the gap.
  On the one-launch route and on the per-series route, before any fit."""
  frames = FRAMES[:3] + [_frame(22, 4)]
  periods = PERIODS[:3] + [((0, 3), (4, 21))]
  aggregates = {"fine": ["a", "b", "c"], "short": ["b", "d"]}
  with pytest.raises(ValueError, match="aggregate 'short': pre_period must span at least 3 time points.*Got 2"):
    ci.fit_causalimpact_panel(frames, periods, names=NAMES, event_aggregates=aggregates, **options)


# ---- the C-ABI ------------------------------------------------------------------------------------------
SYMBOL = "ci_session_pool_event_trajectories"


def test_header_binding_and_library_agree_on_the_signature():
  hdr = open(os.path.join(ROOT, "include", "causalimpact_amd.h")).read()
  hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
  m = re.search(r"\bint\s+" + SYMBOL + r"\s*\(([^)]*)\)\s*;", hdr)
  assert m, f"{SYMBOL} is not declared"
  params = [" ".join(p.split()) for p in m.group(1).split(",")]
  assert params == ["ci_session* session", "const double* scale", "const double* shift",
                    "int32_t num_groups", "const int32_t* offsets", "const int32_t* members",
                    "const double* weights", "const int32_t* first", "const int32_t* width",
                    "int32_t out_stride", "const double* init", "double* out"]
  assert SYMBOL in _native.exported_symbols()
  assert hasattr(C.CDLL(_native.LIB_PATH), SYMBOL)
  bound = getattr(_native.load(), SYMBOL).argtypes
  assert list(bound) == [C.c_void_p if "*" in p else C.c_int32 for p in params]
  assert _native.load().ci_abi_version() == 5 == _native.ABI_VERSION        # additive: no version bump
  assert re.search(r"#define\s+CI_ABI_VERSION\s+5\b", hdr)


def test_null_arguments_are_refused_before_any_device_call():
  """No session can exist without a GPU, so what is reachable here is the first check: a NULL
  session, with every other argument valid, is an error and not a crash.  (The checks behind it
  need a session: tests/test_gpu_panel_event_aggregates.py.)"""
  fn = getattr(_native.load(), SYMBOL)
  one = np.ones(1)
  off, mem = np.array([0, 1], np.int32), np.zeros(1, np.int32)
  first, width = np.zeros(1, np.int32), np.ones(1, np.int32)
  out = np.zeros(4)
  rc = fn(None, one.ctypes.data, one.ctypes.data, 1, off.ctypes.data, mem.ctypes.data, one.ctypes.data,
          first.ctypes.data, width.ctypes.data, 1, None, out.ctypes.data)
  assert rc != 0 and b"NULL argument" in _native.load().ci_last_error()
