"""Joint bands of the pooled aggregates: the host assembly (`batch._frame_analyses`,
`batch._aggregate_paths`) fed `_native.path_excursions_host` in place of the device call, on synthetic
pooled draws; the coverage the bands promise; and a pooled effect that rises and then reverses.  No GPU."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

from causalimpact import _native
from causalimpact import batch
from causalimpact import causalimpact_lib as lib
from causalimpact import data as cid

ALPHA = 0.05
PRE_STEPS, POST_STEPS, TAIL = 30, 24, 2
T = PRE_STEPS + POST_STEPS + TAIL


def _summarize_draws_host(draws, scale, shift, observed, flags, ranks, device=0):
  """ci_summarize_draws_f64 in numpy (csrc/ci_summary.h: summ_cumsum_kernel and the order statistics)."""
  v = np.asarray(draws, np.float64) * scale + shift                          # [N, T]
  obs, flags = np.asarray(observed, np.float64), np.asarray(flags)
  point = -(v - obs)
  base = np.where((flags & 1) != 0, point, 0.0)
  hole = np.isnan(base)
  cum = np.where(hole, np.nan, np.cumsum(np.where(hole, 0.0, base), axis=1))
  win = (flags & 2) != 0
  per_draw = np.stack([v[:, win].sum(axis=1), np.where(np.isnan(point), 0.0, point)[:, win].sum(axis=1)])
  rk = np.asarray(ranks, np.int64)
  return dict(value_order=np.sort(v, axis=0)[rk], cum_order=np.sort(cum, axis=0)[rk], per_draw=per_draw,
              per_draw_order=np.sort(per_draw, axis=1)[:, rk])


def _paths_host(calls):
  def fake(draws, scale, shift, observed, first, count, ranks, want=_native.PATH_OUTPUTS, device=0):
    calls.append(dict(draws=np.array(draws), observed=np.array(observed), first=np.array(first),
                      count=np.array(count), ranks=list(ranks), scale=scale, shift=shift, device=device))
    got = _native.path_excursions_host(draws, scale, shift, observed, first, count, ranks)
    return {k: got[k] for k in want}
  return fake


@pytest.fixture
def host(monkeypatch):
  """`_frame_analyses` with both device calls replaced by their numpy definitions; the recorded calls
  of `summarize_draw_paths`."""
  calls = []
  monkeypatch.setattr(_native, "summarize_draws", _summarize_draws_host)
  monkeypatch.setattr(_native, "summarize_draw_paths", _paths_host(calls))
  return calls


def _flags(width, first, count):
  tau = np.arange(width)
  return (tau >= first).astype(np.uint8) | (((tau >= first) & (tau < first + count)).astype(np.uint8) << 1)


def _row(name, index, observed, draws, n_post=POST_STEPS):
  """One row of `_frame_analyses`: the `CausalImpactData` of the pooled outcome on `index`, PRE_STEPS
  steps of pre-period and n_post of post-period (integer periods are positions into the index)."""
  pre, post = (0, PRE_STEPS - 1), (PRE_STEPS, PRE_STEPS + n_post - 1)
  if not pd.api.types.is_integer_dtype(index):
    pre, post = tuple(index[i] for i in pre), tuple(index[i] for i in post)
  ci_data = cid.CausalImpactData(pd.DataFrame({"y": observed}, index=index), pre, post, standardize_data=False)
  return (name, ci_data, observed, _flags(len(index), PRE_STEPS, n_post), draws.mean(axis=0), draws)


def _reversing(N, seed, d):
  """Pooled draws [N, T] of unit noise around 0 and an observed path that lies d sd above them over the
  first half of the post-period and d sd below over the second: the effects cancel in the total."""
  rng = np.random.default_rng(seed)
  draws = rng.normal(size=(N, T))
  observed = rng.normal(size=T)
  observed[PRE_STEPS:PRE_STEPS + POST_STEPS // 2] += d
  observed[PRE_STEPS + POST_STEPS // 2:PRE_STEPS + POST_STEPS] -= d
  return draws, observed


def test_frames_and_tables_of_groups_with_axes_of_their_own(host):
  """Three groups: two on a calendar of T steps, one on a shorter event-time axis that does not reach
  the window "late"; one device call for all of them."""
  N = 200
  index = pd.date_range("2024-01-01", periods=T, freq="D")
  post = (index[PRE_STEPS], index[PRE_STEPS + POST_STEPS - 1])
  rows = []
  for g, name in enumerate(["up", "flat"]):
    draws, observed = _reversing(N, 10 + g, 5.0 if g == 0 else 0.0)
    if g == 0:
      observed[PRE_STEPS + 3] = np.nan
    rows.append(_row(name, index, observed, draws))
  short = 44                                                       # tau = -30 .. 13
  axis = pd.Index(np.arange(-PRE_STEPS, short - PRE_STEPS), name="event_time")
  draws, observed = _reversing(N, 12, 0.0)
  rows.append(_row("short", axis, observed[:short], draws[:, :short], n_post=14))
  names = ["early", "late"]
  window = lambda name, idx, first, count: lib.EffectWindow(name, idx[first], idx[first + count - 1], first, count)   # pylint: disable=unnecessary-lambda-assignment
  early, late = window("early", index, PRE_STEPS, 8), window("late", index, PRE_STEPS + 14, 10)
  windows = (names, [[early, late], [early, late], [window("early", axis, PRE_STEPS, 8)]])
  ranks = lib._summary_ranks(N, (ALPHA / 2.0, 1.0 - ALPHA / 2.0))
  analyses, table, window_table, joint, window_joint = batch._frame_analyses(
      rows, ALPHA, ranks, 3, windows, joint_bands=True)
  # one call: draws padded with 0.0 and observations with NaN to the widest group, scale 1, shift 0
  assert len(host) == 1
  call = host[0]
  assert call["draws"].shape == (3, N, T) and call["scale"] == 1.0 and call["shift"] == 0.0 and call["device"] == 3
  assert (call["draws"][2, :, short:] == 0.0).all() and np.isnan(call["observed"][2, short:]).all()
  np.testing.assert_array_equal(call["draws"][2, :, :short], draws[:, :short])
  np.testing.assert_array_equal(call["first"], [[30, 30, 44], [30, 30, 44], [30, 30, 0]])
  np.testing.assert_array_equal(call["count"], [[24, 8, 10], [24, 8, 10], [14, 8, 0]])
  assert call["ranks"] == lib._path_ranks(N, ALPHA) and call["first"].dtype == np.int32
  # the tables
  paths = list(lib.JOINT_PATHS)
  assert list(analyses) == ["up", "flat", "short"]
  assert joint.index.names == ["aggregate", None] and window_joint.index.names == ["aggregate", "window", None]
  assert list(joint.index) == [(a, p) for a in analyses for p in paths]
  assert list(window_joint.index) == [(a, w, p) for a in analyses for w in names for p in paths]
  for frame in (joint, window_joint):
    assert list(frame.columns) == list(lib.JOINT_SUMMARY_COLUMNS)
    assert {c: str(t) for c, t in frame.dtypes.items()} == dict(
        critical_value="float64", max_excursion="float64", at="object", n_outside="Int64",
        first_outside="object", p="float64", significant="boolean")
  assert list(table.index) == [(a, r) for a in analyses for r in ("average", "cumulative")]
  assert len(window_table) == 3 * 2 * 2
  # blank rows where the group's axis does not reach the window, and nowhere else
  blank = window_joint.loc["short"].loc["late"]
  assert blank.isna().all().all() and window_table.loc["short"].loc["late"].isna().all().all()
  assert window_joint.drop(index=[("short", "late", p) for p in paths])["p"].notna().all()
  assert joint["p"].notna().all()
  # every group's own frames on its own index; the tables are their slices
  for name, row in zip(analyses, rows):
    one, idx = analyses[name], row[1].data.index
    assert tuple(one.joint_bands.columns) == lib.JOINT_BAND_COLUMNS and one.joint_bands.index.equals(idx)
    assert one.joint_bands["outside"].dtype == bool
    pd.testing.assert_frame_equal(joint.loc[name], one.joint_summary, check_exact=True)
    pd.testing.assert_frame_equal(window_joint.loc[name], one.window_joint_summary, check_exact=True)
    post_rows = (row[3] & 2) != 0
    assert one.joint_bands.loc[~post_rows].drop(columns="outside").isna().all().all()
    assert one.joint_bands.loc[post_rows, "posterior_lower"].notna().all()
  assert analyses["short"].joint_bands.index.name == "event_time"
  assert 0 <= analyses["short"].joint_summary.loc["pointwise", "at"] <= 13       # a label of ITS axis
  assert post[0] <= analyses["up"].joint_summary.loc["pointwise", "at"] <= post[1]
  # the frames are `lib._joint_frames` on the host loop of the group's own draws
  g = 0
  own = lib._paths_record(_native.path_excursions_host(rows[g][5][None], 1.0, 0.0, rows[g][2], [30, 30, 44],
                                                       [24, 8, 10], call["ranks"]))
  bands, summary, by_window = lib._joint_frames({k: v[0] for k, v in own.items()}, call["ranks"], N, ALPHA,
                                                rows[g][2], index, index, names)
  pd.testing.assert_frame_equal(analyses["up"].joint_bands, bands, check_exact=True)
  pd.testing.assert_frame_equal(analyses["up"].joint_summary, summary, check_exact=True)
  pd.testing.assert_frame_equal(analyses["up"].window_joint_summary, by_window, check_exact=True)
  # the missing observation: no cumulative band there, and not outside
  assert np.isnan(bands["cumulative_effects_lower"].iloc[PRE_STEPS + 3]) and not bands["outside"].iloc[PRE_STEPS + 3]


def test_without_joint_bands_or_windows_the_results_are_none(host):
  N = 60
  index = pd.RangeIndex(T)
  draws, observed = _reversing(N, 4, 0.0)
  rows = [_row("only", index, observed, draws)]
  ranks = lib._summary_ranks(N, (ALPHA / 2.0, 1.0 - ALPHA / 2.0))
  off = batch._frame_analyses(rows, ALPHA, ranks)
  assert len(off) == 5 and off[2] is None and off[3] is None and off[4] is None and not host
  assert off[0]["only"].joint_bands is None and off[0]["only"].joint_summary is None
  on = batch._frame_analyses(rows, ALPHA, ranks, joint_bands=True)
  assert len(host) == 1 and host[0]["first"].shape == (1, 1)
  assert on[3] is not None and on[4] is None and on[0]["only"].window_joint_summary is None
  pd.testing.assert_frame_equal(on[1], off[1], check_exact=True)
  pd.testing.assert_frame_equal(on[0]["only"].series, off[0]["only"].series, check_exact=True)

  class Result:
    pass
  res = Result()
  batch._take_aggregates(res, on)
  assert res.aggregates is on[0] and res.aggregate_joint_summary is on[3]
  assert res.aggregate_window_joint_summary is None and res.aggregate_summary is on[1]


def test_the_band_holds_whole_paths_and_significant_means_outside(host):
  """The share of the draws whose whole path lies inside the simultaneous band is at least 1 - alpha -
  1 / N (the critical value is an interpolated order statistic of the N excursions), and
  `significant` is true exactly when some step is outside."""
  N = 400
  index = pd.RangeIndex(T)
  ranks = lib._summary_ranks(N, (ALPHA / 2.0, 1.0 - ALPHA / 2.0))
  rows = []
  for g, d in enumerate([0.0, 0.0, 2.0, 3.5, 6.0]):
    draws, observed = _reversing(N, 20 + g, d)
    draws = np.cumsum(draws, axis=1) * 0.3 + draws               # (paths with dependence along time)
    rows.append(_row(f"g{g}", index, observed, draws))
  analyses, _, _, joint, _ = batch._frame_analyses(rows, ALPHA, ranks, joint_bands=True)
  post = slice(PRE_STEPS, PRE_STEPS + POST_STEPS)
  seen = set()
  for name, row in zip(analyses, rows):
    bands, draws = analyses[name].joint_bands, row[5]
    lower, upper = bands["posterior_lower"].to_numpy()[post], bands["posterior_upper"].to_numpy()[post]
    inside = ((draws[:, post] >= lower) & (draws[:, post] <= upper)).all(axis=1)
    print(f"{name}: {inside.mean():.4f} of the paths inside the band")
    assert inside.mean() >= 1.0 - ALPHA - 1.0 / N
    assert inside.mean() <= 1.0 - ALPHA + 2.0 / N                # (and it is no wider than that takes)
    for path in lib.JOINT_PATHS:
      r = joint.loc[(name, path)]
      assert bool(r["significant"]) == (r["n_outside"] > 0)
      assert (r["first_outside"] is not None) == (r["n_outside"] > 0)
      seen.add(bool(r["significant"]))
    assert int(joint.loc[(name, "pointwise"), "n_outside"]) == int(bands["outside"].sum())
  assert seen == {True, False}


def test_a_pooled_effect_that_rises_and_reverses_is_found_by_the_path_not_by_the_total(host):
  N = 200
  index = pd.RangeIndex(T)
  draws, observed = _reversing(N, 7, 5.0)
  post = slice(PRE_STEPS, PRE_STEPS + POST_STEPS)
  # near-zero total: the noise of the observations is shifted so that the window's sum is the mean
  # prediction's, and what is left of the effect is its shape alone
  observed[post] += (draws.mean(axis=0)[post].sum() - observed[post].sum()) / POST_STEPS
  rows = [_row("pooled", index, observed, draws)]
  ranks = lib._summary_ranks(N, (ALPHA / 2.0, 1.0 - ALPHA / 2.0))
  _, table, _, joint, _ = batch._frame_analyses(rows, ALPHA, ranks, joint_bands=True)
  p_total = table.loc[("pooled", "cumulative"), "p_value"]
  row = joint.loc[("pooled", "pointwise")]
  print(f"total: p = {p_total:.3f}; whole path: p = {row['p']:.4f}, {row['n_outside']} steps outside")
  assert p_total > ALPHA                                           # the total sees nothing
  lower, upper = table.loc[("pooled", "cumulative"), ["abs_effect_lower", "abs_effect_upper"]]
  assert lower < 0.0 < upper
  assert bool(row["significant"]) and row["p"] <= 1.0 / (1.0 + N) + 1e-15 and row["n_outside"] >= POST_STEPS - 2
  assert row["first_outside"] == PRE_STEPS


# ---- the entry point's checks come before any device call ---------------------------------------------
def test_binding_and_library_have_the_entry():
  assert "ci_summarize_draw_paths_f64" in _native.exported_symbols()
  assert "ci_test_summarize_draw_paths_f64" in _native.exported_symbols()
  L = _native.load()
  assert len(L.ci_summarize_draw_paths_f64.argtypes) == 20
  assert len(L.ci_test_summarize_draw_paths_f64.argtypes) == 22
  assert _native.ABI_VERSION == 5


def test_refusals_need_no_device():
  draws, obs = np.zeros((2, 5, 10)), np.zeros(10)
  call = lambda **kw: _native.summarize_draw_paths(**dict(dict(   # pylint: disable=unnecessary-lambda-assignment
      draws=draws, scale=1.0, shift=0.0, observed=obs, first=[3], count=[4], ranks=[0, 4]), **kw))
  for kw, message in [
      (dict(shift=[1.0, np.inf]), "the shift of group 1 is not finite"),
      (dict(scale=[np.nan, 1.0]), "the scale of group 0 is not finite"),
      (dict(draws=np.zeros((2, 1, 10)), ranks=[0]), r"num_draws must be >= 2, got 1"),
      (dict(count=[8]), r"window 0 of group 0: steps 3 .. 10 end beyond the draws' 10 steps"),
      (dict(first=[[3, 1], [3, -1]], count=[[4, 1], [4, 1]]), r"window 1 of group 1: first step -1 is negative"),
      (dict(first=[0] * 65, count=[1] * 65), r"num_windows must be in \[1, 64\], got 65"),
      (dict(ranks=[0, 5]), r"rank 5 out of range \[0, 5\)"),
      (dict(ranks=list(range(5)) * 2), r"num_ranks must be in \[1, 8\], got 10"),
      (dict(max_bytes=500), r"window 0 of group 0: its 4 steps of 5 draws and the group's own draws take "
                            r"1088 bytes of device memory beside 264 of tables, the limit is 500"),
      (dict(max_bytes=100), r"the tables alone take 264 bytes"),
  ]:
    with pytest.raises(_native.NativeError, match=message):
      call(**kw)
  L = _native.load()
  one = np.ones(2)
  i32 = np.array([0, 0], np.int32)
  rc = L.ci_summarize_draw_paths_f64(0, 0, 5, 10, draws.ctypes.data, one.ctypes.data, one.ctypes.data,
                                     obs.ctypes.data, 1, i32.ctypes.data, i32.ctypes.data, 1, i32.ctypes.data,
                                     *[None] * 7)
  assert rc != 0 and b"num_groups must be >= 1, got 0" in L.ci_last_error()
  rc = L.ci_summarize_draw_paths_f64(0, 2, 5, 10, None, one.ctypes.data, one.ctypes.data, obs.ctypes.data, 1,
                                     i32.ctypes.data, i32.ctypes.data, 1, i32.ctypes.data, *[None] * 7)
  assert rc != 0 and b"NULL argument" in L.ci_last_error()
  chunks = C.c_int32(-1)
  rc = L.ci_test_summarize_draw_paths_f64(0, 2, 5, 10, draws.ctypes.data, one.ctypes.data, one.ctypes.data,
                                          obs.ctypes.data, 0, i32.ctypes.data, i32.ctypes.data, 1,
                                          i32.ctypes.data, *[None] * 7, 1 << 30, C.addressof(chunks))
  assert rc != 0 and b"num_windows must be in [1, 64], got 0" in L.ci_last_error() and chunks.value == -1
