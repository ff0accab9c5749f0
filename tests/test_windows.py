"""`effect_windows` without a GPU: the host definition of the window totals against a triple loop
written here, how labels and event-time bounds become (first, count), every refusal, the table
against `summary_table` on the post-period, and the two helpers."""
import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _native
from causalimpact import batch
from causalimpact import causalimpact_lib as lib
from causalimpact import data as cid


def _triple_loop(tr, scale, shift, observed, first, count):
  B, N, _ = tr.shape
  W = first.shape[1]
  out = np.zeros((B, W, 2, N), np.float64)
  for b in range(B):
    for w in range(W):
      for n in range(N):
        pred_sum, point_sum = np.float64(0.0), np.float64(0.0)
        for t in range(first[b, w], first[b, w] + count[b, w]):
          v = np.float64(tr[b, n, t]) * np.float64(scale[b]) + np.float64(shift[b])
          pred_sum = pred_sum + v
          point = -(v - observed[b, t])
          if point == point:
            point_sum = point_sum + point
        out[b, w, 0, n], out[b, w, 1, n] = pred_sum, point_sum
  return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_window_totals_host_equals_a_triple_loop_bit_for_bit(dtype):
  rng = np.random.default_rng(3)
  B, N, T = 3, 11, 23
  tr = rng.normal(size=(B, N, T)).astype(dtype)
  scale, shift = np.array([3.7, -0.5, 1e-3]), np.array([-12.25, 4.0, 1e3])
  observed = rng.normal(size=(B, T)) * 5.0
  observed[0, 9] = observed[1, 4] = observed[2, 22] = np.nan
  first = np.array([[5, 9, 0, 22, 7], [0, 4, 3, 10, 23], [1, 22, 20, 5, 0]])
  count = np.array([[18, 1, 23, 1, 0], [5, 1, 9, 13, 0], [3, 1, 3, 0, 23]])
  got = _native.window_totals_host(tr, scale, shift, observed, first, count)
  assert got.dtype == np.float64 and got.shape == (B, 5, 2, N)
  np.testing.assert_array_equal(got, _triple_loop(tr, scale, shift, observed, first, count))
  assert (got[0, 4] == 0.0).all() and (got[2, 3] == 0.0).all() and not np.isnan(got).any()
  # shared windows and scalar scale / shift broadcast over the series
  one = _native.window_totals_host(tr, 2.0, 1.0, observed[0], first[0], count[0])
  np.testing.assert_array_equal(one, _triple_loop(tr, [2.0] * B, [1.0] * B, np.tile(observed[0], (B, 1)),
                                                  np.tile(first[0], (B, 1)), np.tile(count[0], (B, 1))))
  with pytest.raises(ValueError, match="window 1 of series 0"):
    _native.window_totals_host(tr, 1.0, 0.0, observed, [0, 20], [3, 4])


def _batch_values(B=3, T=40, seed=0):
  rng = np.random.default_rng(seed)
  return 10.0 + rng.normal(size=(B, T, 2)).cumsum(axis=1)


def test_labels_of_a_prepared_batch_become_first_and_count():
  idx = pd.date_range("2024-01-01", periods=40, freq="D")
  # a row before the pre-period (dropped from the model), a gap of two rows, a tail of three
  prep = batch.prepare_batch(_batch_values(), idx, (idx[1], idx[24]), (idx[27], idx[36]))
  plan = batch.batch_windows({"all": (idx[27], idx[36]), "w1": ("2024-01-28", "2024-01-31"),
                              "pos": (33, 36), "one": (idx[30], idx[30])}, prep)
  assert plan.names == ["all", "w1", "pos", "one"]
  # model step = row - 1; integers are positions into the index, as for post_period
  np.testing.assert_array_equal(plan.first, np.tile([26, 26, 32, 29], (3, 1)))
  np.testing.assert_array_equal(plan.count, np.tile([10, 4, 4, 1], (3, 1)))
  assert plan.first.dtype == plan.count.dtype == np.int32
  win = np.flatnonzero(prep.flags & 2)
  assert plan.first[0, 0] == win[0] and plan.count[0, 0] == win.size


def _panel():
  frames, periods = [], []
  for b, (T, n_post) in enumerate([(60, 30), (45, 10), (52, 30)]):
    idx = pd.date_range("2023-05-01", periods=T, freq="D") + pd.Timedelta(days=3 * b)
    frames.append(pd.DataFrame(_batch_values(1, T, 5 + b)[0], index=idx, columns=["y", "x"]))
    start = T - n_post - b                                 # b rows of tail behind the post-period
    periods.append(((idx[b], idx[start - 2]), (idx[start], idx[start + n_post - 1])))
  return frames, periods


def test_event_time_bounds_of_a_prepared_panel_become_first_and_count():
  frames, periods = _panel()
  prep = batch.prepare_panel(frames, periods)
  plan = batch.panel_windows({"w1": (0, 6), "w2": (7, 13), "all": (0, 29), "tip": (9, 9)}, prep)
  assert plan.names == ["w1", "w2", "all", "tip"] and plan.windows == [(0, 6), (7, 13), (0, 29), (9, 9)]
  start = [int(np.flatnonzero(prep.flags[b] & 1)[0]) for b in range(3)]
  assert start == [30 - 0, 35 - 1 - 1, 22 - 2 - 2]         # the series' own rows before the pre-period dropped
  np.testing.assert_array_equal(plan.first, [[30, 37, 30, 39], [33, 0, 0, 42], [18, 25, 18, 27]])
  np.testing.assert_array_equal(plan.count, [[7, 7, 30, 1], [7, 0, 0, 1], [7, 7, 30, 1]])
  for b in range(3):                                       # every covered window lies in the series' own window
    for w in range(4):
      steps = np.arange(plan.first[b, w], plan.first[b, w] + plan.count[b, w])
      assert ((prep.flags[b, steps] & 2) != 0).all()


def test_every_refusal_names_the_window_and_comes_before_any_fit():
  idx = pd.date_range("2024-01-01", periods=40, freq="D")
  values = _batch_values()
  frame = pd.DataFrame(values[0], index=idx, columns=["y", "x"])
  pre, post = (idx[1], idx[24]), (idx[27], idx[36])
  sparse = frame.drop(index=[idx[30], idx[31]])             # two days without a row inside the post-period
  cases = [
      (frame, {"early": (idx[26], idx[30])}, r"effect window 'early'.*leaves the post-period"),
      (frame, {"ok": (idx[27], idx[30]), "late": (idx[30], idx[37])}, r"effect window 'late'.*leaves the post-period"),
      (frame, {"pre": (idx[3], idx[5])}, r"effect window 'pre'.*leaves the post-period"),
      (sparse, {"hole": (idx[30], idx[31])}, r"effect window 'hole'.*contains no row"),
      (frame, {"rev": (idx[33], idx[30])}, r"effect window 'rev'.*Period end must be after period start"),
      (frame, {"three": (idx[28], idx[29], idx[30])}, r"effect window 'three'.*expected \(start, end\)"),
      (frame, {"typed": (1.5, idx[30])}, r"effect window 'typed'.*Expected argument to be str, int, or datetime"),
      (frame, [("w", (idx[28], idx[29]))], "must be a mapping"),
      (frame, {}, "is empty"),
  ]
  for data, windows, msg in cases:
    with pytest.raises(ValueError, match=msg):
      ci.fit_causalimpact(data, pre, post, effect_windows=windows)
  for _, windows, msg in cases[:3] + cases[4:]:
    with pytest.raises(ValueError, match=msg):
      ci.fit_causalimpact_batch(values, pre, post, index=idx, effect_windows=windows)
  # ... the per-series routes of a batch too (float64 compute)
  with pytest.raises(ValueError, match=r"effect window 'early'"):
    ci.fit_causalimpact_batch(values, pre, post, index=idx, effect_windows=cases[0][1],
                              data_options=ci.DataOptions(dtype=np.float64))
  frames, periods = _panel()
  for windows, msg in [
      ({"neg": (-1, 3)}, r"effect window 'neg'.*0 <= tau_first <= tau_last"),
      ({"rev": (5, 3)}, r"effect window 'rev'.*0 <= tau_first <= tau_last"),
      ({"label": ("2023-06-01", "2023-06-03")}, r"effect window 'label'.*integers in event time"),
      ({"ok": (0, 6), "long": (0, 30)}, r"effect window 'long'.*no series has a post-period of 31 rows"),
      ({"one": (3,)}, r"effect window 'one'.*expected \(start, end\)"),
  ]:
    with pytest.raises(ValueError, match=msg):
      ci.fit_causalimpact_panel(frames, periods, effect_windows=windows)
    with pytest.raises(ValueError, match=msg):               # ... and on the per-series route
      ci.fit_causalimpact_panel(frames, periods, effect_windows=windows,
                                data_options=ci.DataOptions(standardize_data=False))


def test_the_table_of_the_post_period_equals_summary_table_exactly():
  """Synthetic totals per draw: the window equal to the post-period gives the batch's `summary`,
  every other window its own statistics, an uncovered window NaN rows."""
  rng = np.random.default_rng(11)
  idx = pd.RangeIndex(40)
  prep = batch.prepare_batch(_batch_values(), idx, (1, 24), (27, 36))
  B, N, T = 3, 60, prep.y.shape[1]
  prep.observed[1, 30] = np.nan                              # a missing observation inside the post-period
  tr = rng.normal(size=(B, N, T)).astype(np.float32)
  means = tr.mean(axis=1)
  ranks = lib._summary_ranks(N, (0.05, 0.95))               # pylint: disable=protected-access
  win = np.flatnonzero(prep.flags & 2)
  post = _native.window_totals_host(tr, prep.outcome_sd, prep.outcome_mean, prep.observed, [win[0]], [win.size])
  dsum = dict(per_draw=post[:, 0], per_draw_order=np.sort(post[:, 0], axis=-1)[..., ranks])
  res = batch.CausalImpactBatchAnalysis(prep, ["a", "b", "c"], 0.1, means, dsum, ranks, ["y", "x"], None)
  plan = batch.batch_windows({"all": (27, 36), "head": (27, 30), "tail": (31, 36)}, prep)
  plan.count[2, 1] = 0                                       # (as a panel's series that does not cover it)
  wsum = dict(per_draw=_native.window_totals_host(tr, prep.outcome_sd, prep.outcome_mean, prep.observed,
                                                  plan.first, plan.count))
  table = batch._window_summary(res, plan, wsum)             # pylint: disable=protected-access
  assert table.index.names == ["series", "window", None] and list(table.columns) == list(res.summary.columns)
  assert len(table) == 3 * 3 * 2
  pd.testing.assert_frame_equal(table.xs("all", level="window"), res.summary, check_exact=True)
  # with the order statistics handed in (the device's per_draw_order) nothing changes
  wsum["per_draw_order"] = np.sort(wsum["per_draw"], axis=-1)[..., ranks]
  pd.testing.assert_frame_equal(batch._window_summary(res, plan, wsum), table, check_exact=True)   # pylint: disable=protected-access
  assert table.loc[("c", "head")].isna().all().all() and not table.drop(index=("c", "head")).isna().any().any()
  # head + tail partition the post-period: the cumulative rows add up, to the bound of re-associating
  # a float64 sum of n terms, n * 2^-52 * sum |terms|
  post_mean = means.astype(np.float64) * prep.outcome_sd[:, None] + prep.outcome_mean[:, None]
  for b, name in enumerate(("a", "b")):
    parts = table.loc[(name, "head", "cumulative")] + table.loc[(name, "tail", "cumulative")]
    whole = table.loc[(name, "all", "cumulative")]
    for col, terms in (("actual", prep.observed[b, win]), ("predicted", post_mean[b, win])):
      assert abs(parts[col] - whole[col]) <= win.size * 2.0 ** -52 * np.nansum(np.abs(terms)), col
  # ... and the slice of a series is what its analysis carries
  res.window_summary = table
  assert res._window_slice(1).index.names == ["window", None]   # pylint: disable=protected-access
  pd.testing.assert_frame_equal(res._window_slice(1), table.xs("b", level="series"), check_exact=True)   # pylint: disable=protected-access


def test_the_host_route_of_a_single_fit_reproduces_its_summary_on_the_post_period():
  """`_compute_impact` with windows: the generalised `window()` of `_compute_summary`."""
  rng = np.random.default_rng(5)
  idx = pd.date_range("2024-01-01", periods=40, freq="D")
  frame = pd.DataFrame(_batch_values()[0], index=idx, columns=["y", "x"])
  frame.iloc[31, 0] = np.nan
  data = cid.CausalImpactData(frame, (idx[1], idx[24]), (idx[27], idx[36]))
  model_idx = lib.posterior_processing.model_index(data)
  tr = rng.normal(size=(50, len(model_idx))).astype(np.float32)
  windows = lib.resolve_windows({"all": (idx[27], idx[36]), "head": (idx[27], idx[30])}, data.data.index,
                                model_idx, data.post_period)
  assert [(w.first, w.count) for w in windows] == [(26, 10), (26, 4)]
  series, summary, table = lib._compute_impact(tr.mean(axis=0), tr, data, 0.1, windows=windows)   # pylint: disable=protected-access
  plain = lib._compute_impact(tr.mean(axis=0), tr, data, 0.1)                                      # pylint: disable=protected-access
  assert len(plain) == 2
  pd.testing.assert_frame_equal(plain[1], summary, check_exact=True)
  pd.testing.assert_frame_equal(plain[0], series, check_exact=True)
  assert table.index.names == ["window", None] and list(table.columns) == list(summary.columns)
  pd.testing.assert_frame_equal(table.loc["all"], summary, check_exact=True)
  head = table.loc["head"]
  assert head.loc["cumulative", "actual"] == np.nansum(frame["y"].to_numpy()[27:31])
  assert head.loc["average", "actual"] == np.nanmean(frame["y"].to_numpy()[27:31])
  # the totals of `window_totals_host` feed the device route's table: the same numbers
  rq = lib._device_summary_request(data, 0.1)                # pylint: disable=protected-access
  totals = _native.window_totals_host(tr[None], rq["scale"], rq["shift"], rq["observed"], [26], [4])[0, 0]
  want = lib._summary_rows(                                   # pylint: disable=protected-access
      np.zeros(4), frame["y"].to_numpy()[27:31], totals[0] / 4, totals[0], totals[1] / 4, totals[1], (0.05, 0.95))[0]
  np.testing.assert_allclose(head.loc["cumulative", "predicted_lower"], want["predicted_lower"][1], rtol=1e-12)
  np.testing.assert_allclose(head.loc["average", "abs_effect_upper"], want["abs_effect_upper"][0], rtol=1e-12)


def test_the_default_adds_nothing():
  one = lib.CausalImpactAnalysis(pd.DataFrame(), pd.DataFrame(), None)
  assert one.window_summary is None
  assert batch.PerSeriesBatchAnalysis(["a"], 0.05, [lib.CausalImpactAnalysis(
      pd.DataFrame(), pd.DataFrame({"actual": [1.0]}), None)]).window_summary is None


def test_calendar_windows_clip_the_periods_to_the_post_period():
  idx = pd.date_range("2024-01-01", periods=60, freq="D")   # 2024-01-01 is a Monday
  got = ci.calendar_windows(idx, ("2024-02-07", "2024-02-25"), "W")   # starts on a Wednesday
  ts = pd.Timestamp
  assert got == {"2024-02-05/2024-02-11": (ts("2024-02-07"), ts("2024-02-11")),
                 "2024-02-12/2024-02-18": (ts("2024-02-12"), ts("2024-02-18")),
                 "2024-02-19/2024-02-25": (ts("2024-02-19"), ts("2024-02-25"))}
  # positions work as for post_period, the end is clipped too, and months are periods like any other
  got = ci.calendar_windows(idx, (37, 58), "M")
  assert got == {"2024-02": (ts("2024-02-07"), ts("2024-02-28"))}
  # the windows resolve against a fit's data: a partition of the post-period
  frame = pd.DataFrame(_batch_values(1, 60)[0], index=idx, columns=["y", "x"])
  data = cid.CausalImpactData(frame, (idx[0], idx[30]), ("2024-02-07", "2024-02-25"))
  wins = lib.resolve_windows(ci.calendar_windows(idx, ("2024-02-07", "2024-02-25"), "W"), idx,
                             lib.posterior_processing.model_index(data), data.post_period)
  assert [(w.first, w.count) for w in wins] == [(37, 5), (42, 7), (49, 7)]


def test_event_windows():
  assert ci.event_windows(7, 3) == {"0..6": (0, 6), "7..13": (7, 13), "14..20": (14, 20)}
  assert ci.event_windows(1, 2) == {"0..0": (0, 0), "1..1": (1, 1)}
  with pytest.raises(ValueError):
    ci.event_windows(0, 2)
