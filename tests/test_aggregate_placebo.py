"""Placebo forecasts of pooled effects without a GPU: the host twin (`_native.pool_placebo_host`,
`_native.finish_placebo_host`) against plain loops, a group of one member against that member's own
placebo columns, the origin plans of event-time aggregates, and the fit functions on the route that
pools everything on the host, with the sampler replaced by random draws."""
import math

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _model
from causalimpact import _native
from causalimpact import batch
from causalimpact import causalimpact_lib as lib

from test_aggregate_joint_bands import _summarize_draws_host
from test_placebo import _fake_float64_fit, _frame

ALPHA = 0.1


# ---- the host twin ---------------------------------------------------------------------------------

def _loop(s, v, offsets, weights, init=None):
  """S and U by the loop of include/causalimpact_amd.h, one scalar at a time."""
  G, (K, O, N) = len(offsets) - 1, s.shape
  out = np.zeros((G, O, 2, N)) if init is None else np.array(init, np.float64)
  for g in range(G):
    for i in range(O):
      for n in range(N):
        S, U = out[g, i, 0, n], out[g, i, 1, n]
        for k in range(offsets[g], offsets[g + 1]):
          S = S + weights[k] * s[k, i, n]
          U = U + (weights[k] * weights[k]) * v[k, i, n]
        out[g, i, 0, n], out[g, i, 1, n] = S, U
  return out


@pytest.mark.parametrize("groups", [[{0: 1.0, 1: 0.5, 2: -2.0}],
                                    [{0: 1.0, 2: 0.3}, {1: 0.7, 2: 1.1, 3: 0.25}, {0: 3.0}],
                                    [{1: 1.5}, {}, {0: 1.0, 3: 0.1}]],
                         ids=["single", "overlapping", "empty"])
def test_host_pool_is_the_plain_loop_and_init_continues_it_bit_for_bit(groups):
  rng = np.random.default_rng(3)
  csr = _native.groups_csr(groups, 4)
  K = int(csr[0][-1])
  s, v = rng.normal(size=(K, 3, 5)) * 50.0, rng.uniform(0.1, 9.0, (K, 3, 5))
  got = _native.pool_placebo_host(s, v, csr)
  np.testing.assert_array_equal(got, _loop(s, v, csr[0], csr[2]))
  np.testing.assert_array_equal(got, _native.pool_placebo_host(s, v, groups))      # (the groups themselves)
  if groups[1:] and not groups[1]:
    assert (got[1] == 0.0).all()
  # the entries of every group cut in two: the second call continues the first through `init`
  halves = [[], []]
  keep = [[], []]
  for g, group in enumerate(groups):
    items = sorted(group.items())
    cut = (len(items) + 1) // 2
    for h, part in enumerate((items[:cut], items[cut:])):
      halves[h].append(dict(part))
      keep[h] += [int(csr[0][g]) + (0 if h == 0 else cut) + j for j in range(len(part))]
  first = _native.pool_placebo_host(s[keep[0]], v[keep[0]], halves[0])
  np.testing.assert_array_equal(_native.pool_placebo_host(s[keep[1]], v[keep[1]], halves[1], init=first), got)
  with pytest.raises(ValueError, match="entries"):
    _native.pool_placebo_host(s[:-1], v[:-1], csr)


def test_finish_is_the_normal_of_the_pooled_sum_and_reads_zero_without_a_counted_step():
  rng = np.random.default_rng(4)
  acc = np.stack([rng.normal(size=(2, 3, 6)) * 10.0, rng.uniform(0.5, 4.0, (2, 3, 6))], axis=2)
  acc[1, 2] = 0.0                                                # a slot no member counts a step in
  seen = rng.normal(size=(2, 3)) * 10.0
  seen[1, 2] = np.nan
  got = _native.finish_placebo_host(acc, seen)
  for g in range(2):
    for i in range(3):
      S, U, e = acc[g, i, 0], acc[g, i, 1], seen[g, i] - acc[g, i, 0]
      if g == 1 and i == 2:
        assert all(got[k][g, i] == 0.0 for k in got)
        continue
      pit = [0.5 * math.erfc(-x / math.sqrt(2.0 * u)) for x, u in zip(e, U)]
      np.testing.assert_allclose(got["predicted_mean"][g, i], S.mean(), rtol=1e-14)
      np.testing.assert_allclose(got["spread_mean"][g, i], (U + e * e).mean(), rtol=1e-14)
      np.testing.assert_allclose(got["pit_mean"][g, i], np.mean(pit), rtol=1e-14)


# ---- a group of one member ---------------------------------------------------------------------------

def _member(T=70, P=2, N=24, seed=8):
  """One series as its sampler saw it, random parameter draws and its data-scale outcome."""
  rng = np.random.default_rng(seed)
  X = np.column_stack([rng.normal(size=(T, P - 1)), np.ones(T)])
  y = 0.4 * X[:, 0] + np.cumsum(rng.normal(scale=0.1, size=T)) + rng.normal(scale=0.4, size=T)
  mask = np.zeros(T, bool)
  mask[[11, 12, 40]] = True
  mask[50:] = True
  spec = _model.series_params(np.where(mask, np.nan, y), mask, X, has_slope=True, num_seasonal_blocks=0)
  draws = dict(observation_noise_scale=rng.uniform(0.3, 0.6, N), level_scale=rng.uniform(0.02, 0.1, N),
               slope_scale=rng.uniform(0.001, 0.01, N), seasonal_drift_scales=np.zeros((N, 0)),
               weights=rng.normal(scale=0.2, size=(N, P)))
  one = lib.SeriesInputs(y, mask, X, np.zeros((0, T), np.uint8), (), True, spec)
  scale, shift = 3.7, -12.25
  return one, draws, scale, shift, np.where(mask, np.nan, y * scale + shift)


def test_a_group_of_one_member_has_that_members_own_columns_and_a_weight_scales_them():
  one, draws, scale, shift, observed = _member()
  origins, H = np.array([3, 4, 11, 35, 41, -1, -1]), 9
  own = lib._placebo_summary_host(*one.filter_inputs(), draws, scale, shift, origins, H)
  cnt, seen = lib._placebo_seen(one.outcome(), one.mask, origins, H, scale, shift)
  want = lib._placebo_columns(dict(own, n_counted=cnt, seen_sum=seen), origins, H, ALPHA, observed)
  entry = lib._placebo_entry_host(one, draws, scale, shift, observed, origins, H)
  np.testing.assert_array_equal(entry["n_counted"], cnt)
  labels = pd.RangeIndex(70)
  frames = {}
  for w in (1.0, 2.0):
    acc = _native.pool_placebo_host(entry["s"][None], entry["v"][None], [{0: w}])
    means = _native.finish_placebo_host(acc, w * entry["seen_sum"][None])
    psum = dict({k: v[0] for k, v in means.items()}, n_counted=cnt, seen_sum=w * entry["seen_sum"])
    frames[w], quality = lib._aggregate_placebo_frames(psum, w * entry["actual"], origins, H, ALPHA, labels, H, 0.05)
    assert list(frames[w].columns) == list(lib.PLACEBO_COLUMNS) and list(frames[w].index) == [3, 4, 11, 35, 41]
    assert list(quality.index) == list(lib.PLACEBO_QUALITY_ENTRIES) and quality["n_origins"] == 5
  got = frames[1.0]
  np.testing.assert_array_equal(got["predicted"], want["predicted"])
  assert list(got["horizon_end"]) == list(want["horizon_end_step"])
  assert list(got["significant"]) == list(want["significant"])
  for k in ("n_counted", "actual", "predicted_sd", "effect", "relative_effect", "pit", "p"):
    np.testing.assert_allclose(got[k], want[k], rtol=1e-12, err_msg=k)
  twice = frames[2.0]
  for k in ("predicted", "predicted_sd", "effect", "actual"):
    np.testing.assert_allclose(twice[k], 2.0 * got[k], rtol=1e-12, err_msg=k)
  np.testing.assert_allclose(twice["pit"], got["pit"], rtol=0, atol=1e-12)
  np.testing.assert_array_equal(twice["n_counted"], got["n_counted"])


# ---- the origin plans of event-time aggregates -------------------------------------------------------

def test_event_time_origins_stay_inside_every_members_own_pre_period():
  csr = _native.groups_csr([{0: 1.0, 1: 0.5, 2: 1.0}, {0: 1.0, 2: 2.0}, {1: 1.0}], 3)
  # three members with 60, 33 and 48 pre-period steps (and gaps 0, 2, 1 before the treatment start)
  pre, start = np.array([60, 33, 48]), np.array([60, 35, 49])
  axes = []
  for g in range(3):
    m = csr[1][csr[0][g]:csr[0][g + 1]]
    L = int(start[m].min())
    axes.append(batch.EventAxis(L=L, gap=int((start - pre)[m].max()), Hwin=[12, 20, 40][g], H=25,
                                first=(start[m] - L).astype(np.int32)))
  plan = batch.EventPlan(["all", "long", "short"], csr, axes, [None] * 3, [None] * 3)
  pp = batch.event_placebo_pool_plan(ci.Placebo(max_origins=5), plan, 1)
  assert pp.origins.shape == (6, 5) and pp.columns.shape == (3, 5)
  for g, axis in enumerate(axes):
    H, cols = lib.placebo_plan(ci.Placebo(max_origins=5), axis.L - axis.gap, axis.Hwin, 1)
    assert pp.horizon[g] == H and list(pp.columns[g, :len(cols)]) == list(cols) and (pp.columns[g, len(cols):] == -1).all()
    assert pp.labels[g].equals(axis.index) and pp.n_post[g] == axis.Hwin
    for k, first in zip(range(csr[0][g], csr[0][g + 1]), axis.first):
      used = pp.origins[k][pp.origins[k] >= 0]
      np.testing.assert_array_equal(used, np.asarray(cols) + first)
      assert len(used) == 0 or used.max() + H <= pre[csr[1][k]]           # inside the member's own pre-period
  # "short": 33 pre-period steps, H = min(40, 33 // 3) = 11, 12 admissible origins, 5 taken
  assert pp.horizon[2] == 11 and (pp.columns[2] >= 0).sum() == 5
  # a group without room: its only member's pre-period is shorter than twice the horizon asked for
  none = batch.event_placebo_pool_plan(ci.Placebo(horizon=20), plan, 1)
  assert (none.columns[2] == -1).all() and (none.origins[5] == -1).all()
  assert (none.columns[1] >= 0).any() and [g for g, _ in none.entries_of(0)] == [1]    # ("all" has 33 steps too)
  assert none.entries_of(1) == []
  frame, quality = lib._aggregate_placebo_frames(None, np.zeros(1), none.columns[2], 20, ALPHA, axes[2].index, 40, 0.1)
  assert len(frame) == 0 and list(frame.columns) == list(lib.PLACEBO_COLUMNS)
  assert quality["n_origins"] == 0 and quality["horizon"] == 20 and np.isnan(quality["false_positive_rate"])


# ---- the fit functions, on the route that pools on the host ------------------------------------------

@pytest.fixture
def host_fit(monkeypatch):
  _fake_float64_fit(monkeypatch)
  monkeypatch.setattr(_native, "summarize_draws", _summarize_draws_host)


KW = dict(data_options=ci.DataOptions(dtype=np.float64), seed=1, alpha=ALPHA,
          inference_options=ci.InferenceOptions(num_results=8, summarize_on_device=False))


def _same_but_the_aggregates_placebo(on, off, names):
  pd.testing.assert_frame_equal(on.summary, off.summary, check_exact=True)
  pd.testing.assert_frame_equal(on.aggregate_summary, off.aggregate_summary, check_exact=True)
  pd.testing.assert_frame_equal(on.placebo_quality, off.placebo_quality, check_exact=True)
  for b in range(len(on)):
    pd.testing.assert_frame_equal(on[b].series, off[b].series, check_exact=True)
    pd.testing.assert_frame_equal(on[b].placebo, off[b].placebo, check_exact=True)
  for name in names:
    pd.testing.assert_frame_equal(on.aggregates[name].series, off.aggregates[name].series, check_exact=True)
    pd.testing.assert_frame_equal(on.aggregates[name].summary, off.aggregates[name].summary, check_exact=True)


def test_batch_on_the_host_route_fills_the_aggregates_placebo(host_fit, monkeypatch):   # pylint: disable=unused-argument
  frames = [_frame(70, seed) for seed in (0, 1, 2)]
  idx = frames[0].index
  periods = ((idx[0], idx[48]), (idx[50], idx[64]))           # 49 and 15 steps: H = 15
  aggregates = {"all": "all", "pair": {0: 1.0, 2: 0.5}}
  placebo = ci.Placebo(max_origins=5)
  got = ci.fit_causalimpact_batch(frames, *periods, aggregates=aggregates, placebo=placebo, **KW)
  assert type(got) is batch.PerSeriesBatchAnalysis
  quality = got.aggregate_placebo_quality
  assert list(quality.index) == ["all", "pair"] and list(quality.columns) == list(lib.PLACEBO_QUALITY_ENTRIES)
  own = got[0].placebo
  for name, members in (("all", {0: 1.0, 1: 1.0, 2: 1.0}), ("pair", {0: 1.0, 2: 0.5})):
    one = got.aggregates[name]
    assert list(one.placebo.columns) == list(lib.PLACEBO_COLUMNS)
    assert one.placebo.index.equals(own.index) and list(one.placebo["horizon_end"]) == list(own["horizon_end"])
    pd.testing.assert_series_equal(one.placebo_quality, quality.loc[name], check_names=False)
    for column, weight in (("actual", lambda w: w), ("n_counted", lambda w: 1.0)):
      want = sum(weight(w) * got[b].placebo[column].to_numpy() for b, w in members.items())
      np.testing.assert_allclose(one.placebo[column], want, rtol=1e-12)
    # the pooled forecast is the weighted sum of the members' forecasts; its variance adds theirs
    want = sum(w * got[b].placebo["predicted"].to_numpy() for b, w in members.items())
    np.testing.assert_allclose(one.placebo["predicted"], want, rtol=1e-10)
    assert ((one.placebo["pit"] > 0) & (one.placebo["pit"] < 1)).all() and (one.placebo["predicted_sd"] > 0).all()
    assert quality.loc[name, "n_origins"] == 5 and quality.loc[name, "horizon"] == 15
    rel = np.abs(one.placebo["relative_effect"].to_numpy())
    fit_rel = abs(one.summary.loc["cumulative", "rel_effect"])
    assert quality.loc[name, "empirical_p"] == (1 + np.count_nonzero(rel >= fit_rel)) / 6
  # without `placebo=` nothing is there; with it nothing else differs
  bare = ci.fit_causalimpact_batch(frames, *periods, aggregates=aggregates, **KW)
  assert bare.aggregate_placebo_quality is None and bare.aggregates["all"].placebo is None
  assert bare.aggregates["all"].placebo_quality is None
  assert ci.fit_causalimpact_batch(frames, *periods, placebo=placebo, **KW).aggregate_placebo_quality is None
  monkeypatch.setattr(batch, "_take_aggregate_placebo", lambda *a, **k: None)
  off = ci.fit_causalimpact_batch(frames, *periods, aggregates=aggregates, placebo=placebo, **KW)
  assert off.aggregates["all"].placebo is None
  _same_but_the_aggregates_placebo(got, off, list(aggregates))


def test_panel_on_the_host_route_indexes_the_frames_by_event_time(host_fit):   # pylint: disable=unused-argument
  frames = [_frame(T, seed) for seed, T in enumerate((70, 41, 64))]
  cut = lambda f, a, b, c: ((f.index[0], f.index[a]), (f.index[b], f.index[c]))   # pylint: disable=unnecessary-lambda-assignment
  periods = [cut(frames[0], 48, 50, 66), cut(frames[1], 29, 30, 40), cut(frames[2], 44, 45, 63)]
  got = ci.fit_causalimpact_panel(frames, periods, event_aggregates={"all": "all", "late": [0, 2]},
                                  placebo=ci.Placebo(max_origins=5), **KW)
  quality = got.aggregate_placebo_quality
  assert list(quality.index) == ["all", "late"]
  # "all": L = 30 and series 0's gap of one step leave 29 pre-period steps, the shortest window has 11:
  # H = min(11, 29 // 3) = 9; "late": L = 45, 44 pre-period steps, window 17: H = min(17, 44 // 3) = 14
  for name, horizon in (("all", 9), ("late", 14)):
    frame = got.aggregates[name].placebo
    assert frame.index.name == "origin" and quality.loc[name, "horizon"] == horizon
    assert (frame.index < 0).all() and (np.asarray(frame["horizon_end"]) < 0).all()   # event time: before the start
    assert list(np.asarray(frame["horizon_end"]) - np.asarray(frame.index)) == [horizon - 1] * len(frame)
    assert len(frame) == 5 and (frame["n_counted"] > 0).all()
    assert ((frame["pit"] > 0) & (frame["pit"] < 1)).all()
