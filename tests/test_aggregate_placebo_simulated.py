"""The simulated placebo forecasts of pooled effects (`Placebo(simulate=True, pool=True)` with
`aggregates=` / `event_aggregates=`) without a device: the option and its refusals, the declarations
of the three C entries, the numpy twins of the accumulate and of the finishing step, the frames of a
pooled group from a simulated summary, and `HostPlaceboPool` in simulated mode through the route that
fits series by series."""
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

from test_aggregate_joint_bands import _summarize_draws_host
from test_placebo import _fake_float64_fit
from test_placebo_simulated import _frame, _level_draws, _level_series, PARAMS

POOL = ci.Placebo(max_origins=5, simulate=True, pool=True)
SIM = ci.Placebo(max_origins=5, simulate=True)
ALPHA = 0.1
KW = dict(data_options=ci.DataOptions(dtype=np.float64), seed=(0, 1), alpha=ALPHA,
          inference_options=ci.InferenceOptions(num_results=8, num_chains=2, summarize_on_device=False))


# ---- the option ---------------------------------------------------------------------------------------

def test_the_option_and_every_refusal_arrive_before_any_fit(monkeypatch):
  def no_fit(*a, **k):
    raise AssertionError("the sampler was reached")
  monkeypatch.setattr(lib, "_run_sampler", no_fit)
  monkeypatch.setattr(batch, "_assemble", no_fit)
  df = _frame().reset_index(drop=True)
  pre, post = (0, 48), (50, 64)
  assert ci.Placebo().pool is False and ci.Placebo(5, 4, 3, True).pool is False         # the default, and the last field
  assert ci.Placebo(5, 4, 3, True, True).pool is True and POOL.simulate is True
  for bad in (1, "yes", None, 0.0):
    with pytest.raises(TypeError, match="Placebo.pool must be True or False"):
      ci.Placebo(simulate=True, pool=bad)
  for simulate in (False,):
    with pytest.raises(ValueError, match=r"Placebo\(pool=True\).*needs `simulate=True`"):
      ci.Placebo(simulate=simulate, pool=True)
  # pool=True without pooled effects, and on the single fit
  for link in (None, "log"):
    with pytest.raises(ValueError, match=r"`Placebo\(pool=True\)` pools the simulated placebo forecasts over `aggregates`"):
      ci.fit_causalimpact_batch([df, df], pre, post, outcome_link=link, placebo=POOL)
    with pytest.raises(ValueError, match=r"`Placebo\(pool=True\)` pools the simulated placebo forecasts over `event_aggregates`"):
      ci.fit_causalimpact_panel([df, df], [(pre, post)] * 2, outcome_link=link, placebo=POOL)
    with pytest.raises(ValueError, match=r"`Placebo\(pool=True\)` is not available on `fit_causalimpact`"):
      ci.fit_causalimpact(df, pre, post, outcome_link=link, placebo=POOL)
  # pool=False: the present refusal keeps the start of its message and now names the option
  old = r"`{}` cannot be combined with `Placebo\(simulate=True\)`.*Placebo\(simulate=True, pool=True\)"
  for link in (None, "log"):
    with pytest.raises(ValueError, match=old.format("aggregates")):
      ci.fit_causalimpact_batch([df, df], pre, post, outcome_link=link, placebo=SIM, aggregates={"all": "all"})
    with pytest.raises(ValueError, match=old.format("event_aggregates")):
      ci.fit_causalimpact_panel([df, df], [(pre, post)] * 2, outcome_link=link, placebo=SIM,
                                event_aggregates={"all": "all"})
  with pytest.raises(ValueError, match=r"`aggregates` cannot be combined with `Placebo\(simulate=True\)`"):
    lib.check_simulated_placebo_pool(SIM, "aggregates")
  # the analytic placebo under a link stays refused, pooled or not
  with pytest.raises(ValueError, match="`placebo=` is not available with `outcome_link`"):
    ci.fit_causalimpact_batch([df, df], pre, post, outcome_link="log", placebo=True, aggregates={"all": "all"})
  # on, with pooled effects: it reaches the fit
  with pytest.raises(AssertionError, match="the sampler was reached"):
    ci.fit_causalimpact_batch([df, df], pre, post, outcome_link="log", placebo=POOL, aggregates={"all": "all"})
  with pytest.raises(AssertionError, match="the sampler was reached"):
    ci.fit_causalimpact_panel([df, df], [(pre, post)] * 2, outcome_link="log", placebo=POOL,
                              event_aggregates={"all": "all"})


# ---- the C-ABI ----------------------------------------------------------------------------------------

def test_the_header_declares_the_three_entries_and_the_binding_lists_them():
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "causalimpact_amd.h")).read(), flags=re.S)
  common = ["const double* scale", "const double* shift", "int32_t num_groups", "const int32_t* offsets",
            "const int32_t* members", "const double* weights", "int32_t max_origins", "const int32_t* origins",
            "const int32_t* horizon", "int32_t link", "const double* init", "double* out", "const double* seen",
            "const int32_t* counted", "int32_t num_ranks", "const int32_t* ranks", "double* predicted_mean",
            "double* spread_mean", "double* below", "double* total_order"]
  want = {"ci_session_pool_simulated_placebo": ["ci_session* session"] + common,
          "ci_session_pool_simulated_placebo_blocks": ["ci_session* session"] + common,
          "ci_test_session_pool_simulated_placebo": ["ci_session* session", "int32_t blocks"] + common +
                                                    ["int32_t chunk_entries"]}
  for name, params in want.items():
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    assert [" ".join(p.split()) for p in m.group(1).split(",")] == params
    assert name in _native.exported_symbols()
    assert list(getattr(_native.load(), name).argtypes) == [C.c_void_p if "*" in p else C.c_int32 for p in params]
  assert re.search(r"#define\s+CI_ABI_VERSION\s+5\b", text) and _native.ABI_VERSION == 5
  for method in ("pool_simulated_placebo", "pool_simulated_placebo_blocks"):
    assert callable(getattr(_native.Session, method))


# ---- the twins ----------------------------------------------------------------------------------------

def test_the_accumulate_twin_is_the_plain_loop_bit_for_bit():
  """Three groups over three series, series 1 in two of them, an empty group, `init` handed on."""
  rng = np.random.default_rng(0)
  groups = [{0: 0.3, 1: 1.7, 2: 1.0}, {}, {1: 0.1, 2: 2.5}]
  csr = _native.groups_csr(groups, 3)
  K, O, N = 5, 4, 11
  totals = np.exp(rng.normal(size=(K, O, N)) * 3.0)
  totals[2, 3] = 0.0
  got = _native.pool_simulated_placebo_host(totals, groups)
  np.testing.assert_array_equal(got, _native.pool_simulated_placebo_host(totals, csr))
  want = np.zeros((3, O, N))
  k = 0
  for g, members in enumerate(groups):
    for b in sorted(members):
      for i in range(O):
        for n in range(N):
          want[g, i, n] = want[g, i, n] + np.float64(members[b]) * totals[k, i, n]
      k += 1
  np.testing.assert_array_equal(got, want)
  assert (got[1] == 0.0).all()
  # cut after the first two series: entries (g0: 0, 1 | 2), (g2: 1 | 2) -- handed on, the same bits
  first = _native.pool_simulated_placebo_host(totals[[0, 1, 3]], [{0: 0.3, 1: 1.7}, {}, {1: 0.1}])
  second = _native.pool_simulated_placebo_host(totals[[2, 4]], [{0: 1.0}, {}, {0: 2.5}], first)
  np.testing.assert_array_equal(second, want)
  assert first is not second and not np.array_equal(first, second)
  with pytest.raises(ValueError, match="the groups have 5 entries, `totals` has 4"):
    _native.pool_simulated_placebo_host(totals[:4], groups)
  with pytest.raises(ValueError, match=r"`totals` must be \[K, O, N\]"):
    _native.pool_simulated_placebo_host(totals[0], groups)


def test_the_finishing_twin_is_the_per_series_definition_on_a_group_of_one():
  """A group {0: 1.0}: the sums are the member's totals and every statistic is `_placebo_simulated_host`'s."""
  y, mask = _level_series(T=30)
  mask = mask.copy()
  mask[[9, 10]] = True
  N, ranks = 74, [0, 3, 36, 70, 73]
  rng = np.random.default_rng(2)
  draws = dict(_level_draws(N), observation_noise_scale=rng.uniform(0.5, 1.0, N), level_scale=rng.uniform(0.1, 0.4, N))
  origins, H = [4, 9, 14, 20, -1], 2                  # (9: a window without observation)
  stream = lib.placebo_stream((3, 4), 2, range(2))
  args = (y, mask, None, np.zeros((0, 30), np.uint8), [], False, PARAMS,
          draws, 0.5, 2.0, origins, H, _native.LINK_LOG, stream)
  plain = lib._placebo_simulated_host(*args)                                  # pylint: disable=protected-access
  seen = plain["totals"][:, 7].copy()
  one = lib._placebo_simulated_host(*args, seen=seen, ranks=ranks)            # pylint: disable=protected-access
  acc = _native.pool_simulated_placebo_host(one["totals"][None], [{0: 1.0}])
  np.testing.assert_array_equal(acc[0], one["totals"])
  got = _native.finish_simulated_placebo_host(acc, seen[None], one["cnt"][None], ranks)
  assert one["cnt"][1] == 0 and one["cnt"][4] == 0 and one["cnt"][0] == 2
  for k in ("predicted_mean", "spread_mean", "below", "total_order"):
    assert got[k].shape == (1,) + one[k].shape
    np.testing.assert_array_equal(got[k][0], one[k], err_msg=k)
  assert (got["below"][0, [0, 2, 3]] >= 1).all() and (got["below"][0, [1, 4]] == 0).all()
  assert (got["spread_mean"][0, [1, 4]] == 0).all() and (got["spread_mean"][0, [0, 2, 3]] > 0).all()


# ---- the frames ---------------------------------------------------------------------------------------

def test_the_frames_of_a_pooled_group_from_a_simulated_summary():
  N = 99
  labels = pd.Index([f"t{i}" for i in range(20)])
  columns = np.array([2, 5, 9, 12, -1])
  stats = dict(predicted_mean=np.array([[10.0, 20.0, 0.0, 40.0, 0.0]]), below=np.array([[0.0, 50.0, 0.0, 99.0, 0.0]]),
               spread_mean=np.array([[5.0, 30.0, 0.0, 125.0, 0.0]]),
               total_order=np.zeros((1, 4, 5)))
  quantiles = (ALPHA / 2, 1 - ALPHA / 2)
  ranks = lib._placebo_sim_ranks(N, quantiles)                                # pylint: disable=protected-access
  stats["total_order"] = np.stack([np.array([8.0, 15.0, 0.0, 30.0, 0.0]) + r for r in range(len(ranks))])[None]
  means = lib._simulated_placebo_means(stats, ranks, N, quantiles)            # pylint: disable=protected-access
  assert set(means) == {"predicted_mean", "spread_mean", "pit_mean", "predicted_lower", "predicted_upper"}
  np.testing.assert_array_equal(means["pit_mean"], (stats["below"] + 0.5) / (N + 1.0))
  psum = dict({k: v[0] for k, v in means.items()}, n_counted=np.array([6.0, 6.0, 0.0, 4.0, 0.0]),
              seen_sum=np.array([11.0, 18.0, 0.0, 50.0, np.nan]))
  actual = np.array([11.5, 18.5, 0.0, 50.5, 0.0])
  frame, quality = lib._aggregate_placebo_frames(psum, actual, columns, 3, ALPHA, labels, 3, 0.25)   # pylint: disable=protected-access
  assert list(frame.columns) == list(lib.PLACEBO_COLUMNS) + list(lib.PLACEBO_SIMULATED_COLUMNS)
  assert list(frame.index) == ["t2", "t5", "t9", "t12"] and frame.index.name == "origin"
  assert list(frame["horizon_end"]) == ["t4", "t7", "t11", "t14"]
  # the window no member counts a step of is a NaN row
  nan_row = frame.loc["t9", [c for c in frame.columns if c not in ("horizon_end", "n_counted", "significant")]]
  assert nan_row.isna().all() and frame.loc["t9", "n_counted"] == 0 and not frame.loc["t9", "significant"]
  ok = frame.drop(index="t9")
  pit = (np.array([0.0, 50.0, 99.0]) + 0.5) / (N + 1.0)
  np.testing.assert_array_equal(ok["pit"], pit)
  np.testing.assert_array_equal(ok["p"], 2.0 * np.minimum(pit, 1.0 - pit))
  assert list(ok["significant"]) == [True, False, True]
  np.testing.assert_array_equal(ok["actual"], [11.5, 18.5, 50.5])
  np.testing.assert_array_equal(ok["predicted"], [10.0, 20.0, 40.0])
  effect = np.array([1.0, -2.0, 10.0])
  np.testing.assert_array_equal(ok["effect"], effect)
  np.testing.assert_array_equal(ok["predicted_sd"], np.sqrt(np.maximum(np.array([5.0, 30.0, 125.0]) - effect ** 2, 0.0)))
  np.testing.assert_array_equal(ok["relative_effect"], effect / np.array([10.0, 20.0, 40.0]))
  # the quantile columns: interpolated from the order statistics as `_simulated_placebo_summaries` does
  (lo_a, hi_a, g_a), (lo_b, hi_b, g_b) = lib._quantile_ranks(N, quantiles)   # pylint: disable=protected-access
  order = {r: stats["total_order"][0, i] for i, r in enumerate(ranks)}
  np.testing.assert_array_equal(ok["predicted_lower"], np.delete(lib._lerp_order_stats(order, lo_a, hi_a, g_a), [2, 4]))   # pylint: disable=protected-access
  np.testing.assert_array_equal(ok["predicted_upper"], np.delete(lib._lerp_order_stats(order, lo_b, hi_b, g_b), [2, 4]))   # pylint: disable=protected-access
  assert (ok["predicted_lower"] < ok["predicted_upper"]).all()
  assert quality["n_origins"] == 3 and quality["false_positive_rate"] == pytest.approx(2 / 3)
  # an analytic summary keeps the analytic columns
  plain = {k: v for k, v in psum.items() if k not in lib.PLACEBO_SIMULATED_COLUMNS}
  assert list(lib._aggregate_placebo_frames(plain, actual, columns, 3, ALPHA, labels, 3, 0.25)[0].columns) == \
      list(lib.PLACEBO_COLUMNS)                                               # pylint: disable=protected-access


# ---- the route that fits series by series ----------------------------------------------------------------

def _frames():
  return [_frame(70, seed) for seed in (0, 1, 2)]


def _host_fit(monkeypatch):
  """The fit by random draws and the effect summary in numpy: nothing reaches a device."""
  _fake_float64_fit(monkeypatch)
  monkeypatch.setattr(_native, "summarize_draws", _summarize_draws_host)


def test_the_host_pool_in_simulated_mode_through_the_batch(monkeypatch):
  _host_fit(monkeypatch)
  frames = _frames()
  idx = frames[0].index
  periods = ((idx[0], idx[48]), (idx[50], idx[64]))
  aggregates = {"all": "all", "one": [1], "weighted": {0: 0.5, 2: 2.0}}
  kw = dict(KW, outcome_link="log")
  got = ci.fit_causalimpact_batch(frames, *periods, placebo=POOL, aggregates=aggregates, **kw)
  sim = ci.fit_causalimpact_batch(frames, *periods, placebo=SIM, **kw)
  off = ci.fit_causalimpact_batch(frames, *periods, aggregates=aggregates, **kw)
  columns = list(lib.PLACEBO_COLUMNS) + list(lib.PLACEBO_SIMULATED_COLUMNS)
  for b in range(3):                     # the per-series frames are those of the call without `pool`
    pd.testing.assert_frame_equal(got[b].placebo, sim[b].placebo, check_exact=True)
    pd.testing.assert_frame_equal(got[b].series, off[b].series, check_exact=True)
  assert off.aggregate_placebo_quality is None and sim.aggregate_placebo_quality is None
  assert list(got.aggregate_placebo_quality.index) == list(aggregates)
  assert list(got.aggregate_placebo_quality.columns) == list(lib.PLACEBO_QUALITY_ENTRIES)
  for name in aggregates:
    one = got.aggregates[name]
    assert list(one.placebo.columns) == columns and len(one.placebo) == 5
    assert off.aggregates[name].placebo is None
    pd.testing.assert_frame_equal(one.series, off.aggregates[name].series, check_exact=True)
    pd.testing.assert_series_equal(one.placebo_quality, got.aggregate_placebo_quality.loc[name], check_names=False)
    below = one.placebo["pit"].to_numpy() * 17 - 0.5
    np.testing.assert_allclose(below, np.round(below), atol=1e-12)
    assert (one.placebo["predicted_lower"] < one.placebo["predicted_upper"]).all()
    assert (one.placebo["predicted_lower"] > 0).all()
  # a group {1: 1.0} reproduces the frame of series 1 exactly
  pd.testing.assert_frame_equal(got.aggregates["one"].placebo, got[1].placebo, check_exact=True)
  # the pooled observed total under the link: the weighted sum of the members' raw outcomes
  w = got.aggregates["weighted"].placebo
  np.testing.assert_allclose(w["actual"], 0.5 * got[0].placebo["actual"].to_numpy() + 2.0 * got[2].placebo["actual"].to_numpy(),
                             rtol=1e-13)
  np.testing.assert_allclose(w["effect"], w["actual"] - w["predicted"], rtol=1e-9, atol=1e-9)
  assert list(w["n_counted"]) == list(got[0].placebo["n_counted"] + got[2].placebo["n_counted"])
  # the pooled totals are the weighted sums of the members' totals: the mean is linear
  np.testing.assert_allclose(w["predicted"], 0.5 * got[0].placebo["predicted"].to_numpy() +
                             2.0 * got[2].placebo["predicted"].to_numpy(), rtol=1e-12)
  a = got.aggregates["all"].placebo
  np.testing.assert_allclose(a["predicted"], sum(got[b].placebo["predicted"].to_numpy() for b in range(3)), rtol=1e-12)
  # independent members: the pooled spread about the mean is below the sum of the members' sds
  assert (a["predicted_sd"] < sum(got[b].placebo["predicted_sd"].to_numpy() for b in range(3))).all()


def test_the_host_pool_in_simulated_mode_through_the_panel(monkeypatch):
  _host_fit(monkeypatch)
  frames = [_frame(70, 0), _frame(70, 1).iloc[:60], _frame(70, 2)]
  every = [((f.index[0], f.index[40 + b]), (f.index[42 + b], f.index[55])) for b, f in enumerate(frames)]
  kw = dict(KW, outcome_link="log")
  event = {"all": "all", "one": [1]}
  got = ci.fit_causalimpact_panel(frames, every, placebo=POOL, event_aggregates=event, **kw)
  sim = ci.fit_causalimpact_panel(frames, every, placebo=SIM, **kw)
  for b in range(3):
    pd.testing.assert_frame_equal(got[b].placebo, sim[b].placebo, check_exact=True)
  assert list(got.aggregate_placebo_quality.index) == list(event)
  for name in event:
    frame = got.aggregates[name].placebo
    assert list(frame.columns) == list(lib.PLACEBO_COLUMNS) + list(lib.PLACEBO_SIMULATED_COLUMNS) and len(frame) >= 3
    assert frame.index.name == "origin" and (frame.index < 0).all()          # (event time: before the treatment)
    assert ((frame["pit"] > 0) & (frame["pit"] < 1)).all()
  # the group of one member: its own simulated totals at the group's origins -- the numbers of a frame
  # of `_placebo_simulated_host` for that series (another plan than the series' own frame's)
  one = got.aggregates["one"].placebo
  assert (one["predicted_lower"] < one["predicted"]).all() and (one["predicted"] < one["predicted_upper"]).all()
