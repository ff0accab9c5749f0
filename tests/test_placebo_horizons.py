"""`Placebo(horizons=...)` without a GPU: the horizon lists, `_placebo_summary_host` and `_placebo_seen`
at several horizons against themselves at one, the two frames, the panel's own horizons, the refusals
before any fit, and the binding's checks of the horizon table."""
import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _model
from causalimpact import _native
from causalimpact import batch
from causalimpact import causalimpact_lib as lib

import test_placebo as base


# ---- the option ----------------------------------------------------------------------------------

def test_the_int_form_spreads_the_horizons_and_h_is_always_last():
  P = lib.Placebo
  assert lib.placebo_horizon_list(P(), 116) is None                 # off by default
  # unique(max(1, (H i) // k)), i = 1..k
  np.testing.assert_array_equal(lib.placebo_horizon_list(P(horizons=4), 116), [29, 58, 87, 116])
  np.testing.assert_array_equal(lib.placebo_horizon_list(P(horizons=8), 116), [14, 29, 43, 58, 72, 87, 101, 116])
  np.testing.assert_array_equal(lib.placebo_horizon_list(P(horizons=3), 10), [3, 6, 10])
  np.testing.assert_array_equal(lib.placebo_horizon_list(P(horizons=8), 3), [1, 2, 3])   # duplicates dropped
  np.testing.assert_array_equal(lib.placebo_horizon_list(P(horizons=2), 1), [1])
  for k in (2, 5, 16, 64):
    for H in (1, 7, 30, 116):
      hs = lib.placebo_horizon_list(P(horizons=k), H)
      assert hs[-1] == H and hs[0] >= 1 and (np.diff(hs) > 0).all() and len(hs) <= k and hs.dtype == np.int32
  # a sequence: sorted, unique, H added as the last one
  np.testing.assert_array_equal(lib.placebo_horizon_list(P(horizons=(5, 2, 5)), 9), [2, 5, 9])
  np.testing.assert_array_equal(lib.placebo_horizon_list(P(horizons=[9, 1]), 9), [1, 9])
  assert P(horizons=[5, 2, 5]).horizons == (2, 5) and P(horizons=np.int64(3)).horizons == 3
  # beyond H: refused by name -- or, for a panel's series, dropped
  with pytest.raises(ValueError, match=r"Placebo.horizons: the horizon 12 is beyond the placebo horizon 9"):
    lib.placebo_horizon_list(P(horizons=(2, 12)), 9)
  np.testing.assert_array_equal(lib.placebo_horizon_list(P(horizons=(2, 12)), 9, strict=False), [2, 9])
  assert lib.placebo_horizon_list(P(horizons=(2, 5)), 0) is None    # no window at all


def test_bad_options_are_refused_with_the_argument_named():
  P = lib.Placebo
  for bad, kind in ((1, ValueError), (0, ValueError), (65, ValueError), ((0, 3), ValueError), ((), TypeError),
                    ((2.5,), TypeError), ("3", TypeError), (True, TypeError), (tuple(range(1, 66)), ValueError)):
    with pytest.raises(kind, match="Placebo.horizons"):
      P(horizons=bad)
  with pytest.raises(ValueError, match=r"Placebo.horizons is not available with `simulate=True`"):
    P(horizons=3, simulate=True)
  with pytest.raises(ValueError, match=r"Placebo.horizons is not available with `simulate=True`"):
    P(horizons=(2, 5), simulate=True, pool=True)
  # 64 listed horizons below H: H makes 65
  with pytest.raises(ValueError, match="at most 64 horizons, got 65"):
    lib.placebo_horizon_list(P(horizons=tuple(range(1, 65))), 100)
  assert len(lib.placebo_horizon_list(P(horizons=tuple(range(1, 65))), 64)) == 64


def test_horizon_tables_of_a_batch_and_a_panel():
  P = lib.Placebo
  assert batch.placebo_horizon_tables(P(), [9, 9]) is None and batch.placebo_horizon_tables(None, [9]) is None
  np.testing.assert_array_equal(batch.placebo_horizon_tables(P(horizons=(2, 5)), [9, 9]), [[2, 5, 9]] * 2)
  with pytest.raises(ValueError, match="Placebo.horizons: the horizon 5 is beyond the placebo horizon 4"):
    batch.placebo_horizon_tables(P(horizons=(2, 5)), [9, 4])
  # a panel: every series keeps the listed horizons <= its own H; H < 1: a row of -1
  table = batch.placebo_horizon_tables(P(horizons=(2, 5)), [9, 4, 2, 0, 5], strict=False)
  np.testing.assert_array_equal(table, [[2, 5, 9], [2, 4, -1], [2, -1, -1], [-1, -1, -1], [2, 5, -1]])
  assert table.dtype == np.int32
  np.testing.assert_array_equal(batch.placebo_horizon_tables(P(horizons=4), [8, 2], strict=False),
                                [[2, 4, 6, 8], [1, 2, -1, -1]])


# ---- the numpy twin ------------------------------------------------------------------------------

@pytest.mark.parametrize("T,P,has_slope,seasons", [
    (60, 3, False, ()), (60, 0, True, ()), (60, 2, True, ((7, 1),)), (60, 0, False, ((2, 1),)),
    (60, 2, True, ((3, 1), (4, 2))),
])
def test_the_host_summary_at_several_horizons_equals_one_horizon_at_a_time_bit_for_bit(T, P, has_slope, seasons):
  y, mask, X, spec, draws = base._case(T, P, has_slope, seasons)                # pylint: disable=protected-access
  num_seasons, season_change = _model.expand_seasons(seasons, T)
  args = (y, mask, X, season_change, num_seasons, has_slope, spec, draws, 2.5, -3.0)
  origins, hs = [3, 4, 11, 35, T - 13, -1, -1], [1, 2, 9, 13, -1]
  got = lib._placebo_summary_host(*args, origins, horizons=hs)                  # pylint: disable=protected-access
  for k, h in enumerate(hs[:4]):
    one = lib._placebo_summary_host(*args, origins, horizon=h)                  # pylint: disable=protected-access
    for name in _native.PLACEBO_OUTPUTS:
      assert got[name].shape == (7, 5)
      np.testing.assert_array_equal(got[name][:, k], one[name], err_msg=f"{name} h={h}")
  for name in _native.PLACEBO_OUTPUTS:
    assert (got[name][:, 4] == 0.0).all() and (got[name][5:] == 0.0).all()      # the unused slots
    assert (got[name][2, :2] == 0.0).all() and (got[name][2, 2:4] != 0.0).all() # origin 11: steps 11, 12 are missing
  # `horizon` is the table's last one whatever is passed
  same = lib._placebo_summary_host(*args, origins, 1, horizons=hs)              # pylint: disable=protected-access
  np.testing.assert_array_equal(same["pit_mean"], got["pit_mean"])
  for bad in ([2, 2], [5, 2], [-1, 2], [0, 2], [-1, -1], []):
    with pytest.raises(ValueError, match="placebo horizons must be at least 1 and strictly ascending"):
      lib._placebo_summary_host(*args, origins, horizons=bad)                   # pylint: disable=protected-access
  with pytest.raises(ValueError, match="reaches beyond the series"):
    lib._placebo_summary_host(*args, origins, horizons=[2, 14])                 # pylint: disable=protected-access


def test_seen_sums_at_several_horizons_are_the_prefixes_of_the_same_sum():
  rng = np.random.default_rng(3)
  y32 = rng.normal(size=40).astype(np.float32)
  mask = np.zeros(40, bool)
  mask[[11, 12, 20]] = True
  origins, hs = [3, 11, 18, 31, -1], [1, 2, 9, -1]
  cnt, seen = lib._placebo_seen(y32, mask, origins, 9, 2.0, 1.0, horizons=hs)   # pylint: disable=protected-access
  assert cnt.shape == seen.shape == (5, 4)
  for k, h in enumerate(hs[:3]):
    c1, s1 = lib._placebo_seen(y32, mask, origins, h, 2.0, 1.0)                 # pylint: disable=protected-access
    np.testing.assert_array_equal(cnt[:, k], c1)
    np.testing.assert_array_equal(seen[:, k], s1)
  assert (cnt[:, 3] == 0).all() and np.isnan(seen[:, 3]).all() and np.isnan(seen[4]).all()
  np.testing.assert_array_equal(cnt[1], [0, 0, 7, 0])                           # origin 11: 11 and 12 are missing


# ---- the frames ------------------------------------------------------------------------------------

def _hand_table():
  """`test_placebo._hand_placebo` (horizon 2) as the last of the horizons [1, 2, -1]; at horizon 1 the
  window of origin 6 (step 6) is counted and that of origin 4 is not."""
  psum, origins, observed = base._hand_placebo()                                # pylint: disable=protected-access
  psum = {k: np.append(v, 0.0) for k, v in psum.items()}                        # (the unused origin slot)
  one = dict(predicted_mean=np.array([2.5, 0.0, 7.5, 8.0, 0.0]), spread_mean=np.array([1.25, 0.0, 0.5, 2.0, 0.0]),
             pit_mean=np.array([0.3, 0.0, 0.4, 0.9, 0.0]), n_counted=np.array([1.0, 0.0, 1.0, 1.0, 0.0]),
             seen_sum=np.array([2.0, np.nan, 7.0, 9.0, np.nan]))
  table = {"horizons_" + k: np.stack([one[k], psum[k], np.zeros(5)], axis=1) for k in psum}
  return dict(psum, **table), origins, observed


def test_frames_index_columns_and_the_empirical_p_rule_by_hand():
  psum, origins, observed = _hand_table()
  idx = pd.date_range("2024-01-01", periods=10)
  by_h, profile = lib._placebo_horizon_frames(psum, origins, [1, 2, -1], 0.5, observed, idx, 2, -0.3)   # pylint: disable=protected-access
  placebo, quality = lib._placebo_frames(psum, origins, 2, 0.5, observed, idx, 2, -0.3)                 # pylint: disable=protected-access
  assert by_h.index.names == ["origin", "horizon"] and list(by_h.columns) == list(lib.PLACEBO_COLUMNS)
  assert list(by_h.index) == [(idx[o], h) for o in (1, 4, 6, 8) for h in (1, 2)]
  # the slice at H is the frame of H alone; the one at 1 is taken per horizon
  pd.testing.assert_frame_equal(by_h.xs(2, level="horizon"), placebo, check_exact=True)
  at1 = by_h.xs(1, level="horizon")
  assert list(at1["horizon_end"]) == list(idx[[1, 4, 6, 8]])
  np.testing.assert_array_equal(at1["n_counted"], [1, 0, 1, 1])
  np.testing.assert_array_equal(at1["actual"], [2.0, np.nan, 7.0, 9.0])
  np.testing.assert_array_equal(at1["effect"], [-0.5, np.nan, -0.5, 1.0])
  np.testing.assert_array_equal(at1["predicted_sd"], [1.0, np.nan, 0.5, 1.0])   # sqrt(spread - e^2)
  assert list(at1["significant"]) == [False, False, False, True]               # alpha 0.5: pit outside [0.25, 0.75]
  # the profile: the quality entries but the horizon, and relative_sd
  assert profile.index.name == "horizon" and list(profile.index) == [1, 2]
  assert list(profile.columns) == list(lib.PLACEBO_PROFILE_COLUMNS)
  assert lib.PLACEBO_PROFILE_COLUMNS == ("n_origins", "false_positive_rate", "mean_relative_effect", "mde_relative",
                                         "empirical_p", "relative_sd")
  shared = [k for k in lib.PLACEBO_QUALITY_ENTRIES if k != "horizon"]
  pd.testing.assert_series_equal(profile.iloc[-1][shared], quality[shared], check_names=False, check_exact=True)
  assert profile.index[-1] == quality["horizon"]
  # empirical_p on the row h == n_post alone (|placebo| >= 0.3: none of three -> 1 / 4)
  assert np.isnan(profile.loc[1, "empirical_p"]) and profile.loc[2, "empirical_p"] == 0.25
  assert profile.loc[1, "n_origins"] == 3 and profile.loc[1, "false_positive_rate"] == 1 / 3
  assert profile.loc[1, "mean_relative_effect"] == np.mean([-0.2, -0.5 / 7.5, 0.125])
  assert profile.loc[1, "relative_sd"] == np.median([1.0 / 2.5, 0.5 / 7.5, 1.0 / 8.0])
  assert profile.loc[2, "relative_sd"] == np.median([2.0 / 4.0, 0.0, 3.0 / 20.0])
  # n_post 3: no row has the post-period's horizon
  assert lib._placebo_horizon_frames(psum, origins, [1, 2, -1], 0.5, observed, idx, 3, -0.3)[1]["empirical_p"].isna().all()   # pylint: disable=protected-access


def test_a_series_without_origin_or_horizon_has_empty_frames():
  for psum, origins, hs in ((None, np.array([-1, -1]), [2, 5]), ({}, np.array([-1]), [2]), (None, np.array([3]), None)):
    by_h, profile = lib._placebo_horizon_frames(psum, origins, hs, 0.05, np.zeros(4), pd.RangeIndex(4), 3, 0.1)   # pylint: disable=protected-access
    assert len(by_h) == 0 and list(by_h.columns) == list(lib.PLACEBO_COLUMNS) and by_h.index.names == ["origin", "horizon"]
    assert len(profile) == 0 and list(profile.columns) == list(lib.PLACEBO_PROFILE_COLUMNS) and profile.index.name == "horizon"


def test_the_panels_profile_keeps_each_series_own_horizons_and_gives_nan_rows_elsewhere():
  psum, origins, observed = _hand_table()
  T = 10
  res = batch.CausalImpactBatchAnalysis.__new__(batch.CausalImpactBatchAnalysis)
  res._names, res.alpha = ["a", "b", "c"], 0.5
  res._prep = type("P", (), dict(observed=np.stack([observed] * 3)))()
  res._series_view = lambda b: (None, None, None, T)
  res.summary = pd.DataFrame({"rel_effect": [0.0, -0.3, 0.0, 0.2, 0.0, 0.1]})
  res._placebo_profile = None
  # series a: horizons 1 and 2; b: only the first column, read as ITS horizon 1 = its own H; c: no origin
  res._placebo = dict(summary={k: np.stack([v, v, np.zeros_like(v)]) for k, v in psum.items()},
                      origins=np.stack([origins, origins, np.full(5, -1)]), horizon=np.array([2, 1, 0]),
                      n_post=np.array([2, 2, 2]), horizons=np.array([[1, 2, -1], [1, -1, -1], [-1, -1, -1]]))
  prof = res.placebo_profile
  assert prof.index.names == ["series", "horizon"] and list(prof.columns) == list(lib.PLACEBO_PROFILE_COLUMNS)
  assert list(prof.index) == [(s, h) for s in "abc" for h in (1, 2)]
  want = lib._placebo_horizon_frames(psum, origins, [1, 2, -1], 0.5, observed, pd.RangeIndex(T), 2, -0.3)[1]   # pylint: disable=protected-access
  pd.testing.assert_frame_equal(prof.loc["a"], want, check_exact=True)
  pd.testing.assert_series_equal(prof.loc[("b", 1)], want.loc[1], check_names=False, check_exact=True)
  assert prof.loc[("b", 2)].isna().all() and prof.loc["c"].isna().all().all()
  res._placebo = dict(res._placebo, horizons=None)
  assert res.placebo_profile is None
  res._placebo = None
  assert res.placebo_profile is None


# ---- the fit functions -----------------------------------------------------------------------------

def test_fit_causalimpact_frames_on_the_numpy_route(monkeypatch):
  base._fake_float64_fit(monkeypatch)                                          # pylint: disable=protected-access
  df = base._frame()                                                           # pylint: disable=protected-access
  idx = df.index
  kw = dict(data_options=ci.DataOptions(dtype=np.float64), seed=1,
            inference_options=ci.InferenceOptions(num_results=8, summarize_on_device=False))
  periods = ((idx[0], idx[89]), (idx[90], idx[119]))
  plain = ci.fit_causalimpact(df, *periods, placebo=ci.Placebo(max_origins=40), **kw)
  assert plain.placebo_by_horizon is None and plain.placebo_profile is None
  on = ci.fit_causalimpact(df, *periods, placebo=ci.Placebo(max_origins=40, horizons=(2, 12)), **kw)
  # nothing else differs
  pd.testing.assert_frame_equal(on.placebo, plain.placebo, check_exact=True)
  pd.testing.assert_series_equal(on.placebo_quality, plain.placebo_quality, check_exact=True)
  pd.testing.assert_frame_equal(on.series, plain.series, check_exact=True)
  # n_pre 90, n_post 30: H = 30, the origins of the plan at H for every horizon
  by_h, prof = on.placebo_by_horizon, on.placebo_profile
  assert list(prof.index) == [2, 12, 30] and list(by_h.index.get_level_values("horizon")[:3]) == [2, 12, 30]
  assert by_h.index.get_level_values("origin").unique().equals(plain.placebo.index)
  pd.testing.assert_frame_equal(by_h.xs(30, level="horizon"), on.placebo, check_exact=True)
  shared = [k for k in lib.PLACEBO_QUALITY_ENTRIES if k != "horizon"]
  pd.testing.assert_series_equal(prof.iloc[-1][shared], on.placebo_quality[shared], check_names=False, check_exact=True)
  assert prof["empirical_p"].notna().tolist() == [False, False, True]
  # every horizon alone, from the same origins, gives its slice
  for h in (2, 12):
    alone = ci.fit_causalimpact(df, *periods, placebo=ci.Placebo(horizon=h, max_origins=64, min_history=30), **kw)
    want = alone.placebo.loc[alone.placebo.index.intersection(plain.placebo.index)]
    got = by_h.xs(h, level="horizon").loc[want.index]
    assert len(want) == 31                     # (every admissible origin of the plan at H = 30: 30 .. 60)
    pd.testing.assert_frame_equal(got, want, check_exact=True)
  y = df["y"].to_numpy()
  at2 = by_h.xs(2, level="horizon")
  assert list(at2["horizon_end"]) == [o + pd.Timedelta(days=1) for o in at2.index]
  np.testing.assert_allclose(at2["actual"], [np.nansum(y[idx.get_loc(o):idx.get_loc(o) + 2]) for o in at2.index], rtol=1e-13)
  assert (prof["relative_sd"] > 0).all() and prof.loc[2, "relative_sd"] != prof.loc[30, "relative_sd"]
  # the int form
  spread = ci.fit_causalimpact(df, *periods, placebo=ci.Placebo(max_origins=3, horizons=3), **kw)
  assert list(spread.placebo_profile.index) == [10, 20, 30]


def test_refusals_arrive_before_any_fit(monkeypatch):
  def no_fit(*a, **k):
    raise AssertionError("the sampler was reached")
  monkeypatch.setattr(lib, "_run_sampler", no_fit)
  monkeypatch.setattr(batch, "_assemble", no_fit)
  df = base._frame(120).reset_index(drop=True)                                 # pylint: disable=protected-access
  opts = ci.InferenceOptions(num_results=5)
  periods = ((0, 89), (90, 119))                                               # H = 30
  beyond = ci.Placebo(horizons=(2, 31))
  f64 = ci.DataOptions(dtype=np.float64)                                       # (the series-by-series route)
  for call in (lambda: ci.fit_causalimpact(df, *periods, placebo=beyond, inference_options=opts),
               lambda: batch.fit_causalimpact_batch([df, df], *periods, placebo=beyond, inference_options=opts),
               lambda: batch.fit_causalimpact_batch([df, df], *periods, placebo=beyond, inference_options=opts,
                                                    data_options=f64)):
    with pytest.raises(ValueError, match="Placebo.horizons: the horizon 31 is beyond the placebo horizon 30"):
      call()
  # 64 listed horizons and H: 65
  many = ci.Placebo(horizon=80, min_history=5, horizons=tuple(range(1, 65)))
  for call in (lambda: ci.fit_causalimpact(df, *periods, placebo=many, inference_options=opts),
               lambda: batch.fit_causalimpact_batch([df, df], *periods, placebo=many, inference_options=opts)):
    with pytest.raises(ValueError, match="Placebo.horizons: at most 64 horizons, got 65"):
      call()
  # with simulate=True the option itself is refused, so no `outcome_link` fit can carry it
  with pytest.raises(ValueError, match="Placebo.horizons is not available with `simulate=True`"):
    ci.fit_causalimpact(df, *periods, placebo=ci.Placebo(simulate=True, horizons=3), outcome_link="log")
  with pytest.raises(ValueError, match="`placebo=` is not available with `outcome_link`"):
    ci.fit_causalimpact(df, *periods, placebo=ci.Placebo(horizons=3), outcome_link="log")
  # ... and a panel keeps the horizons every series has room for: it goes on to its fit
  with pytest.raises(AssertionError, match="the sampler was reached"):
    batch.fit_causalimpact_panel([df, df], [periods, ((0, 29), (30, 119))], placebo=beyond, inference_options=opts)


# ---- the binding's checks of the horizon table ----------------------------------------------------

def test_the_binding_checks_the_horizon_table_without_a_device():
  np.testing.assert_array_equal(_native.horizon_table([1, 2, 9, -1], 2), [[1, 2, 9, -1]] * 2)
  table = _native.horizon_table([[1, 2], [5, -1]], 2)
  assert table.dtype == np.int32 and table.flags["C_CONTIGUOUS"] and table.shape == (2, 2)
  assert _native.horizon_table(np.arange(1, 65), 1).shape == (1, 64) and _native.MAX_PLACEBO_HORIZONS == 64
  for bad, msg in (([[2, 2], [5, -1]], r"horizons\[0\] must be strictly ascending .*slot 1 holds 2"),
                   ([[5, 2], [5, -1]], r"horizons\[0\] must be strictly ascending"),
                   ([[2, 5], [-1, 5]], r"horizons\[1\] must be strictly ascending .*slot 1 holds 5"),
                   ([[2, 5], [0, -1]], r"horizons\[1, 0\] must be at least 1, or -1 \(unused\), got 0"),
                   ([[2, 5], [-2, -1]], r"horizons\[1, 0\] must be at least 1"),
                   ([[2, 5], [-1, -1]], r"horizons\[1\] holds no horizon"),
                   (np.arange(1, 66), "1 to 64 slots per series, got 65"),
                   (np.zeros((2, 0), np.int32), "1 to 64 slots per series, got 0"),
                   ([[1, 2]], r"`horizons` must be \[2, K\] or \[K\]"),
                   ([[1.5, 2.0]] * 2, "must hold integers")):
    with pytest.raises(ValueError, match=msg):
      _native.horizon_table(bad, 2)
  # ... and `Session.summarize_placebo_horizons` runs them before the library is called
  class NoLibrary:
    def __getattr__(self, name):
      raise AssertionError("the library was reached")
  sess = _native.Session.__new__(_native.Session)
  sess._lib, sess.pb = type("L", (), dict(ci_session_summarize_placebo_horizons=NoLibrary().__getattr__))(), type("pb", (), dict(num_series=2))()
  with pytest.raises(ValueError, match=r"horizons\[0\] must be strictly ascending"):
    sess.summarize_placebo_horizons(1.0, 0.0, [[3, 9], [3, -1]], [[5, 2], [5, -1]])
  with pytest.raises(ValueError, match=r"`origins` must be \[2, O\]"):
    sess.summarize_placebo_horizons(1.0, 0.0, [3, 9], [2, 5])
  with pytest.raises(ValueError, match="unknown placebo outputs"):
    sess.summarize_placebo_horizons(1.0, 0.0, [[3, 9], [3, -1]], [2, 5], want=["pit"])
  assert callable(_native.DrawsSession.summarize_placebo_horizons)
