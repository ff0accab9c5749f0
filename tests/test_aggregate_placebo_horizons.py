"""Placebo forecasts of pooled effects at several horizons without a GPU: the host twins
(`_native.pool_placebo_horizons_host`, `_native.finish_placebo_horizons_host`) against the plain loop per
column, the header and the binding, a group of one member against that member's own table, and
`Placebo(horizons=...)` with `aggregates=` / `event_aggregates=` on the route that pools everything on
the host, with the sampler replaced by random draws."""
import ctypes as C
import os
import re
import types

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _native
from causalimpact import batch
from causalimpact import causalimpact_lib as lib

from test_aggregate_placebo import KW, _loop, _member, host_fit   # pylint: disable=unused-import
from test_placebo import _frame

ALPHA = 0.1
SHARED = [k for k in lib.PLACEBO_QUALITY_ENTRIES if k != "horizon"]


# ---- the host twins ------------------------------------------------------------------------------------

@pytest.mark.parametrize("groups", [[{0: 1.0, 1: 0.5, 2: -2.0}],
                                    [{0: 1.0, 2: 0.3}, {1: 0.7, 2: 1.1, 3: 0.25}, {0: 3.0}],
                                    [{1: 1.5}, {}, {0: 1.0, 3: 0.1}]],
                         ids=["single", "overlapping", "empty"])
def test_the_accumulate_twin_is_the_plain_loop_per_column_and_init_continues_it(groups):
  rng = np.random.default_rng(3)
  csr = _native.groups_csr(groups, 4)
  E, O, K, N = int(csr[0][-1]), 3, 4, 5
  s, v = rng.normal(size=(E, O, K, N)) * 50.0, rng.uniform(0.1, 9.0, (E, O, K, N))
  s[:, :, 3], v[:, :, 3] = 0.0, 0.0                               # an unused horizon slot adds terms of 0
  got = _native.pool_placebo_horizons_host(s, v, csr)
  assert got.shape == (len(groups), O, K, 2, N) and (got[:, :, 3] == 0.0).all()
  for k in range(K):
    np.testing.assert_array_equal(got[:, :, k], _loop(s[:, :, k], v[:, :, k], csr[0], csr[2]))
    np.testing.assert_array_equal(got[:, :, k], _native.pool_placebo_host(s[:, :, k], v[:, :, k], csr))
  # `init` continues a sum bit for bit: the loop per column from the same initial values
  init = rng.normal(size=got.shape)
  on = _native.pool_placebo_horizons_host(s, v, csr, init=init)
  for k in range(K):
    np.testing.assert_array_equal(on[:, :, k], _loop(s[:, :, k], v[:, :, k], csr[0], csr[2], init=init[:, :, k]))
  np.testing.assert_array_equal(on[:, :, 3], init[:, :, 3])      # ... and the unused slot keeps it
  # the entries of every group cut in two: the second call continues the first
  halves, keep = [[], []], [[], []]
  for g, group in enumerate(groups):
    items = sorted(group.items())
    cut = (len(items) + 1) // 2
    for h, part in enumerate((items[:cut], items[cut:])):
      halves[h].append(dict(part))
      keep[h] += [int(csr[0][g]) + (0 if h == 0 else cut) + j for j in range(len(part))]
  first = _native.pool_placebo_horizons_host(s[keep[0]], v[keep[0]], halves[0])
  np.testing.assert_array_equal(_native.pool_placebo_horizons_host(s[keep[1]], v[keep[1]], halves[1], init=first), got)
  with pytest.raises(ValueError, match=r"\[E, O, K, N\]"):
    _native.pool_placebo_horizons_host(s[:, :, 0], v[:, :, 0], csr)


def test_the_finishing_twin_is_the_one_horizon_twin_per_column():
  rng = np.random.default_rng(4)
  acc = np.stack([rng.normal(size=(2, 3, 4, 6)) * 10.0, rng.uniform(0.5, 4.0, (2, 3, 4, 6))], axis=3)
  acc[1, 2, 1] = 0.0                                             # a slot no member counts a step in
  acc[:, :, 3] = 0.0                                             # an unused horizon slot
  seen = rng.normal(size=(2, 3, 4)) * 10.0
  got = _native.finish_placebo_horizons_host(acc, seen)
  for k in range(4):
    one = _native.finish_placebo_host(acc[:, :, k], seen[:, :, k])
    for name in _native.PLACEBO_OUTPUTS:
      assert got[name].shape == (2, 3, 4)
      np.testing.assert_array_equal(got[name][:, :, k], one[name], err_msg=f"{name} column {k}")
  for name in _native.PLACEBO_OUTPUTS:
    assert (got[name][:, :, 3] == 0.0).all() and got[name][1, 2, 1] == 0.0 and (got[name][:, :, 0] != 0.0).all()


def test_the_numpy_summary_returns_the_per_draw_terms_at_the_checkpoints():
  one, draws, scale, shift, _ = _member()
  origins, hs = np.array([3, 4, 11, 35, 41, -1, -1]), [1, 2, 9, -1]
  args = (*one.filter_inputs(), draws, scale, shift, origins)
  got = lib._placebo_summary_host(*args, per_draw=True, horizons=hs)            # pylint: disable=protected-access
  table = lib._placebo_summary_host(*args, horizons=hs)                         # pylint: disable=protected-access
  assert got["C"].shape == (7, 4, 24) and got["cnt"].shape == (7, 4)
  for k, h in enumerate(hs[:3]):
    alone = lib._placebo_summary_host(*args, h, per_draw=True)                  # pylint: disable=protected-access
    for name in ("C", "V"):
      np.testing.assert_array_equal(got[name][:, k], alone[name], err_msg=f"{name} h={h}")
    np.testing.assert_array_equal(got["cnt"][:, k], alone["cnt"])
    np.testing.assert_array_equal(got["A"][:, k], alone["A"])
  for name in _native.PLACEBO_OUTPUTS:
    np.testing.assert_array_equal(got[name], table[name])
  assert (got["C"][:, 3] == 0.0).all() and (got["cnt"][2, :2] == 0).all() and got["cnt"][2, 2] == 7
  s, v = _native.placebo_terms_host(got["C"], got["V"], got["cnt"], scale, shift)
  assert s.shape == (7, 4, 24) and (s[2, :2] == 0.0).all() and (v[2, 2] > 0.0).all() and (v[:2, :3] > 0.0).all()


# ---- the C-ABI and the binding ----------------------------------------------------------------------------

def test_the_header_declares_the_entries_and_the_binding_lists_them():
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "causalimpact_amd.h")).read(), flags=re.S)
  common = ["const double* scale", "const double* shift", "int32_t num_groups", "const int32_t* offsets",
            "const int32_t* members", "const double* weights", "int32_t max_origins", "const int32_t* origins",
            "int32_t max_horizons", "const int32_t* horizons", "const double* init", "double* out",
            "const double* seen", "double* predicted_mean", "double* spread_mean", "double* pit_mean"]
  want = {"ci_session_pool_placebo_horizons": ["ci_session* session"] + common,
          "ci_session_pool_placebo_horizons_blocks": ["ci_session* session"] + common,
          "ci_test_session_pool_placebo_horizons": ["ci_session* session", "int32_t blocks"] + common +
                                                   ["int32_t chunk_entries", "int32_t* num_chunks"]}
  for name, params in want.items():
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    assert [" ".join(p.split()) for p in m.group(1).split(",")] == params
    assert name in _native.exported_symbols()
    assert list(getattr(_native.load(), name).argtypes) == [C.c_void_p if "*" in p else C.c_int32 for p in params]
  assert re.search(r"#define\s+CI_ABI_VERSION\s+5\b", text) and _native.ABI_VERSION == 5
  assert callable(_native.Session.pool_placebo_horizons) and callable(_native.DrawsSession.pool_placebo_horizons)


class _NoLibrary:
  def __getattr__(self, name):
    raise AssertionError(f"the library was reached ({name})")


def test_the_binding_refuses_bad_horizon_tables_before_the_library_is_reached():
  sess = object.__new__(_native.Session)
  sess.pb, sess._h, sess._lib = types.SimpleNamespace(num_series=2, num_chains=2, num_results=3), None, _NoLibrary()   # pylint: disable=protected-access
  groups, origins = ({0: 1.0, 1: 2.0}, {1: 1.0}), np.array([[3, 9], [3, -1]], np.int32)
  for bad, msg in (([[2, 2], [5, -1]], r"horizons\[0\] must be strictly ascending"),
                   ([[2, 5], [-1, 5]], r"horizons\[1\] must be strictly ascending .* \(slot 1 holds 5\)"),
                   ([[2, 5], [0, -1]], r"horizons\[1, 0\] must be at least 1, or -1 \(unused\), got 0"),
                   ([[2, 5], [-1, -1]], r"horizons\[1\] holds no horizon: every group needs at least one"),
                   ([[2, 5]], r"`horizons` must be \[2, K\] or \[K\]"),
                   (list(range(1, 66)), r"`horizons` must have 1 to 64 slots per group, got 65"),
                   ([1.5, 2.0], r"`horizons` must hold integers")):
    with pytest.raises(ValueError, match=msg):
      sess.pool_placebo_horizons(1.0, 0.0, groups, origins, bad)
  with pytest.raises(ValueError, match=r"`init` must be \[2, 2, 2, 2, 6\]"):
    sess.pool_placebo_horizons(1.0, 0.0, groups, origins, [2, 5], init=np.zeros((2, 2, 2, 6)))
  with pytest.raises(ValueError, match=r"`seen` must be \[2, 2, 2\]"):
    sess.pool_placebo_horizons(1.0, 0.0, groups, origins, [2, 5], seen=np.zeros((2, 2)))
  with pytest.raises(AssertionError, match="the library was reached"):     # (a good table goes on to it)
    sess.pool_placebo_horizons(1.0, 0.0, groups, origins, [2, 5])
  # the per-series table keeps its wording
  with pytest.raises(ValueError, match=r"horizons\[1\] holds no horizon: every series needs at least one"):
    _native.horizon_table([[2, 5], [-1, -1]], 2)


# ---- a group of one member -------------------------------------------------------------------------------

def test_a_group_of_one_member_has_that_members_own_table():
  one, draws, scale, shift, observed = _member()
  origins, hs, n_post = np.array([3, 4, 11, 35, 41, -1, -1]), np.array([2, 5, 9, -1]), 9
  own = lib._placebo_summary_host(*one.filter_inputs(), draws, scale, shift, origins, horizons=hs)   # pylint: disable=protected-access
  cnt, seen = lib._placebo_seen(one.outcome(), one.mask, origins, 9, scale, shift, horizons=hs)      # pylint: disable=protected-access
  labels = pd.RangeIndex(70)
  psum = dict({"horizons_" + k: v for k, v in own.items()}, horizons_n_counted=cnt, horizons_seen_sum=seen)
  want_by, want_prof = lib._placebo_horizon_frames(psum, origins, hs, ALPHA, observed, labels, n_post, 0.05)   # pylint: disable=protected-access
  entry = lib._placebo_entry_host(one, draws, scale, shift, observed, origins, 9, hs)               # pylint: disable=protected-access
  assert entry["s"].shape == (7, 4, 24) and entry["actual"].shape == (7, 4)
  np.testing.assert_array_equal(entry["n_counted"], cnt)
  for k, h in enumerate(hs[:3]):                                  # column k is the one-horizon entry at h
    alone = lib._placebo_entry_host(one, draws, scale, shift, observed, origins, int(h))            # pylint: disable=protected-access
    for name in alone:
      np.testing.assert_array_equal(entry[name][:, k], alone[name], err_msg=f"{name} h={h}")
  acc = _native.pool_placebo_horizons_host(entry["s"][None], entry["v"][None], [{0: 1.0}])
  means = _native.finish_placebo_horizons_host(acc, entry["seen_sum"][None])
  pooled = dict({k: v[0] for k, v in means.items()}, n_counted=cnt, seen_sum=entry["seen_sum"])
  got_by, got_prof = lib._aggregate_placebo_horizon_frames(pooled, entry["actual"], origins, hs, ALPHA, labels,   # pylint: disable=protected-access
                                                           n_post, 0.05)
  assert got_by.index.equals(want_by.index) and list(got_by.columns) == list(lib.PLACEBO_COLUMNS)
  assert list(got_prof.index) == [2, 5, 9] and list(got_prof.columns) == list(lib.PLACEBO_PROFILE_COLUMNS)
  np.testing.assert_array_equal(got_by["predicted"], want_by["predicted"])
  assert list(got_by["horizon_end"]) == list(want_by["horizon_end"])
  assert list(got_by["significant"]) == list(want_by["significant"])
  for k in ("n_counted", "actual", "predicted_sd", "effect", "relative_effect", "pit", "p"):
    np.testing.assert_allclose(got_by[k], want_by[k], rtol=1e-12, err_msg=k)
  np.testing.assert_allclose(got_prof.to_numpy(), want_prof.to_numpy(), rtol=1e-12)
  assert got_prof["empirical_p"].notna().tolist() == [False, False, True]
  # no origin, or no summary: empty frames
  for args in ((None, entry["actual"], origins), (pooled, entry["actual"], np.full(7, -1))):
    by, prof = lib._aggregate_placebo_horizon_frames(*args, hs, ALPHA, labels, n_post, 0.05)        # pylint: disable=protected-access
    assert len(by) == 0 and by.index.names == ["origin", "horizon"] and len(prof) == 0 and prof.index.name == "horizon"


# ---- the fit functions, on the route that pools on the host -------------------------------------------------

def _assert_identities(one, plain, listed, what):
  """The slice at H is `placebo`, the profile's last row `placebo_quality`; both equal the call
  without horizons, exactly."""
  by_h, prof = one.placebo_by_horizon, one.placebo_profile
  H = int(one.placebo_quality["horizon"])
  assert by_h.index.names == ["origin", "horizon"] and list(by_h.columns) == list(lib.PLACEBO_COLUMNS), what
  assert prof.index.name == "horizon" and list(prof.columns) == list(lib.PLACEBO_PROFILE_COLUMNS), what
  assert list(prof.index) == sorted({h for h in listed if h <= H} | {H}), what
  pd.testing.assert_frame_equal(by_h.xs(H, level="horizon"), one.placebo, check_exact=True)
  pd.testing.assert_series_equal(prof.iloc[-1][SHARED], one.placebo_quality[SHARED], check_names=False, check_exact=True)
  pd.testing.assert_frame_equal(one.placebo, plain.placebo, check_exact=True)
  pd.testing.assert_series_equal(one.placebo_quality, plain.placebo_quality, check_exact=True)
  assert plain.placebo_by_horizon is None and plain.placebo_profile is None, what
  n_post = H if not np.isnan(one.placebo_quality["empirical_p"]) else -1
  assert list(prof["empirical_p"].notna()) == [h == n_post for h in prof.index], what
  assert (prof["n_origins"] > 0).all() and (prof["relative_sd"] > 0).all(), what
  assert len(one.placebo) >= 3 and (by_h["predicted_sd"] > 0).all(), what


def _assert_rest_equal(on, off, names):
  pd.testing.assert_frame_equal(on.summary, off.summary, check_exact=True)
  pd.testing.assert_frame_equal(on.aggregate_summary, off.aggregate_summary, check_exact=True)
  pd.testing.assert_frame_equal(on.placebo_quality, off.placebo_quality, check_exact=True)
  pd.testing.assert_frame_equal(on.aggregate_placebo_quality, off.aggregate_placebo_quality, check_exact=True)
  for b in range(len(on)):
    pd.testing.assert_frame_equal(on[b].series, off[b].series, check_exact=True)
    pd.testing.assert_frame_equal(on[b].summary, off[b].summary, check_exact=True)
    pd.testing.assert_frame_equal(on[b].placebo, off[b].placebo, check_exact=True)
  for name in names:
    pd.testing.assert_frame_equal(on.aggregates[name].series, off.aggregates[name].series, check_exact=True)
    pd.testing.assert_frame_equal(on.aggregates[name].summary, off.aggregates[name].summary, check_exact=True)


def test_batch_on_the_host_route_fills_the_aggregates_horizon_frames(host_fit):   # pylint: disable=unused-argument
  frames = [_frame(70, seed) for seed in (0, 1, 2)]
  idx = frames[0].index
  periods = ((idx[0], idx[48]), (idx[50], idx[64]))           # 49 and 15 steps: H = 15, origins 15 .. 34
  aggregates = {"all": "all", "pair": {0: 1.0, 2: 0.5}, "one": {1: 1.0}}
  several = ci.Placebo(max_origins=64, horizons=(2, 5))
  got = ci.fit_causalimpact_batch(frames, *periods, aggregates=aggregates, placebo=several, **KW)
  plain = ci.fit_causalimpact_batch(frames, *periods, aggregates=aggregates, placebo=ci.Placebo(max_origins=64), **KW)
  assert type(got) is batch.PerSeriesBatchAnalysis and plain.aggregate_placebo_profile is None
  _assert_rest_equal(got, plain, list(aggregates))
  prof = got.aggregate_placebo_profile
  assert prof.index.names == ["aggregate", "horizon"] and list(prof.columns) == list(lib.PLACEBO_PROFILE_COLUMNS)
  assert list(prof.index) == [(name, h) for name in aggregates for h in (2, 5, 15)]
  for name in aggregates:
    one = got.aggregates[name]
    _assert_identities(one, plain.aggregates[name], (2, 5), f"batch {name!r}")
    pd.testing.assert_frame_equal(prof.loc[name], one.placebo_profile, check_exact=True)
    assert len(one.placebo) == 20 and one.placebo_by_horizon.xs(2, level="horizon").index.equals(one.placebo.index)
    assert (one.placebo_by_horizon.xs(2, level="horizon")["n_counted"] <= 2 * len(frames)).all()
  # every listed horizon alone, from the same aggregates, gives its slice on the shared origins
  for h in (2, 5):
    alone = ci.fit_causalimpact_batch(frames, *periods, aggregates=aggregates,
                                      placebo=ci.Placebo(horizon=h, min_history=15, max_origins=64), **KW)
    for name in aggregates:
      want = alone.aggregates[name].placebo
      want = want.loc[want.index.intersection(got.aggregates[name].placebo.index)]
      assert len(want) == 20
      pd.testing.assert_frame_equal(got.aggregates[name].placebo_by_horizon.xs(h, level="horizon").loc[want.index], want,
                                    check_exact=True)
  # a group of one member at weight 1 has that member's own columns
  own, one = got[1].placebo_by_horizon, got.aggregates["one"].placebo_by_horizon
  assert own.index.equals(one.index)
  np.testing.assert_array_equal(one["predicted"], own["predicted"])
  for k in ("n_counted", "actual", "predicted_sd", "effect", "relative_effect", "pit", "p"):
    np.testing.assert_allclose(one[k], own[k], rtol=1e-12, err_msg=k)


def test_panel_on_the_host_route_keeps_every_groups_own_horizons(host_fit):   # pylint: disable=unused-argument
  frames = [_frame(T, seed) for seed, T in enumerate((70, 41, 64))]
  cut = lambda f, a, b, c: ((f.index[0], f.index[a]), (f.index[b], f.index[c]))   # pylint: disable=unnecessary-lambda-assignment
  periods = [cut(frames[0], 48, 50, 66), cut(frames[1], 29, 30, 40), cut(frames[2], 44, 45, 63)]
  aggregates = {"all": "all", "late": [0, 2]}
  several = ci.Placebo(max_origins=64, horizons=(2, 5, 12))
  got = ci.fit_causalimpact_panel(frames, periods, event_aggregates=aggregates, placebo=several, **KW)
  plain = ci.fit_causalimpact_panel(frames, periods, event_aggregates=aggregates, placebo=ci.Placebo(max_origins=64), **KW)
  _assert_rest_equal(got, plain, list(aggregates))
  # "all": H = 9 keeps 2 and 5; "late": H = 14 keeps 2, 5 and 12
  own = {"all": [2, 5, 9], "late": [2, 5, 12, 14]}
  prof = got.aggregate_placebo_profile
  assert list(prof.index) == [(name, h) for name in aggregates for h in (2, 5, 9, 12, 14)]
  for name in aggregates:
    one = got.aggregates[name]
    _assert_identities(one, plain.aggregates[name], (2, 5, 12), f"panel {name!r}")
    assert list(one.placebo_profile.index) == own[name]
    pd.testing.assert_frame_equal(prof.loc[name].loc[own[name]], one.placebo_profile, check_exact=True)
    others = [h for h in (2, 5, 9, 12, 14) if h not in own[name]]
    assert others and prof.loc[name].loc[others].isna().all().all()    # NaN rows for the horizons it lacks
    by_h = one.placebo_by_horizon
    assert (by_h.index.get_level_values("origin") < 0).all() and (np.asarray(by_h["horizon_end"]) < 0).all()
  for h in (2, 5):
    alone = ci.fit_causalimpact_panel(frames, periods, event_aggregates=aggregates,
                                      placebo=ci.Placebo(horizon=h, min_history=14, max_origins=64), **KW)
    for name in aggregates:
      want = alone.aggregates[name].placebo
      want = want.loc[want.index.intersection(got.aggregates[name].placebo.index)]
      assert len(want) >= 5
      pd.testing.assert_frame_equal(got.aggregates[name].placebo_by_horizon.xs(h, level="horizon").loc[want.index], want,
                                    check_exact=True)


def test_without_horizons_or_without_aggregates_nothing_is_added(host_fit, monkeypatch):   # pylint: disable=unused-argument
  frames = [_frame(70, seed) for seed in (0, 1)]
  idx = frames[0].index
  periods = ((idx[0], idx[48]), (idx[50], idx[64]))
  got = ci.fit_causalimpact_batch(frames, *periods, placebo=ci.Placebo(max_origins=5, horizons=(2, 5)), **KW)
  assert got.aggregate_placebo_profile is None and got.aggregates is None and got.placebo_profile is not None

  def never(*a, **k):
    raise AssertionError("the several-horizons frames were reached")
  monkeypatch.setattr(lib, "_aggregate_placebo_horizon_frames", never)
  monkeypatch.setattr(_native, "pool_placebo_horizons_host", never)
  monkeypatch.setattr(_native, "finish_placebo_horizons_host", never)
  plain = ci.fit_causalimpact_batch(frames, *periods, aggregates={"all": "all"}, placebo=ci.Placebo(max_origins=5), **KW)
  assert plain.aggregate_placebo_profile is None and plain.aggregates["all"].placebo_by_horizon is None
  assert plain.aggregates["all"].placebo is not None
