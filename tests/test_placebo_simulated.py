"""The simulated placebo forecasts (`Placebo(simulate=True)`) without a device: the numpy twin
`_placebo_simulated_host` -- its random stream against the oracle's, its single step against the
prediction filter, the chain rule against the exact moments of the analytic placebo, the log link
against the closed form of a sum of lognormals, gaps and slots, its statistics -- and the option on
the three fit functions through the route that pools the draws on the host."""
import ctypes as C
import os
import re

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _model
from causalimpact import _native
from causalimpact import batch
from causalimpact import causalimpact_lib as lib
from oracle import ci_oracle as orc

from test_placebo import _fake_float64_fit

SITE = 18
PARAMS = dict(init_level_loc=0.2, init_level_scale=1.5, init_slope_scale=0.7, init_seasonal_scale=0.9)
NO_SEASONS = np.zeros((0, 12), np.uint8)


def _level_draws(N, obs=1.0, level=0.5):
  return dict(observation_noise_scale=np.full(N, obs), level_scale=np.full(N, level), slope_scale=np.zeros(N),
              seasonal_drift_scales=np.zeros((N, 0)), weights=np.zeros((N, 0)))


def _level_series(T=12, seed=3):
  rng = np.random.default_rng(seed)
  return np.cumsum(rng.normal(scale=0.5, size=T)) + rng.normal(size=T), np.zeros(T, bool)


# ---- the stream -----------------------------------------------------------------------------------

def test_the_twins_philox_words_and_normals_are_the_oracles():
  assert _native.SITE_PLACEBO_SIM == SITE
  key = _native.series_stream_key((5, 9), 3)
  assert key != (5, 9)
  rng = np.random.default_rng(0)
  ctr = rng.integers(0, 2 ** 32, size=(7, 4), dtype=np.uint64)
  words = _native.philox4x32_10_host(ctr, key)
  assert words.dtype == np.uint32
  for row, got in zip(ctr, words):
    np.testing.assert_array_equal(got, orc.philox([int(v) for v in row], key))
  idx = np.arange(10)
  for chain in (0, 5):
    for sub in (0, 2):
      got = _native.normals_host(key, chain, 7, SITE, sub, idx)
      want = np.array([orc.normal(key, chain, 7, SITE, sub, int(i)) for i in idx])
      # log, sqrt, cos / sin and the product are each good to about an ulp in both libms and
      # |z| < 6.7: the gap stays below 8 ulp of 8
      np.testing.assert_allclose(got, want, rtol=0, atol=1e-14)
      # the counter's words: call idx >> 2, site | sub << 8, iteration, chain
      call1 = orc.philox([1, SITE | (sub << 8), 7, chain], key)
      np.testing.assert_array_equal(
          _native.philox4x32_10_host([1, SITE | (sub << 8), 7, chain], key), call1)
  # vectorised over chains and iterations at once
  grid = _native.normals_host(key, np.array([0, 5])[:, None], np.array([7, 8])[None, :], SITE, 2, 9)
  assert grid.shape == (2, 2) and grid[1, 0] == _native.normals_host(key, 5, 7, SITE, 2, 9)


# ---- H = 1 ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("link", [_native.LINK_IDENTITY, _native.LINK_LOG, _native.LINK_LOG1P])
def test_horizon_one_is_the_link_of_one_draw_from_the_one_step_forecast(link):
  T, N = 30, 3
  rng = np.random.default_rng(1)
  y, mask = rng.normal(size=T), np.zeros(T, bool)
  mask[[6, 7]] = True
  X = rng.normal(size=(T, 2))
  num_seasons, sc = _model.expand_seasons([(4, 1), (3, 2)], T)
  draws = dict(observation_noise_scale=rng.uniform(0.5, 1, N), level_scale=rng.uniform(0.1, 0.3, N),
               slope_scale=rng.uniform(0.01, 0.1, N), seasonal_drift_scales=rng.uniform(0.05, 0.2, (N, 2)),
               weights=rng.normal(size=(N, 2)))
  key, chain = _native.series_stream_key((1, 2), 4), 6
  scale, shift, origins = 0.4, 1.5, [3, 9, 20, -1]
  got = lib._placebo_simulated_host(y, mask, X, sc, num_seasons, True, PARAMS, draws, scale, shift, origins, 1, link,
                                    (key, (chain,)))
  assert got["totals"].shape == (4, N) and (got["totals"][3] == 0).all()
  for n in range(N):
    one = {k: v[n:n + 1] for k, v in draws.items()}
    pred = lib._prediction_summary_host(y, mask, X, sc, num_seasons, True, PARAMS, one, 1.0, 0.0, [0])
    for slot, o in enumerate(origins[:3]):
      f, F = pred["forecast_mean"][o], pred["variance_mean"][o]
      z = _native.normals_host(key, chain, n, SITE, slot, 0)
      want = _native.link_values_host((f + np.sqrt(F) * z) * scale + shift, link)
      np.testing.assert_allclose(got["totals"][slot, n], want, rtol=1e-12)


# ---- the chain rule and the log link: N = 20000 draws with the same parameters ---------------------

N_BIG, CHAINS = 20000, (0, 1, 2, 3)
STREAM = ((11, 2024), CHAINS)


def test_the_chain_rule_gives_the_exact_moments_of_the_analytic_placebo():
  """Local level, T = 12, one origin at 6, H = 5, no gaps: mean and variance of the simulated totals
  against C and V of the analytic placebo.  A branch without the update on the simulated value loses
  the cross-covariances of the window's steps and misses the second bound by far (checked below)."""
  y, mask = _level_series()
  draws = _level_draws(N_BIG)
  args = (y, mask, None, NO_SEASONS, [], False, PARAMS, draws, 1.0, 0.0, [6], 5)
  exact = lib._placebo_summary_host(*args, per_draw=True)
  C, V = exact["C"][0, 0], exact["V"][0, 0]
  totals = lib._placebo_simulated_host(*args, _native.LINK_IDENTITY, STREAM)["totals"][0]
  mean, var = totals.mean(), totals.var(ddof=1)
  print(f"C {C:.6f} mean {mean:.6f} bound {5 * np.sqrt(V / N_BIG):.6f};  V {V:.5f} var {var:.5f} "
        f"bound {5 * V * np.sqrt(2 / (N_BIG - 1)):.5f}")
  assert abs(mean - C) <= 5 * np.sqrt(V / N_BIG)
  assert abs(var - V) <= 5 * V * np.sqrt(2.0 / (N_BIG - 1))
  # the variance of five INDEPENDENT draws from the marginal forecasts -- what a branch without the
  # update would simulate -- is far outside the bound
  one = lib._placebo_summary_host(y, mask, None, NO_SEASONS, [], False, PARAMS, _level_draws(1), 1.0, 0.0, [6], 5,
                                  per_draw=True)
  pred = lib._prediction_summary_host(y, mask, None, NO_SEASONS, [], False, PARAMS, _level_draws(1), 1.0, 0.0, [0])
  p0 = pred["variance_mean"][6] - 1.0
  independent = sum(p0 + h * 0.25 + 1.0 for h in range(5))
  assert one["V"][0, 0] == V and abs(independent - V) > 20 * V * np.sqrt(2.0 / (N_BIG - 1))


def test_the_log_link_gives_the_mean_of_a_sum_of_lognormals():
  y, mask = _level_series()
  scale, shift, H, o = 0.3, 1.2, 5, 6
  args = (y, mask, None, NO_SEASONS, [], False, PARAMS, _level_draws(N_BIG), scale, shift, [o], H)
  totals = lib._placebo_simulated_host(*args, _native.LINK_LOG, STREAM)["totals"][0]
  pred = lib._prediction_summary_host(y, mask, None, NO_SEASONS, [], False, PARAMS, _level_draws(1), 1.0, 0.0, [0])
  a, p0 = pred["forecast_mean"][o], pred["variance_mean"][o] - 1.0      # the level's predicted moments at o
  mu = np.full(H, a * scale + shift)
  p = (p0 + 0.25 * np.arange(H)) * scale * scale                          # Var(level at o + h), data scale
  s = p[np.minimum.outer(np.arange(H), np.arange(H))] + np.eye(H) * scale * scale
  E = np.exp(mu + np.diag(s) / 2.0)
  want, var = E.sum(), float((np.outer(E, E) * (np.exp(s) - 1.0)).sum())
  print(f"mean {totals.mean():.5f} closed form {want:.5f} standard error {np.sqrt(var / N_BIG):.5f}")
  assert abs(totals.mean() - want) <= 5 * np.sqrt(var / N_BIG)


# ---- gaps and slots -----------------------------------------------------------------------------------

def _scalar_reference(y, mask, obs, level, key, chain, it, slot, o, H, scale, shift, link):
  """The definition for a local level, one draw, written out with scalars."""
  a, P = PARAMS["init_level_loc"], PARAMS["init_level_scale"] ** 2
  for t in range(o):
    if not mask[t]:
      F = P + obs * obs
      a, P = a + (P / F) * (y[t] - a), P - P * P / F
    P = P + level * level
  total, cnt = 0.0, 0
  for h in range(H):
    if not mask[o + h]:
      F = P + obs * obs
      z = orc.normal(key, chain, it, SITE, slot, h)                     # idx = h, counted or not
      v = np.sqrt(F) * z
      total += float(_native.link_values_host((a + v) * scale + shift, link))
      cnt += 1
      a, P = a + (P / F) * v, P - P * P / F
    if h + 1 < H:
      P = P + level * level
  return total, cnt


def test_a_masked_step_is_skipped_and_later_normals_keep_their_index():
  T, H = 24, 6
  rng = np.random.default_rng(8)
  y, mask = rng.normal(size=T), np.zeros(T, bool)
  mask[[5, 9, 10]] = True
  mask[14:20] = True                                                     # the window of origin 14: nothing counted
  key = _native.series_stream_key((3, 4), 2)
  origins = [2, 7, 14, -1, -1]
  C, S = (5, 9), 2                                                       # chains 5 and 9, two kept draws each
  draws = _level_draws(4, 0.8, 0.3)
  got = lib._placebo_simulated_host(y, mask, None, np.zeros((0, T), np.uint8), [], False, PARAMS, draws, 0.5, 1.0,
                                    origins, H, _native.LINK_LOG, (key, C), seen=[9.0, 9.0, 9.0, np.nan, np.nan],
                                    ranks=[0, 3])
  np.testing.assert_array_equal(got["cnt"], [5, 4, 0, 0, 0])
  for n in range(4):
    for slot, o in enumerate(origins[:2]):
      want, cnt = _scalar_reference(y, mask, 0.8, 0.3, key, C[n // S], n % S, slot, o, H, 0.5, 1.0, _native.LINK_LOG)
      assert cnt == got["cnt"][slot]
      np.testing.assert_allclose(got["totals"][slot, n], want, rtol=1e-12)
  # nothing counted, and the unused slots at the end of the row: 0 everywhere
  for k in ("totals", "predicted_mean", "spread_mean", "below"):
    assert (got[k][2:] == 0).all(), k
  assert (got["total_order"][:, 2:] == 0).all()
  # ... and NaN in the frame
  psum = dict(predicted_mean=got["predicted_mean"], spread_mean=got["spread_mean"],
              pit_mean=(got["below"] + 0.5) / 5.0, n_counted=got["cnt"], seen_sum=np.array([9.0, 9.0, 0, np.nan, np.nan]),
              predicted_lower=got["total_order"][0], predicted_upper=got["total_order"][1])
  frame, _ = lib._placebo_frames(psum, origins, H, 0.1, np.where(mask, np.nan, y), pd.RangeIndex(T), H, 0.1)
  assert list(frame.columns) == list(lib.PLACEBO_COLUMNS) + ["predicted_lower", "predicted_upper"]
  assert list(frame.index) == [2, 7, 14]
  assert frame.loc[14, ["predicted", "predicted_sd", "pit", "p", "predicted_lower", "predicted_upper"]].isna().all()
  assert frame.loc[[2, 7]].notna().all().all() and not frame.loc[14, "significant"]
  for bad in ([7, 2, -1], [2, -1, 7], [2, 2], [-2]):
    with pytest.raises(ValueError, match="strictly ascending steps with the unused slots"):
      lib._placebo_simulated_host(y, mask, None, np.zeros((0, T), np.uint8), [], False, PARAMS, draws, 1.0, 0.0,
                                  bad, H, 0, (key, C))
  with pytest.raises(ValueError, match="reaches beyond the series' 24 steps"):
    lib._placebo_simulated_host(y, mask, None, np.zeros((0, T), np.uint8), [], False, PARAMS, draws, 1.0, 0.0,
                                [19], H, 0, (key, C))
  with pytest.raises(ValueError, match="not a whole number of draws"):
    lib._placebo_simulated_host(y, mask, None, np.zeros((0, T), np.uint8), [], False, PARAMS, draws, 1.0, 0.0,
                                [2], H, 0, (key, (0, 1, 2)))


def test_a_block_model_runs_and_its_statistics_equal_plain_numpy_on_the_totals():
  T, N, H = 40, 74, 5
  rng = np.random.default_rng(2)
  y, mask = rng.normal(size=T), np.zeros(T, bool)
  mask[[11, 12]] = True
  num_seasons, sc = _model.expand_seasons([(4, 1), (3, 1)], T)
  draws = dict(observation_noise_scale=rng.uniform(0.5, 1, N), level_scale=rng.uniform(0.1, 0.3, N),
               slope_scale=rng.uniform(0.01, 0.1, N), seasonal_drift_scales=rng.uniform(0.05, 0.2, (N, 2)),
               weights=np.zeros((N, 0)))
  origins, ranks = [8, 9, 20, -1], [0, 1, 36, 72, 73]
  stream = lib.placebo_stream((5, 9), 1, range(2))
  assert stream == (_native.series_stream_key((5, 9), 1), (0, 1)) and lib.placebo_stream(7) == ((0, 7), (0,))
  first = lib._placebo_simulated_host(y, mask, None, sc, num_seasons, True, PARAMS, draws, 0.5, 2.0, origins, H,
                                      _native.LINK_LOG1P, stream)
  assert "below" not in first and "spread_mean" not in first
  seen = np.append(first["totals"][:3, 7], np.nan)                        # (a tie with draw 7)
  got = lib._placebo_simulated_host(y, mask, None, sc, num_seasons, True, PARAMS, draws, 0.5, 2.0, origins, H,
                                    _native.LINK_LOG1P, stream, seen=seen, ranks=ranks)
  totals = got["totals"]
  np.testing.assert_array_equal(totals, first["totals"])
  assert np.isfinite(totals).all() and (totals[:3] > 0).all() and list(got["cnt"]) == [3, 3, 5, 0]
  np.testing.assert_allclose(got["predicted_mean"], totals.mean(axis=1), rtol=1e-13)
  np.testing.assert_array_equal(got["predicted_mean"], _native.row_means_host(totals))
  np.testing.assert_array_equal(got["total_order"], np.sort(totals, axis=1)[:, ranks].T)
  below = (totals[:3] <= seen[:3, None]).sum(axis=1)
  np.testing.assert_array_equal(got["below"], np.append(below, 0))
  assert (below >= 1).all()
  spread = ((totals[:3] - seen[:3, None]) ** 2)
  np.testing.assert_allclose(got["spread_mean"][:3], spread.mean(axis=1), rtol=1e-13)
  np.testing.assert_array_equal(got["spread_mean"], np.append(_native.row_means_host(spread), 0.0))
  # the chains are addressed by their global ids: the draws of chain 1 alone give its half of the totals
  half = {k: v[37:] for k, v in draws.items()}
  alone = lib._placebo_simulated_host(y, mask, None, sc, num_seasons, True, PARAMS, half, 0.5, 2.0, origins, H,
                                      _native.LINK_LOG1P, (stream[0], (1,)))
  np.testing.assert_array_equal(alone["totals"], totals[:, 37:])


# ---- the option on the three fit functions, on the route that pools the draws on the host ------------

ALPHA = 0.1
KW = dict(data_options=ci.DataOptions(dtype=np.float64), seed=(0, 1), alpha=ALPHA,
          inference_options=ci.InferenceOptions(num_results=8, num_chains=2, summarize_on_device=False))
SIM = ci.Placebo(max_origins=5, simulate=True)
NEW = ["predicted_lower", "predicted_upper"]


def _frame(T=70, seed=0):
  rng = np.random.default_rng(seed)
  x = rng.normal(size=T)
  y = np.exp(2.0 + 0.2 * x + np.cumsum(rng.normal(scale=0.02, size=T)) + rng.normal(scale=0.1, size=T))
  y[[11, 12, 40]] = np.nan
  return pd.DataFrame({"y": y, "x": x}, index=pd.date_range("2024-01-01", periods=T))


def _check_frame(placebo, frame, n_draws=16):
  assert list(placebo.columns) == list(lib.PLACEBO_COLUMNS) + NEW and len(placebo) == 5
  y = frame["y"].to_numpy()
  rows = [frame.index.get_loc(o) for o in placebo.index]
  H = frame.index.get_loc(placebo["horizon_end"].iloc[0]) - rows[0] + 1
  np.testing.assert_allclose(placebo["actual"], [np.nansum(y[o:o + H]) for o in rows], rtol=1e-13)
  # seen_sum is the sum of the raw outcome over the counted steps: effect = it - predicted
  np.testing.assert_allclose(placebo["effect"], placebo["actual"] - placebo["predicted"], rtol=1e-9, atol=1e-9)
  below = placebo["pit"].to_numpy() * (n_draws + 1) - 0.5
  np.testing.assert_allclose(below, np.round(below), atol=1e-12)
  assert ((below >= 0) & (below <= n_draws)).all()
  np.testing.assert_allclose(placebo["p"], 2 * np.minimum(placebo["pit"], 1 - placebo["pit"]))
  assert (placebo["p"] >= 1.0 / (n_draws + 1) - 1e-15).all()             # the Monte-Carlo floor
  assert (placebo["predicted_lower"] < placebo["predicted_upper"]).all() and (placebo["predicted_lower"] > 0).all()
  assert ((placebo["predicted"] > placebo["predicted_lower"]) & (placebo["predicted"] < placebo["predicted_upper"])).all()
  assert (placebo["predicted_sd"] > 0).all()
  assert list(placebo["significant"]) == list((placebo["pit"] < ALPHA / 2) | (placebo["pit"] > 1 - ALPHA / 2))


def test_fit_causalimpact_with_a_log_link(monkeypatch):
  _fake_float64_fit(monkeypatch)
  df = _frame()
  idx = df.index
  periods = ((idx[0], idx[48]), (idx[50], idx[64]))
  assert ci.Placebo().simulate is False and ci.Placebo(5, 4, 3).simulate is False      # the default, and the last field
  off = ci.fit_causalimpact(df, *periods, outcome_link="log", **KW)
  on = ci.fit_causalimpact(df, *periods, outcome_link="log", placebo=SIM, **KW)
  _check_frame(on.placebo, df)
  assert list(on.placebo_quality.index) == list(lib.PLACEBO_QUALITY_ENTRIES) and on.placebo_quality["n_origins"] == 5
  pd.testing.assert_frame_equal(on.series, off.series, check_exact=True)
  pd.testing.assert_frame_equal(on.summary, off.summary, check_exact=True)
  assert off.placebo is None
  # the same seed, the same frame; another seed, other totals
  again = ci.fit_causalimpact(df, *periods, outcome_link="log", placebo=SIM, **KW)
  pd.testing.assert_frame_equal(again.placebo, on.placebo, check_exact=True)
  other = ci.fit_causalimpact(df, *periods, outcome_link="log", placebo=SIM, **dict(KW, seed=(0, 2)))
  assert (other.placebo["predicted"] != on.placebo["predicted"]).all()
  # under the identity the two routes describe the same forecast: the new columns on this route only
  analytic = ci.fit_causalimpact(df, *periods, placebo=ci.Placebo(max_origins=5), **KW)
  simulated = ci.fit_causalimpact(df, *periods, placebo=SIM, **KW)
  assert list(analytic.placebo.columns) == list(lib.PLACEBO_COLUMNS)
  assert list(simulated.placebo.columns) == list(lib.PLACEBO_COLUMNS) + NEW
  for column in ("n_counted", "actual", "horizon_end"):
    assert list(simulated.placebo[column]) == list(analytic.placebo[column])
  # (16 draws: the simulated mean lies within a few predictive sds / 4 of the exact one)
  assert (np.abs(simulated.placebo["predicted"] - analytic.placebo["predicted"]) < 2.0 * analytic.placebo["predicted_sd"]).all()
  # log1p runs too
  _check_frame(ci.fit_causalimpact(df, *periods, outcome_link="log1p", placebo=SIM, **KW).placebo, df)


def test_batch_and_panel_with_a_log_link_key_every_series_by_its_own_stream(monkeypatch):
  _fake_float64_fit(monkeypatch)
  frames = [_frame(70, seed) for seed in (0, 1, 2)]
  idx = frames[0].index
  periods = ((idx[0], idx[48]), (idx[50], idx[64]))
  got = ci.fit_causalimpact_batch(frames, *periods, outcome_link="log", placebo=SIM, **KW)
  assert got.placebo_quality.shape == (3, len(lib.PLACEBO_QUALITY_ENTRIES))
  panel = ci.fit_causalimpact_panel(frames, [periods] * 3, outcome_link="log", placebo=SIM, **KW)
  for b in range(3):
    _check_frame(got[b].placebo, frames[b])
    # series b is the single fit on the key of series id b
    one = ci.fit_causalimpact(frames[b], *periods, outcome_link="log", placebo=SIM,
                              **dict(KW, seed=_native.series_stream_key(KW["seed"], b)))
    pd.testing.assert_frame_equal(got[b].placebo, one.placebo, check_exact=True)
    pd.testing.assert_frame_equal(panel[b].placebo, one.placebo, check_exact=True)
  assert (got[1].placebo["pit"].to_numpy() != got[2].placebo["pit"].to_numpy()).any()
  off = ci.fit_causalimpact_batch(frames, *periods, outcome_link="log", **KW)
  assert off.placebo_quality is None and off[0].placebo is None


def test_refusals_arrive_before_any_fit(monkeypatch):
  def no_fit(*a, **k):
    raise AssertionError("the sampler was reached")
  monkeypatch.setattr(lib, "_run_sampler", no_fit)
  monkeypatch.setattr(batch, "_assemble", no_fit)
  df = _frame().reset_index(drop=True)
  pre, post = (0, 48), (50, 64)
  for bad in (1, "yes", None, 0.0):
    with pytest.raises(TypeError, match="Placebo.simulate must be True or False"):
      ci.Placebo(simulate=bad)
  # off: the present refusal under a link, now pointing to the option
  for placebo in (True, ci.Placebo(), ci.Placebo(simulate=False)):
    for call in (lambda p: ci.fit_causalimpact(df, pre, post, outcome_link="log", placebo=p),
                 lambda p: ci.fit_causalimpact_batch([df, df], pre, post, outcome_link="log1p", placebo=p),
                 lambda p: ci.fit_causalimpact_panel([df, df], [(pre, post)] * 2, outcome_link="log", placebo=p)):
      with pytest.raises(ValueError, match=r"`placebo=` is not available with `outcome_link`.*Placebo\(simulate=True\)"):
        call(placebo)
  # on: it reaches the fit
  with pytest.raises(AssertionError, match="the sampler was reached"):
    ci.fit_causalimpact(df, pre, post, outcome_link="log", placebo=SIM)
  # the pooled combinations are refused by name, with and without a link
  for link in (None, "log"):
    with pytest.raises(ValueError, match=r"`aggregates` cannot be combined with `Placebo\(simulate=True\)`"):
      ci.fit_causalimpact_batch([df, df], pre, post, outcome_link=link, placebo=SIM, aggregates={"all": "all"})
    with pytest.raises(ValueError, match=r"`event_aggregates` cannot be combined with `Placebo\(simulate=True\)`"):
      ci.fit_causalimpact_panel([df, df], [(pre, post)] * 2, outcome_link=link, placebo=SIM,
                                event_aggregates={"all": "all"})


def test_the_header_declares_both_entries_and_the_binding_lists_them():
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "causalimpact_amd.h")).read(), flags=re.S)
  for name in ("ci_session_simulate_placebo", "ci_session_simulate_placebo_blocks"):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["ci_session* session", "const double* scale", "const double* shift", "int32_t max_origins",
                      "const int32_t* origins", "const int32_t* horizon", "int32_t link", "const double* seen",
                      "int32_t num_ranks", "const int32_t* ranks", "double* predicted_mean", "double* spread_mean",
                      "double* below", "double* total_order", "double* totals"]
    assert name in _native.exported_symbols()
    assert list(getattr(_native.load(), name).argtypes) == [C.c_void_p if "*" in p else C.c_int32 for p in params]
  assert re.search(r"#define\s+CI_ABI_VERSION\s+5\b", text) and _native.ABI_VERSION == 5
  assert callable(_native.Session.simulate_placebo) and callable(_native.Session.simulate_placebo_blocks)
