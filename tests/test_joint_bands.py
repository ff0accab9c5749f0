"""Simultaneous bands and the whole-path test (`joint_bands=True`) without a device: the definitions
in `_native.path_excursions_host`, their calibration, and the frames `causalimpact_lib` builds from
the path arrays of a record."""
import inspect

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _native
from causalimpact import batch
from causalimpact import causalimpact_lib as lib

NAN = np.nan


def test_hand_computed_example():
  """N = 3, T = 5, the window is the steps 1 .. 3 and step 2 has no observation.
    prediction          t1: 1 2 3 (center 2, spread 1)   t2: 2 2 5 (3, sqrt 3)   t3: 3 5 1 (3, 2)
    observed            4, -, 6: excursions 2 at t1 and 1.5 at t3
    cumulative effect   t1: 3 2 1 (2, 1)   t2: the same, not reported   t3: 6 3 6 (5, sqrt 3)
    target 0:           excursions 2 at t1 and 5 / sqrt 3 at t3"""
  traj = np.array([[[9, 1, 2, 3, 9], [9, 2, 2, 5, 9], [9, 3, 5, 1, 9]]], np.float32)
  obs = np.array([0.0, 4.0, NAN, 6.0, 0.0])
  got = _native.path_excursions_host(traj, 1.0, 0.0, obs, [1], [3], ranks=[0, 2])
  r3 = np.sqrt(3.0)
  np.testing.assert_array_equal(got["center"][0, 0], [[NAN, 2, 3, 3, NAN], [NAN, 2, NAN, 5, NAN]])
  np.testing.assert_allclose(got["spread"][0, 0], [[NAN, 1, r3, 2, NAN], [NAN, 1, NAN, r3, NAN]], rtol=1e-15)
  np.testing.assert_array_equal(got["x"][0, 0, 1][:, 1:4], [[3, 3, 6], [2, 2, 3], [1, 1, 6]])
  np.testing.assert_allclose(got["excursion"][0, 0], [[1, 1, 1], [1, 2 / r3, 1]], rtol=1e-15)
  np.testing.assert_allclose(got["observed_excursion"][0, 0], [2.0, 5 / r3], rtol=1e-15)
  np.testing.assert_array_equal(got["at"][0, 0], [1, 3])
  np.testing.assert_array_equal(got["exceed"][0, 0], [0, 0])
  np.testing.assert_allclose(got["excursion_order"][0, 0], [[1, 1], [1, 2 / r3]], rtol=1e-15)
  # a scale and a shift move both the draws' values and nothing else: the observations move along
  moved = _native.path_excursions_host(traj, 2.0, -1.0, obs * 2.0 - 1.0, [1], [3])
  np.testing.assert_allclose(moved["excursion"], got["excursion"], rtol=1e-15)
  np.testing.assert_array_equal(moved["at"], got["at"])
  # the second stage from given moments reproduces itself
  again = _native.path_excursions_host(traj, 1.0, 0.0, obs, [1], [3], ranks=[0, 2], center=got["center"],
                                       spread=got["spread"])
  for k, v in got.items():
    np.testing.assert_array_equal(again[k], v, err_msg=k)
  with pytest.raises(ValueError, match="go together"):
    _native.path_excursions_host(traj, 1.0, 0.0, obs, [1], [3], center=got["center"])
  with pytest.raises(ValueError, match=r"window 0 of series 0: steps 3 .. 5 leave \[0, 5\)"):
    _native.path_excursions_host(traj, 1.0, 0.0, obs, [3], [3])


def test_steps_without_spread_are_left_out_of_the_maxima():
  """Step 1: every draw predicts 2.0, the observation is 100 -- an infinite excursion, were the step
  counted.  The cumulative path has no spread there either (every draw's effect is 98)."""
  traj = np.array([[[2, 1], [2, 2], [2, 6]]], np.float32).transpose(0, 1, 2)
  obs = np.array([100.0, 4.0])
  got = _native.path_excursions_host(traj, 1.0, 0.0, obs, [0], [2])
  np.testing.assert_array_equal(got["spread"][0, 0, :, 0], [0.0, 0.0])
  np.testing.assert_array_equal(got["at"][0, 0], [1, 1])
  assert np.isfinite(got["excursion"]).all() and np.isfinite(got["observed_excursion"]).all()
  # step 1 alone: center 3, devs -2 -1 3, spread sqrt 7; the observation 4 lies 1 / sqrt 7 away
  np.testing.assert_allclose(got["observed_excursion"][0, 0, 0], 1 / np.sqrt(7.0), rtol=1e-15)
  np.testing.assert_allclose(got["excursion"][0, 0, 0], np.array([2, 1, 3]) / np.sqrt(7.0), rtol=1e-15)
  # ... and a window of that step alone counts nothing
  none = _native.path_excursions_host(traj, 1.0, 0.0, obs, [0], [1], ranks=[0, 2])
  assert (none["excursion"] == 0.0).all() and (none["at"] == -1).all()
  assert np.isnan(none["observed_excursion"]).all() and (none["exceed"] == 0).all()


def test_empty_window_and_window_without_an_observation():
  rng = np.random.default_rng(1)
  traj = rng.normal(size=(1, 7, 6)).astype(np.float32)
  obs = np.array([1.0, NAN, NAN, 2.0, 0.5, NAN])
  got = _native.path_excursions_host(traj, 1.5, 0.25, obs, [3, 1, 0], [0, 2, 6], ranks=[0, 3, 6])
  for w in (0, 1):
    assert (got["excursion"][0, w] == 0.0).all() and (got["excursion_order"][0, w] == 0.0).all()
    assert np.isnan(got["observed_excursion"][0, w]).all()
    assert (got["at"][0, w] == -1).all() and (got["exceed"][0, w] == 0).all()
  assert np.isnan(got["center"][0, 0]).all() and np.isnan(got["spread"][0, 0]).all()
  # without an observation the prediction still has its moments, the cumulative path reports none
  assert not np.isnan(got["center"][0, 1, 0, 1:3]).any() and np.isnan(got["center"][0, 1, 1]).all()
  assert (got["excursion"][0, 2] > 0.0).all() and (got["at"][0, 2] >= 0).all()
  np.testing.assert_array_equal(np.isnan(got["center"][0, 2, 1]), np.isnan(obs))


def test_the_p_value_is_calibrated():
  """Draws and the observed path from one law (iid Gaussian steps): p = (1 + exceed) / (1 + N) is
  uniform, so of 400 replications those with p <= 0.05 number 20 +- 4 binomial standard deviations
  (sqrt(400 * 0.05 * 0.95) = 4.4): [3, 38].  (Every draw is part of its own center and spread and the
  observed path is not, so the rate sits a little above 0.05: 0.065 over 20000 replications of this
  shape, 33 of these 400.)"""
  rng = np.random.default_rng(2024)
  N, T, hits = 200, 30, 0
  for _ in range(400):
    paths = rng.normal(size=(N + 1, T))
    got = _native.path_excursions_host(paths[None, :N], 1.0, 0.0, paths[N], [0], [T])
    hits += (1.0 + got["exceed"][0, 0, 0]) / (1.0 + N) <= 0.05
  print("p <= 0.05 in", hits, "of 400 replications")
  assert 3 <= hits <= 38


def _reversing(d=5.0, N=200, T=30, seed=7):
  rng = np.random.default_rng(seed)
  draws = rng.normal(size=(1, N, T))
  effect = np.where(np.arange(T) < T // 2, d, -d)
  return draws, rng.normal(size=T) + effect


def test_a_reversing_effect_is_missed_by_the_total_and_found_by_the_path():
  """+5 sd over the first half of the window and -5 sd over the second: the effects cancel in the
  total (a sum of 30 unit steps has sd 5.5), every single step lies 5 sd out."""
  draws, obs = _reversing()
  T, alpha = obs.size, 0.05
  totals = _native.window_totals_host(draws, 1.0, 0.0, obs, [0], [T])[0, 0, 1]      # per-draw effect sums
  lower, upper = np.quantile(totals, [alpha / 2, 1 - alpha / 2])
  print(f"total effect: band {lower:.2f} .. {upper:.2f}")
  assert lower < 0.0 < upper                                       # not significant by the total
  got = _native.path_excursions_host(draws, 1.0, 0.0, obs, [0], [T])
  critical = np.quantile(got["excursion"][0, 0], 1 - alpha, axis=-1)
  print("critical values", critical, "observed", got["observed_excursion"][0, 0], "exceed", got["exceed"][0, 0])
  assert got["observed_excursion"][0, 0, 0] > critical[0] and got["exceed"][0, 0, 0] == 0
  # the cumulative effect leaves its band too: it peaks at 15 * 5 in the middle of the window
  assert got["observed_excursion"][0, 0, 1] > critical[1] and abs(got["at"][0, 0, 1] - T // 2) <= 2


def _record(draws, obs, first, count, alpha):
  N = draws.shape[1]
  ranks = lib._path_ranks(N, alpha)                              # pylint: disable=protected-access
  got = _native.path_excursions_host(draws, 1.0, 0.0, obs, first, count, ranks=ranks)
  return {k: v[0] for k, v in lib._paths_record(got).items()}, ranks, got   # pylint: disable=protected-access


def test_frames_and_tables_from_a_record():
  draws, post = _reversing()
  N, alpha, pre = draws.shape[1], 0.05, 10
  rng = np.random.default_rng(3)
  draws = np.concatenate([rng.normal(size=(1, N, pre)), draws], axis=2)
  obs = np.concatenate([rng.normal(size=pre), post])
  obs[pre + 4] = NAN
  T = obs.size
  model_idx = pd.date_range("2024-01-01", periods=T, freq="D")
  full_index = pd.date_range("2023-12-30", periods=T + 3, freq="D")
  # window 0 the post-period, then two effect windows, the second one not covered (count 0)
  psum, ranks, got = _record(draws, obs, [pre, pre + 20, pre], [T - pre, 10, 0], alpha)
  bands, summary, by_window = lib._joint_frames(psum, ranks, N, alpha, obs, model_idx, full_index,   # pylint: disable=protected-access
                                                ["late", "absent"])
  assert tuple(bands.columns) == lib.JOINT_BAND_COLUMNS and bands.index.equals(full_index)
  assert tuple(summary.columns) == lib.JOINT_SUMMARY_COLUMNS and tuple(summary.index) == lib.JOINT_PATHS
  inside = bands.loc[model_idx[pre]:model_idx[-1]]
  assert bands.drop(columns="outside").drop(inside.index).isna().all().all()
  assert not bands["outside"].drop(inside.index).any() and bands["outside"].dtype == bool
  # the critical value is numpy's quantile of the excursions, the bands center -+ c * spread
  critical = np.quantile(got["excursion"][0, 0], 1 - alpha, axis=-1)
  np.testing.assert_array_equal(summary["critical_value"].to_numpy(float), critical)
  c0, s0 = got["center"][0, 0, 0, pre:], got["spread"][0, 0, 0, pre:]
  np.testing.assert_array_equal(inside["posterior_lower"].to_numpy(), c0 - critical[0] * s0)
  np.testing.assert_array_equal(inside["posterior_upper"].to_numpy(), c0 + critical[0] * s0)
  np.testing.assert_array_equal(inside["point_effects_lower"].to_numpy(), obs[pre:] - (c0 + critical[0] * s0))
  np.testing.assert_array_equal(inside["point_effects_upper"].to_numpy(), obs[pre:] - (c0 - critical[0] * s0))
  c1, s1 = got["center"][0, 0, 1, pre:], got["spread"][0, 0, 1, pre:]
  np.testing.assert_array_equal(inside["cumulative_effects_upper"].to_numpy(), c1 + critical[1] * s1)
  assert np.isnan(inside["cumulative_effects_lower"].iloc[4]) and not np.isnan(inside["posterior_lower"].iloc[4])
  assert not inside["outside"].iloc[4]                             # (no observation: not outside)
  # the labels, and the flag that never disagrees with the band
  row = summary.loc["pointwise"]
  assert row["at"] == model_idx[got["at"][0, 0, 0]] and row["max_excursion"] == got["observed_excursion"][0, 0, 0]
  assert row["n_outside"] == inside["outside"].sum() > 0
  assert row["first_outside"] == inside.index[inside["outside"].to_numpy()][0]
  assert bool(row["significant"]) is bool(inside["outside"].any()) is True
  assert row["p"] == (1.0 + got["exceed"][0, 0, 0]) / (1.0 + N)
  # ... also where nothing is outside: the observed path replaced by one of the draws' own law
  quiet = obs.copy()
  quiet[pre:] = draws[0, 0, pre:] * 0.5
  psum_q, _, _ = _record(draws, quiet, [pre], [T - pre], alpha)
  bands_q, summary_q, none = lib._joint_frames(psum_q, ranks, N, alpha, quiet, model_idx, full_index)   # pylint: disable=protected-access
  assert none is None and not bands_q["outside"].any()
  assert summary_q.loc["pointwise", "significant"] is False or summary_q.loc["pointwise", "significant"] == False  # noqa: E712
  assert summary_q.loc["pointwise", "first_outside"] is None and summary_q.loc["pointwise", "n_outside"] == 0
  # the windows: their own steps alone, NaN rows where a series does not reach one
  assert by_window.index.names == ["window", None] and len(by_window) == 4
  late = by_window.loc["late"]
  np.testing.assert_array_equal(late["critical_value"].to_numpy(float),
                                np.quantile(got["excursion"][0, 1], 1 - alpha, axis=-1))
  assert model_idx[pre + 20] <= late.loc["pointwise", "at"] <= model_idx[pre + 29]
  absent = by_window.loc["absent"]
  assert absent[["critical_value", "max_excursion", "p", "n_outside"]].isna().all().all()
  assert absent["at"].isna().all() and absent["first_outside"].isna().all()


class _FakeSession:
  summaries = ("effect", "windows", "paths")

  def __init__(self):
    self.calls = []

  def summarize(self, scale, shift, observed, flags, ranks):
    self.calls.append("summarize")
    return dict(value_order=np.zeros((len(ranks), 12)), cum_order=np.zeros((len(ranks), 12)),
                per_draw=np.zeros((2, 6)), per_draw_order=np.zeros((2, len(ranks))))

  def summarize_windows(self, scale, shift, observed, first, count, ranks):
    self.calls.append("summarize_windows")
    return dict(per_draw=np.zeros((1, len(first), 2, 6)))

  def summarize_paths(self, scale, shift, observed, first, count, ranks, want):
    self.calls.append(("summarize_paths", tuple(np.ravel(first)), tuple(np.ravel(count)), tuple(ranks), tuple(want)))
    return {k: np.zeros((1, len(first), 2, 1)) for k in want}


def _request(**parts):
  flags = np.zeros(12, np.uint8)
  flags[8:11] = 3
  return lib.SummaryRequest(scale=2.0, shift=-3.0, observed=np.zeros(12), flags=flags, ranks=[0, 5], **parts), flags


def test_take_summaries_asks_for_the_paths_after_the_windows_and_only_when_asked():
  request, flags = _request(windows=lib.Windows([9], [2]))
  sess = _FakeSession()
  record = lib.take_summaries(sess, request)
  assert sess.calls == ["summarize", "summarize_windows"] and set(record.windows) == {"per_draw"}
  paths = lib.joint_windows(flags, request.windows)
  np.testing.assert_array_equal(paths.first, [8, 9])
  np.testing.assert_array_equal(paths.count, [3, 2])
  request, _ = _request(windows=request.windows, paths=paths, path_ranks=[4, 5])
  sess = _FakeSession()
  record = lib.take_summaries(sess, request)
  assert [c if isinstance(c, str) else c[0] for c in sess.calls] == ["summarize", "summarize_windows", "summarize_paths"]
  assert sess.calls[2][1:4] == ((8, 9), (3, 2), (4, 5))
  assert set(record.windows) == {"per_draw"} | {"path_" + k for k in sess.calls[2][4]}
  assert "excursion" not in sess.calls[2][4]                        # (the per-draw excursions stay on the device)
  # the paths alone: the `windows` kind is there for them
  request, _ = _request(paths=lib.joint_windows(flags), path_ranks=[4, 5])
  record = lib.take_summaries(_FakeSession(), request)
  assert record.windows is not None and "per_draw" not in record.windows
  assert [kind for kind, arrays in record.kinds() if arrays is not None] == ["effect", "windows"]
  whole = lib.SUMMARY_KINDS["windows"].whole
  assert {k for k in record.windows if k not in whole} == {"path_center", "path_spread"}   # (over time)


def test_the_option_is_off_by_default_and_leaves_every_attribute_none():
  for fn in (ci.fit_causalimpact, ci.fit_causalimpact_batch, ci.fit_causalimpact_panel):
    assert inspect.signature(fn).parameters["joint_bands"].default is False
  one = lib.CausalImpactAnalysis(pd.DataFrame(), pd.DataFrame(), None)
  assert one.joint_bands is None and one.joint_summary is None and one.window_joint_summary is None
  summary = pd.DataFrame({"a": [1.0, 2.0]}, index=["average", "cumulative"])
  several = batch.PerSeriesBatchAnalysis(["u", "v"], 0.05, [lib.CausalImpactAnalysis(pd.DataFrame(), summary, None)] * 2)
  assert several.joint_summary is None and several.window_joint_summary is None
  assert several[0].joint_bands is None
  assert "paths" in _native.Session.summaries and "paths" in _native.BatchLogLikSession.summaries
  assert lib.SummaryRequest(1.0, 0.0, np.zeros(3), np.zeros(3, np.uint8), [0]).paths is None
