"""Panels of weekly-seasonal series on the device: the ragged build of the time-parallel trend +
seasonal kernel (per-series lengths in one launch) gives every series the bits of its single-series
fit and the oracle's draws; `fit_causalimpact_panel` with `Seasons(7)` against `fit_causalimpact`."""
import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _model
from causalimpact import _native
from causalimpact import _synthetic as syn
from oracle import ci_oracle as orc

pytestmark = pytest.mark.gpu

_KEYS = ("observation_noise_scale", "level_scale", "slope_scale", "seasonal_drift_scales", "weights",
         "level", "slope", "seasonal_levels", "posterior_means", "posterior_trajectories")
_OVER_TIME = ("level", "slope", "seasonal_levels", "posterior_means", "posterior_trajectories")

# lengths per class of the draw's grid (steps per chunk): T % 4 != 0 next to T % 4 == 0, a series
# shorter than one virtual workgroup of chunks, a series exactly at the class bound
_CLASS_LENGTHS = {
    4: [61, 64, 130, 257, 1000, 2048, 2047, 12],
    8: [2049, 2052, 3001, 4096],
}


def _series(T, p, seed, has_slope, b):
  """Sampler inputs of one series: its own pre-period length, a weekly cycle, missing pre-period
  outcomes in every second series."""
  y, mask, X, _ = syn.standardize_for_sampler(*syn.make_raw_series(T, p, seed),
                                              max(2, min(T - 1, int(0.6 * T) + b)))
  y = y + 0.8 * np.sin(2 * np.pi * (np.arange(T) + b) / 7.0)
  if b % 2 == 1 and T > 30:
    mask[[4, 11]] = True
  spec = _model.series_params(np.where(mask, np.nan, y), mask, X, has_slope=has_slope,
                              num_seasonal_blocks=1)
  return y, mask, X, spec


def _over_time(a, k):
  """[.., T] view of a fetched array: seasonal_levels is [.., T, K] with K = 1 here."""
  return a[..., 0] if k == "seasonal_levels" else a


def _pad(arrs, T, fill):
  out = np.full((len(arrs), T) + arrs[0].shape[1:], fill, arrs[0].dtype)
  for b, a in enumerate(arrs):
    out[b, :a.shape[0]] = a
  return out


def _problem(T, P, has_slope, seasons, B=1, C=2, W=3, S=5, seed=(5, 9), **kw):
  return _native.make_problem(T=T, P=P, has_slope=has_slope, num_warmup=W, num_results=S,
                              num_chains=C, num_series=B, seed=seed,
                              num_seasons=_model.expand_seasons(seasons, 1)[0], **kw)


def _fit_ragged(series, has_slope, seasons, flags=0, series_ids=None, series_offset=0, **kw):
  lengths = [s[0].shape[0] for s in series]
  T = (max(lengths) + 3) & ~3                   # the stride: a multiple of 4
  P = 0 if series[0][2] is None else series[0][2].shape[1]
  pb = _problem(T, P, has_slope, seasons, B=len(series), flags=flags, series_offset=series_offset, **kw)
  X = None if P == 0 else _pad([s[2] for s in series], T, 7.5)      # (padding rows are never read)
  sess = _native.Session.ragged(pb, lengths, _pad([s[0] for s in series], T, np.nan),
                                _pad([s[1] for s in series], T, True), X,
                                _native.make_params([s[3] for s in series]), series_ids=series_ids,
                                season_change=_model.expand_seasons(seasons, T)[1])
  try:
    sess.run()
    return sess.fetch(), sess.kernel_name(), sess.algorithmic_bytes()
  finally:
    sess.close()


def _fit_single(s, has_slope, seasons, flags=0, series_offset=0, **kw):
  y, mask, X, spec = s
  T = y.shape[0]
  pb = _problem(T, 0 if X is None else X.shape[1], has_slope, seasons, flags=flags,
                series_offset=series_offset, **kw)
  sess = _native.Session(pb, y[None], mask[None], None if X is None else X[None],
                         _model.expand_seasons(seasons, T)[1], _native.make_params([spec]))
  try:
    sess.run()
    return sess.fetch(), sess.kernel_name(), sess.algorithmic_bytes()
  finally:
    sess.close()


def _assert_series_equals_single(got, b, one, Tb, stride, has_slope):
  for k in _KEYS:
    if k in _OVER_TIME:
      g, w = _over_time(got[k][b], k), _over_time(one[k][0], k)
      np.testing.assert_array_equal(g[..., :Tb], w, err_msg=f"{k} series {b}")
      assert not g[..., Tb:].any(), f"{k} series {b}: padding [{Tb}, {stride}) is not 0"
    else:
      np.testing.assert_array_equal(got[k][b], one[k][0], err_msg=f"{k} series {b}")
  assert np.isfinite(got["level"][b]).all() and got["level"][b][..., :Tb].any()
  assert got["seasonal_levels"][b][..., :Tb, :].any()
  assert got["slope"][b][..., :Tb].any() == bool(has_slope)


@pytest.mark.parametrize("cls,has_slope,seasons,P", [
    (4, False, ((2, 1),), 0),
    (4, True, ((7, 1),), 6),
    (4, False, ((7, 1),), 20),
    (4, True, ((4, 3),), 17),
    (4, True, ((7, 1),), 52),
    (8, True, ((7, 1),), 6),
    (8, False, ((3, 1),), 20),
])
def test_ragged_seasonal_launch_gives_every_series_the_bits_of_its_single_fit(cls, has_slope, seasons, P):
  """One ragged seasonal launch per class of the draw's grid against single-series sessions (shared
  streams, 2 chains): every fetched array over the real steps [0, T_b), bit for bit; the padding
  [T_b, stride) of the five per-step outputs exactly 0, so that no series writes into its
  neighbour's rows.  The single fits run clusters of workgroups where the stock session chooses
  them (T % 4 == 0, P > 0), the panel always one workgroup per chain."""
  lengths = _CLASS_LENGTHS[cls]
  series = [_series(T, max(P - 1, 0), 300 + 17 * b + cls, has_slope, b) for b, T in enumerate(lengths)]
  shared = _native.FLAG_SHARED_SERIES_STREAMS
  got, name, nbytes = _fit_ragged(series, has_slope, seasons, flags=shared)
  assert name == f"ci::gibbs_wide_kernel<{2 if has_slope else 1},{seasons[0][0]},ragged>"
  stride, want_bytes = (max(lengths) + 3) & ~3, 0.0
  assert got["level"].shape[-1] == stride
  for b, s in enumerate(series):
    one, name1, bytes1 = _fit_single(s, has_slope, seasons, flags=shared)
    assert "ragged" not in name1 and "gibbs_wide_kernel" in name1
    want_bytes += bytes1
    _assert_series_equals_single(got, b, one, lengths[b], stride, has_slope)
  assert nbytes == want_bytes                       # real steps, not padding


def test_a_seasonal_series_does_not_depend_on_its_company():
  """Per-series streams: series b of a ragged seasonal launch draws from the streams of ITS id.  The
  same arrays come out when the panel is fitted whole, in two halves that carry their ids
  (contiguous through series_offset, scattered through series_ids), in another order, and among
  strangers of other lengths; series 0 is the plain single fit, series b the single fit with
  series_offset = b."""
  lengths, has_slope, seasons = [300, 512, 257, 400, 333, 500], True, ((7, 1),)
  series = [_series(T, 3, 900 + b, has_slope, b) for b, T in enumerate(lengths)]
  whole, _, _ = _fit_ragged(series, has_slope, seasons)
  for b in (0, 2, 5):
    one, _, _ = _fit_single(series[b], has_slope, seasons, series_offset=b)
    _assert_series_equals_single(whole, b, one, lengths[b], 512, has_slope)
  assert not np.array_equal(whole["level"][0][..., :300], whole["level"][4][..., :300])

  def same(got, rows, ids):
    T = got["level"].shape[-1]
    for r, b in zip(rows, ids):
      Tb = lengths[b]
      for k in _KEYS:
        a, w = got[k][r], whole[k][b]
        if k in _OVER_TIME:
          a, w = _over_time(a, k), _over_time(w, k)
          assert not a[..., Tb:T].any()
          a, w = a[..., :Tb], w[..., :Tb]
        np.testing.assert_array_equal(a, w, err_msg=f"{k} series {b}")

  lo, _, _ = _fit_ragged(series[:3], has_slope, seasons)                       # ids 0..2
  hi, _, _ = _fit_ragged(series[3:], has_slope, seasons, series_offset=3)      # ids 3..5 by offset
  same(lo, range(3), [0, 1, 2])
  same(hi, range(3), [3, 4, 5])
  odd, _, _ = _fit_ragged([series[b] for b in (5, 1, 3)], has_slope, seasons, series_ids=[5, 1, 3])
  same(odd, range(3), [5, 1, 3])
  # other company: series 2 and 4 among strangers of other lengths
  strangers = [_series(T, 3, 5000 + b, has_slope, b) for b, T in enumerate([511, 290])]
  mixed, _, _ = _fit_ragged([strangers[0], series[2], strangers[1], series[4]], has_slope, seasons,
                            series_ids=[40, 2, 41, 4])
  same(mixed, [1, 3], [2, 4])


def test_ragged_seasonal_launch_matches_the_oracle_per_draw():
  """The first draws of one ragged launch (trend with slope, 7 seasons, P = 3; lengths 140, 126, 97)
  against the oracle's, same random numbers: the checks and tolerances of
  test_gpu_gibbs.py::test_seasonal_first_iterations_match_oracle_per_draw.  The reference is the
  oracle's value.  (As there: no warm-up and four draws, while float32 and float64 still walk
  together; both chains of the launch are compared.)"""
  lengths, seasons, S = [140, 126, 97], ((7, 1),), 4
  inputs = []
  for b, T in enumerate(lengths):
    y, mask, X, _ = syn.make_sampler_inputs(T, 2, 7 + b)
    rng = np.random.default_rng(b)
    y = y + 0.8 * np.sin(2 * np.pi * np.arange(T) / 7.0) + 0.1 * rng.normal(size=T)
    if T >= 100:                                          # missing outcomes inside the pre-period
      mask = mask.copy()
      mask[[2, 3, 40, T // 2]] = True
    spec = orc.default_spec(y, mask, X, has_slope=True, seasons=seasons)
    assert spec["P"] == 3
    inputs.append((y, mask, X, spec))
  got, name, _ = _fit_ragged(inputs, 1, seasons, flags=_native.FLAG_SHARED_SERIES_STREAMS,
                             C=2, W=0, S=S, seed=(2, 6))
  assert "ragged" in name
  for b, (y, mask, X, spec) in enumerate(inputs):
    T = lengths[b]
    for c in range(2):
      w = orc.fit_gibbs(y, mask, X, spec, num_results=S, num_warmup=0, seed=(2, 6), chain=c)
      np.testing.assert_allclose(got["level"][b, c][..., :T], w["level"], atol=5e-3)
      np.testing.assert_allclose(got["seasonal_levels"][b, c][..., :T, :], w["seasonal"], atol=5e-3)
      np.testing.assert_allclose(got["seasonal_drift_scales"][b, c], w["drift_scales"], rtol=2e-2)
      np.testing.assert_allclose(got["observation_noise_scale"][b, c], w["obs_scale"], rtol=5e-3)
      np.testing.assert_allclose(got["level_scale"][b, c], w["level_scale"], rtol=5e-3)
      np.testing.assert_allclose(got["slope"][b, c][..., :T], w["slope"], atol=5e-3)
      np.testing.assert_allclose(got["weights"][b, c], w["weights"], atol=5e-3)
      np.testing.assert_allclose(got["posterior_trajectories"][b, c][..., :T], w["trajectories"], atol=1e-2)
      np.testing.assert_allclose(got["posterior_means"][b, c][..., :T], w["pred_mean"], atol=5e-3)
  assert got["seasonal_levels"].shape == (3, 2, S, 140, 1)


def test_ordinary_seasonal_sessions_keep_the_stock_build():
  seasons = ((7, 1),)
  s = _series(300, 3, 1, False, 0)
  _, name, _ = _fit_single(s, False, seasons)
  assert name == "ci::gibbs_wide_kernel<1,7>"
  _, name, _ = _fit_ragged([s, _series(281, 3, 2, False, 1)], False, seasons)
  assert name == "ci::gibbs_wide_kernel<1,7,ragged>"
  pb = _problem(300, 4, False, seasons, B=1)
  sess = _native.Session.ragged(pb, [300], s[0][None], s[1][None], s[2][None],
                                _native.make_params([s[3]]),
                                season_change=_model.expand_seasons(seasons, 300)[1])
  try:
    with pytest.raises(_native.NativeError, match="does not take ragged sessions"):
      sess.run_streamed()
    with pytest.raises(_native.NativeError, match="does not take ragged sessions"):
      sess.profile(True)
  finally:
    sess.close()


def _frames(lengths, p, seed=0):
  frames, periods = [], []
  for b, T in enumerate(lengths):
    idx = pd.date_range("2021-01-04", periods=T, freq="D") + pd.Timedelta(days=2 * b)
    y, X = syn.make_raw_series(T, p, seed + b, effect=5.0 + b)
    y = y + 3.0 * np.sin(2 * np.pi * (np.arange(T) + b) / 7.0)
    frames.append(pd.DataFrame(np.column_stack([y, X]), index=idx,
                               columns=["y"] + [f"x{j}" for j in range(p)]))
    last_pre = (6 * T) // 10 + b
    # rows before the pre-period, a gap, a post-period that ends before the data does
    periods.append(((idx[1 + b % 3], idx[last_pre]), (idx[last_pre + 1 + b % 2], idx[T - 1 - 2 * (b % 3)])))
  frames[1].iloc[[6, 19], 0] = np.nan            # missing pre-period outcomes
  return frames, periods


def _assert_close_to_single(got, b, name, one):
  np.testing.assert_allclose(got.summary.loc[name].to_numpy(float), one.summary.to_numpy(float),
                             rtol=2e-5, atol=1e-7)
  mine = got[b]
  assert list(mine.series.columns) == list(one.series.columns)
  assert mine.series.index.equals(one.series.index)
  num = [c for c in one.series.columns if one.series[c].dtype.kind == "f"]
  np.testing.assert_allclose(mine.series[num].to_numpy(float), one.series[num].to_numpy(float),
                             rtol=2e-5, atol=1e-6, equal_nan=True)


_PANEL_LENGTHS = [140, 126, 133, 97, 140]
_PANEL_KW = dict(alpha=0.1, seed=8, inference_options=ci.InferenceOptions(num_results=120, num_chains=2),
                 model_options=ci.ModelOptions(seasons=[ci.Seasons(num_seasons=7)]))


def test_weekly_panel_fit_equals_separate_fits():
  """`Seasons(7)`, own lengths and periods (one ragged seasonal launch, a stride that is not the
  longest series): the summary rows and per-series frames of `fit_causalimpact` on every frame
  under shared streams, and the same table when the panel is given in reversed order; per-series
  streams: series 0 the plain fit, series b the fit seeded with its stream key."""
  frames, periods = _frames(_PANEL_LENGTHS, 1, seed=30)
  names = [f"geo{b}" for b in range(len(frames))]
  got = ci.fit_causalimpact_panel(frames, periods, names=names, shared_streams=True, **_PANEL_KW)
  assert isinstance(got, ci.CausalImpactPanelAnalysis)
  assert got.summary.shape == (2 * len(frames), 15)
  for b, f in enumerate(frames):
    one = ci.fit_causalimpact(f, *periods[b], **_PANEL_KW)
    _assert_close_to_single(got, b, names[b], one)
  back = ci.fit_causalimpact_panel(frames[::-1], periods[::-1], names=names[::-1], shared_streams=True,
                                   **_PANEL_KW)
  pd.testing.assert_frame_equal(back.summary.loc[names], got.summary.loc[names], check_exact=True)
  ind = ci.fit_causalimpact_panel(frames, periods, names=names, **_PANEL_KW)
  for b in (0, 3):
    kw = dict(_PANEL_KW)
    if b > 0:
      kw["seed"] = _native.series_stream_key(8, b)
    _assert_close_to_single(ind, b, names[b], ci.fit_causalimpact(frames[b], *periods[b], **kw))
  assert not np.allclose(ind.summary.loc["geo3"].to_numpy(float),
                         got.summary.loc["geo3"].to_numpy(float), rtol=1e-6)


def test_weekly_panel_runs_one_ragged_seasonal_launch(monkeypatch):
  """The public call reaches `Session.ragged(..., season_change=...)` once for the whole panel."""
  calls = []
  real = _native.Session.ragged.__func__

  def spy(cls, pb, lengths, *a, **kw):
    calls.append((pb.T, list(lengths), kw.get("season_change") is not None))
    return real(cls, pb, lengths, *a, **kw)

  monkeypatch.setattr(_native.Session, "ragged", classmethod(spy))
  frames, periods = _frames(_PANEL_LENGTHS, 1, seed=30)
  ci.fit_causalimpact_panel(frames, periods, **_PANEL_KW)
  assert len(calls) == 1 and calls[0][2]
  assert calls[0][0] % 4 == 0 and calls[0][0] - 4 < max(calls[0][1]) <= calls[0][0]


def test_weekly_panel_over_two_devices_equals_one_device():
  if _native.device_count() < 2:
    pytest.skip("needs two GPUs")
  frames, periods = _frames(_PANEL_LENGTHS, 1, seed=30)
  one = ci.fit_causalimpact_panel(frames, periods, **_PANEL_KW)
  kw = dict(_PANEL_KW)
  kw["inference_options"] = ci.InferenceOptions(num_results=120, num_chains=2, devices=[0, 1])
  two = ci.fit_causalimpact_panel(frames, periods, **kw)
  pd.testing.assert_frame_equal(one.summary, two.summary, check_exact=True)
  for b in range(len(frames)):
    pd.testing.assert_frame_equal(one[b].series, two[b].series, check_exact=True)
