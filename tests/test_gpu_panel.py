"""Panels on the device: the ragged build of the four-wavefront trend kernel (per-series lengths in
one launch) gives every series the bits of its single-series fit; `fit_causalimpact_panel` on its
three routes against `fit_causalimpact` and `fit_causalimpact_batch`."""
import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _model
from causalimpact import _native
from causalimpact import _synthetic as syn

pytestmark = pytest.mark.gpu

_KEYS = ("observation_noise_scale", "level_scale", "slope_scale", "weights", "level", "slope",
         "posterior_means", "posterior_trajectories")
_OVER_TIME = ("level", "slope", "posterior_means", "posterior_trajectories")

# lengths per steps-per-thread class: T % 4 != 0 next to T % 4 == 0, T < 64, a series exactly at 256 L
_CLASS_LENGTHS = {
    1: [40, 64, 200, 256, 63, 3, 255],
    2: [257, 500, 512, 301],
    4: [513, 1000, 1024, 999],
    8: [2000, 1025, 2048],
    16: [4096, 2049, 3001, 4000],
}


def _series(T, p, seed, has_slope, b):
  """Sampler inputs of one series: its own pre-period length, missing pre-period outcomes in every
  second series."""
  y, mask, X, _ = syn.standardize_for_sampler(*syn.make_raw_series(T, p, seed),
                                              max(2, min(T - 1, int(0.6 * T) + b)))
  if b % 2 == 1 and T > 30:
    mask[[4, 11]] = True
  spec = _model.series_params(np.where(mask, np.nan, y), mask, X, has_slope=has_slope)
  return y, mask, X, spec


def _pad(arrs, T, fill):
  out = np.full((len(arrs), T) + arrs[0].shape[1:], fill, arrs[0].dtype)
  for b, a in enumerate(arrs):
    out[b, :a.shape[0]] = a
  return out


def _problem(T, P, has_slope, B=1, C=2, W=3, S=5, **kw):
  return _native.make_problem(T=T, P=P, has_slope=has_slope, num_warmup=W, num_results=S,
                              num_chains=C, num_series=B, seed=(5, 9), **kw)


def _fit_ragged(series, has_slope, flags=0, series_ids=None, series_offset=0):
  lengths = [s[0].shape[0] for s in series]
  T = max(lengths)
  P = 0 if series[0][2] is None else series[0][2].shape[1]
  pb = _problem(T, P, has_slope, B=len(series), flags=flags, series_offset=series_offset)
  X = None if P == 0 else _pad([s[2] for s in series], T, 7.5)      # (padding rows are never read)
  sess = _native.Session.ragged(pb, lengths, _pad([s[0] for s in series], T, np.nan),
                                _pad([s[1] for s in series], T, True), X,
                                _native.make_params([s[3] for s in series]), series_ids=series_ids)
  try:
    sess.run()
    return sess.fetch(), sess.kernel_name(), sess.algorithmic_bytes()
  finally:
    sess.close()


def _fit_single(s, has_slope, flags=0, series_offset=0):
  y, mask, X, spec = s
  pb = _problem(y.shape[0], 0 if X is None else X.shape[1], has_slope, flags=flags,
                series_offset=series_offset)
  sess = _native.Session(pb, y[None], mask[None], None if X is None else X[None], None,
                         _native.make_params([spec]))
  try:
    sess.run()
    return sess.fetch(), sess.kernel_name(), sess.algorithmic_bytes()
  finally:
    sess.close()


def _assert_series_equals_single(got, b, one, Tb, stride, has_slope):
  for k in _KEYS:
    if k in _OVER_TIME:
      np.testing.assert_array_equal(got[k][b][..., :Tb], one[k][0], err_msg=f"{k} series {b}")
      assert not got[k][b][..., Tb:].any(), f"{k} series {b}: padding [{Tb}, {stride}) is not 0"
    else:
      np.testing.assert_array_equal(got[k][b], one[k][0], err_msg=f"{k} series {b}")
  assert np.isfinite(got["level"][b]).all() and got["level"][b][..., :Tb].any()
  assert got["slope"][b][..., :Tb].any() == bool(has_slope)


@pytest.mark.parametrize("cls,P,has_slope", [
    (1, 0, False), (1, 6, True), (1, 6, False), (1, 40, True), (1, 20, False),
    (2, 0, True), (2, 6, True), (2, 20, False), (2, 40, True),
    (4, 0, False), (4, 6, True), (4, 20, True),
    (8, 0, False), (8, 6, True), (8, 16, False), (8, 20, False),
    (16, 0, False), (16, 6, True), (16, 16, True), (16, 40, False),
])
def test_ragged_launch_gives_every_series_the_bits_of_its_single_fit(cls, P, has_slope):
  """One ragged launch per steps-per-thread class against single-series sessions (shared streams,
  2 chains): every fetched array over the real steps [0, T_b), bit for bit; the padding
  [T_b, stride) of the four per-step outputs exactly 0, so that no series writes into its
  neighbour's rows (series b's last step and series b+1's first equal their single fits).  The single
  fits run on the eight-wavefront kernel where it exists (P <= 16), the panel always on the
  four-wavefront one."""
  # (the three-step series only without covariates: three rows against 6-40 columns test the
  #  regression prior, not the lengths)
  lengths = [12 if (T == 3 and P > 0) else T for T in _CLASS_LENGTHS[cls]]
  series = [_series(T, max(P - 1, 0), 300 + 17 * b + cls, has_slope, b) for b, T in enumerate(lengths)]
  shared = _native.FLAG_SHARED_SERIES_STREAMS
  got, name, nbytes = _fit_ragged(series, has_slope, flags=shared)
  assert "ragged" in name and f"gibbs_kernel<{2 if has_slope else 1},{cls}," in name
  stride, want_bytes = max(lengths), 0.0
  for b, s in enumerate(series):
    one, name1, bytes1 = _fit_single(s, has_slope, flags=shared)
    assert "ragged" not in name1
    want_bytes += bytes1
    _assert_series_equals_single(got, b, one, lengths[b], stride, has_slope)
  assert nbytes == want_bytes                       # real steps, not padding


def test_a_series_does_not_depend_on_its_company():
  """Per-series streams: series b of a ragged launch draws from the streams of ITS id.  The same
  arrays come out when the panel is fitted whole, in two halves that carry their ids (contiguous
  through series_offset, scattered through series_ids), and when every other series is replaced;
  series 0 is the plain single fit, series b the single fit with series_offset = b."""
  lengths, has_slope = [300, 512, 257, 400, 333, 500], True
  series = [_series(T, 3, 900 + b, has_slope, b) for b, T in enumerate(lengths)]
  whole, _, _ = _fit_ragged(series, has_slope)
  for b in (0, 2, 5):
    one, _, _ = _fit_single(series[b], has_slope, series_offset=b)
    _assert_series_equals_single(whole, b, one, lengths[b], 512, has_slope)
  assert not np.array_equal(whole["level"][0][..., :300], whole["level"][4][..., :300])

  def same(got, rows, ids):
    T = got["level"].shape[-1]
    for r, b in zip(rows, ids):
      Tb = lengths[b]
      for k in _KEYS:
        a, w = got[k][r], whole[k][b]
        if k in _OVER_TIME:
          a, w = a[..., :Tb], w[..., :Tb]
          assert not got[k][r][..., Tb:T].any()
        np.testing.assert_array_equal(a, w, err_msg=f"{k} series {b}")

  lo, _, _ = _fit_ragged(series[:3], has_slope)                       # ids 0..2
  hi, _, _ = _fit_ragged(series[3:], has_slope, series_offset=3)      # ids 3..5 by offset
  same(lo, range(3), [0, 1, 2])
  same(hi, range(3), [3, 4, 5])
  odd, _, _ = _fit_ragged([series[b] for b in (5, 1, 3)], has_slope, series_ids=[5, 1, 3])
  same(odd, range(3), [5, 1, 3])
  # other company: series 2 and 4 among strangers of other lengths
  strangers = [_series(T, 3, 5000 + b, has_slope, b) for b, T in enumerate([512, 290])]
  mixed, _, _ = _fit_ragged([strangers[0], series[2], strangers[1], series[4]], has_slope,
                            series_ids=[40, 2, 41, 4])
  same(mixed, [1, 3], [2, 4])


def test_ordinary_sessions_keep_the_stock_build():
  s = _series(300, 3, 1, False, 0)
  _, name, _ = _fit_single(s, False, flags=_native.FLAG_FOUR_WAVES)
  assert name == "ci::gibbs_kernel<1,2,1,false>"
  _, name, _ = _fit_ragged([s, _series(280, 3, 2, False, 1)], False)
  assert name == "ci::gibbs_kernel<1,2,1,false,ragged>"
  pb = _problem(300, 4, False, B=1)
  sess = _native.Session.ragged(pb, [300], s[0][None], s[1][None], s[2][None],
                                _native.make_params([s[3]]))
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


def test_panel_fit_equals_separate_fits():
  """Two steps-per-thread classes (two ragged launches), own lengths and periods: the summary rows
  and the per-series frames of `fit_causalimpact` on every frame, shared streams; per-series
  streams: series 0 the plain fit, series b the fit seeded with its stream key."""
  lengths = [120, 300, 90, 257, 256, 410]
  frames, periods = _frames(lengths, 2)
  opts = ci.InferenceOptions(num_results=150, num_chains=2)
  names = [f"geo{b}" for b in range(len(lengths))]
  got = ci.fit_causalimpact_panel(frames, periods, alpha=0.1, seed=5, inference_options=opts,
                                  names=names, shared_streams=True)
  assert isinstance(got, ci.CausalImpactPanelAnalysis)
  assert len(got) == len(lengths) and got.summary.shape == (2 * len(lengths), 15)
  for b, f in enumerate(frames):
    one = ci.fit_causalimpact(f, *periods[b], alpha=0.1, seed=5, inference_options=opts)
    _assert_close_to_single(got, b, names[b], one)
    assert ci.summary(got[b]) == ci.summary(one)
  assert set(got.diagnostics) == {"split_rhat", "ess_bulk", "ess_tail"}
  ind = ci.fit_causalimpact_panel(frames, periods, alpha=0.1, seed=5, inference_options=opts,
                                  names=names)
  for b in (0, 3):
    seed_b = 5 if b == 0 else _native.series_stream_key(5, b)
    one = ci.fit_causalimpact(frames[b], *periods[b], alpha=0.1, seed=seed_b, inference_options=opts)
    _assert_close_to_single(ind, b, names[b], one)
  assert not np.allclose(ind.summary.loc["geo3"].to_numpy(float),
                         got.summary.loc["geo3"].to_numpy(float), rtol=1e-6)
  # the same series in other company, in another order: the same rows (ids travel with the series)
  sub = [4, 1, 3]
  part = ci.fit_causalimpact_panel([frames[b] for b in sub], [periods[b] for b in sub], alpha=0.1,
                                   seed=5, inference_options=opts, names=[names[b] for b in sub],
                                   shared_streams=True)
  for b in sub:
    np.testing.assert_array_equal(part.summary.loc[names[b]].to_numpy(float),
                                  got.summary.loc[names[b]].to_numpy(float))


def test_equal_length_panel_with_one_period_is_the_batch():
  """Same arithmetic in the kernels, same summary path: the table and the frames of
  `fit_causalimpact_batch`, bit for bit."""
  T, B = 100, 5
  idx = pd.date_range("2021-01-04", periods=T, freq="D")
  frames = []
  for b in range(B):
    y, X = syn.make_raw_series(T, 2, 60 + b, effect=5.0 + b)
    frames.append(pd.DataFrame(np.column_stack([y, X]), index=idx, columns=["y", "x0", "x1"]))
  frames[1].iloc[[3, 17], 0] = np.nan
  pre, post = (idx[0], idx[69]), (idx[72], idx[95])
  opts = ci.InferenceOptions(num_results=120, num_chains=2)
  for shared in (True, False):
    one = ci.fit_causalimpact_batch(frames, pre, post, alpha=0.1, seed=7, inference_options=opts,
                                    shared_streams=shared)
    two = ci.fit_causalimpact_panel(frames, [(pre, post)] * B, alpha=0.1, seed=7,
                                    inference_options=opts, shared_streams=shared)
    pd.testing.assert_frame_equal(one.summary, two.summary, check_exact=True)
    for b in range(B):
      pd.testing.assert_frame_equal(one[b].series, two[b].series, check_exact=True)
      pd.testing.assert_frame_equal(one[b].summary, two[b].summary, check_exact=True)


def test_seasonal_panel_takes_the_equal_length_groups():
  lengths = [140, 126, 140, 126]
  frames, periods = _frames(lengths, 1, seed=30)
  for b, f in enumerate(frames):
    f["y"] += 3.0 * np.sin(2 * np.pi * (np.arange(len(f)) + b) / 7.0)
  # one model length per frame length: the same first pre-period row everywhere
  periods = [((f.index[0], p[0][1]), p[1]) for f, p in zip(frames, periods)]
  kw = dict(seed=8, inference_options=ci.InferenceOptions(num_results=120),
            model_options=ci.ModelOptions(seasons=[ci.Seasons(num_seasons=7)]))
  for shared in (True, False):
    got = ci.fit_causalimpact_panel(frames, periods, shared_streams=shared, **kw)
    for b, f in enumerate(frames):
      k = dict(kw)
      if not shared and b > 0:
        k["seed"] = _native.series_stream_key(8, b)
      one = ci.fit_causalimpact(f, *periods[b], **k)
      _assert_close_to_single(got, b, b, one)


def test_float64_panel_is_fitted_series_by_series():
  from causalimpact import batch
  frames, periods = _frames([80, 64, 95], 1, seed=11)
  do = ci.DataOptions(dtype=np.float64)
  io = ci.InferenceOptions(num_results=60, num_chains=2)
  for shared in (False, True):
    got = ci.fit_causalimpact_panel(frames, periods, seed=3, data_options=do, inference_options=io,
                                    names=["a", "b", "c"], shared_streams=shared)
    assert isinstance(got, batch.PerSeriesBatchAnalysis) and got.summary.shape == (6, 15)
    for b, name in enumerate("abc"):
      seed_b = 3 if shared or b == 0 else _native.series_stream_key(3, b)
      one = ci.fit_causalimpact(frames[b], *periods[b], seed=seed_b, data_options=do,
                                inference_options=io)
      _assert_close_to_single(got, b, name, one)


def test_panel_over_two_devices_equals_one_device():
  if _native.device_count() < 2:
    pytest.skip("needs two GPUs")
  lengths = [120, 300, 90, 257, 256, 410, 77]
  frames, periods = _frames(lengths, 2, seed=70)
  one = ci.fit_causalimpact_panel(frames, periods, seed=5,
                                  inference_options=ci.InferenceOptions(num_results=80, num_chains=2))
  two = ci.fit_causalimpact_panel(frames, periods, seed=5,
                                  inference_options=ci.InferenceOptions(num_results=80, num_chains=2,
                                                                        devices=[0, 1]))
  pd.testing.assert_frame_equal(one.summary, two.summary, check_exact=True)
  for b in range(len(lengths)):
    pd.testing.assert_frame_equal(one[b].series, two[b].series, check_exact=True)
