"""Panels (series with their own index, length and periods), the host side: vectorised data
preparation == per-series CausalImpactData, the routing table, the ragged entry point's argument
checks (no device touched) and the per-series-window summary table."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _native
from causalimpact import _synthetic as syn
from causalimpact import batch
from causalimpact import causalimpact_lib as lib
from causalimpact import data as cid


def _panel(lengths, p, seed=0, dates=True):
  """Frames of the given lengths (own start dates) and own periods: rows before the pre-period, a
  gap and a tail."""
  frames, periods = [], []
  for b, T in enumerate(lengths):
    idx = (pd.date_range("2021-01-04", periods=T, freq="D") + pd.Timedelta(days=3 * b)) if dates \
        else pd.RangeIndex(T)                      # (integer periods are positions into the index)
    y, X = syn.make_raw_series(T, p, seed + b, effect=5.0 + b)
    frames.append(pd.DataFrame(np.column_stack([y, X]), index=idx,
                               columns=["y"] + [f"x{j}" for j in range(p)]))
    first, last_pre = 2 + b, (6 * T) // 10 + b
    post0, post1 = last_pre + 1 + (b % 3), T - 1 - (b % 4)
    periods.append(((idx[first], idx[last_pre]), (idx[post0], idx[post1])))
  return frames, periods


@pytest.mark.parametrize("standardize", [True, False])
@pytest.mark.parametrize("dates", [True, False])
def test_prepare_panel_equals_causal_impact_data(standardize, dates):
  lengths, p = [90, 61, 140, 90, 75], 2
  frames, periods = _panel(lengths, p, dates=dates)
  frames[1].iloc[[5, 17], 0] = np.nan          # missing pre-period outcomes
  frames[2].iloc[:, 1] = 7.0                   # constant covariate: left unscaled
  prep = batch.prepare_panel(frames, periods, standardize)
  T_max = prep.y.shape[1]
  assert T_max == int(prep.lengths.max()) and prep.design.shape == (len(frames), T_max, p + 1)
  for b, f in enumerate(frames):
    pre, post = periods[b]
    one = cid.CausalImpactData(f, pre, post, standardize_data=standardize, dtype=np.float64)
    n_pre = len(one.outcome_ts.time_series)
    Tb = n_pre + one.num_steps_forecast
    assert prep.num_pre[b] == n_pre and prep.lengths[b] == Tb
    np.testing.assert_allclose(prep.y[b, :n_pre], one.outcome_ts.time_series, rtol=1e-12,
                               equal_nan=True)
    assert prep.mask[b, n_pre:].all() and np.isnan(prep.y[b, n_pre:]).all()
    np.testing.assert_array_equal(prep.mask[b, :n_pre], one.outcome_ts.is_missing)
    np.testing.assert_allclose(prep.design[b, :Tb], one.feature_ts.values, rtol=1e-12)
    assert (prep.design[b, Tb:] == 0).all()
    if standardize:
      np.testing.assert_allclose(prep.outcome_mean[b], one.outcome_scaler.mean_, rtol=1e-13)
      np.testing.assert_allclose(prep.outcome_sd[b], one.outcome_scaler.stddev_, rtol=1e-13)
    assert list(f.index[prep.model_rows[b]]) == list(f.index[2 + b:])
    # what the device summary is asked for: the single-series request, padded with NaN / 0
    rq = lib._device_summary_request(one, 0.05)                          # pylint: disable=protected-access
    np.testing.assert_array_equal(prep.observed[b, :Tb], rq["observed"])
    np.testing.assert_array_equal(prep.flags[b, :Tb], rq["flags"])
    assert np.isnan(prep.observed[b, Tb:]).all() and (prep.flags[b, Tb:] == 0).all()


def test_prepare_panel_without_covariates_and_from_arrays():
  frames, periods = _panel([40, 55], 0, dates=False)
  prep = batch.prepare_panel([f.to_numpy() for f in frames], periods,
                             indices_=[f.index for f in frames])
  assert prep.design is None
  for b, f in enumerate(frames):
    one = cid.CausalImpactData(f, *periods[b], dtype=np.float64)
    n = len(one.outcome_ts.time_series)
    np.testing.assert_allclose(prep.y[b, :n], one.outcome_ts.time_series, rtol=1e-12)


def test_prepare_panel_rejects_what_the_reference_rejects_naming_the_series():
  frames, periods = _panel([40, 50, 45], 1, dates=False)
  names = ["north", "south", "west"]
  bad = [f.copy() for f in frames]
  bad[1]["y"] = 3.0
  with pytest.raises(ValueError, match="'south'.*cannot be constant"):
    batch.prepare_panel(bad, periods, names=names)
  bad = [f.copy() for f in frames]
  bad[2].iloc[4, 1] = np.nan
  with pytest.raises(ValueError, match="'west'.*cannot have any missing values"):
    batch.prepare_panel(bad, periods, names=names)
  bad = [f.copy() for f in frames]
  bad[0].iloc[2:, 0] = np.nan
  with pytest.raises(ValueError, match="'north'.*at least 3 observations"):
    batch.prepare_panel(bad, periods, names=names)
  i1 = frames[1].index
  overlap = list(periods)
  overlap[1] = ((i1[0], i1[30]), (i1[25], i1[45]))
  with pytest.raises(ValueError, match="'south'.*cannot overlap"):
    batch.prepare_panel(frames, overlap, names=names)
  short = list(periods)
  short[2] = ((frames[2].index[0], frames[2].index[1]), periods[2][1])
  with pytest.raises(ValueError, match="'west'.*at least 3 time points"):
    batch.prepare_panel(frames, short, names=names)
  with pytest.raises(ValueError, match="one .* per series"):
    batch.prepare_panel(frames, periods[:2])
  with pytest.raises(ValueError, match="share the columns"):
    batch.prepare_panel([frames[0], frames[1][["y"]]], periods[:2])


_LENGTHS = [200, 256, 257, 1024, 1025, 4096, 4097]


@pytest.mark.parametrize("kw,route,groups", [
    (dict(lengths=_LENGTHS[:-1]), "ragged",
     [(1, [0, 1]), (2, [2]), (4, [3]), (8, [4]), (16, [5])]),
    (dict(lengths=[500, 40, 300, 257, 512, 3]), "ragged", [(1, [1, 5]), (2, [0, 2, 3, 4])]),
    (dict(lengths=_LENGTHS), "equal_length", [(t, [b]) for b, t in enumerate(_LENGTHS)]),
    (dict(lengths=[300, 200, 300, 200], num_seasonal_blocks=1), "equal_length",
     [(200, [1, 3]), (300, [0, 2])]),
    (dict(lengths=[300, 200, 300], P=53), "equal_length", [(200, [1]), (300, [0, 2])]),
    (dict(lengths=[300, 200], P=52), "ragged", [(1, [1]), (2, [0])]),
    (dict(lengths=[300, 200], float64=True), "per_series", [(0, [0]), (1, [1])]),
    (dict(lengths=[300, 200], standardize_data=False), "per_series", [(0, [0]), (1, [1])]),
    (dict(lengths=[300, 200], sampler="hmc"), "per_series", [(0, [0]), (1, [1])]),
])
def test_panel_route(kw, route, groups):
  a = dict(float64=False, standardize_data=True, sampler="gibbs", num_seasonal_blocks=0, P=6)
  a.update(kw)
  got = batch.panel_route(**a)
  assert got["route"] == route and got["groups"] == groups


def test_steps_class_is_the_kernels_steps_per_thread():
  assert [batch.steps_class(t) for t in (3, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097)] == \
      [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 0]


def test_panel_stream_ids_do_not_depend_on_the_grouping():
  """Every launch carries the panel positions of its series -- the ids its streams are keyed by --
  whatever the route, the number of devices or the composition of the panel; ordinary sessions
  (series_offset + b) only ever get runs of consecutive positions unless the streams are shared."""
  lengths = [500, 40, 300, 257, 512, 3, 1000, 41]
  for devices in ([0], [0, 1], [0, 1, 2]):
    for blocks in (0, 1):
      r = batch.panel_route(float64=False, standardize_data=True, sampler="gibbs",
                            num_seasonal_blocks=blocks, P=2, lengths=lengths)
      for shared in (False, True):
        launches = batch.panel_launches(r, devices, shared)
        ids = sorted(b for _, _, part in launches for b in part)
        assert ids == list(range(len(lengths)))                    # every series once, by position
        for dev, key, part in launches:
          assert dev in devices
          want_key = (lambda t: t) if blocks else batch.steps_class
          assert {want_key(lengths[b]) for b in part} == {key}
          if blocks and not shared:
            assert part == list(range(part[0], part[0] + len(part)))
  # equal lengths far apart in the panel: one launch when shared, else one per run of neighbours
  r = batch.panel_route(float64=False, standardize_data=True, sampler="gibbs", num_seasonal_blocks=1,
                        P=0, lengths=[100, 100, 50, 100])
  assert [p for _, _, p in batch.panel_launches(r, [0], True)] == [[2], [0, 1, 3]]
  assert [p for _, _, p in batch.panel_launches(r, [0], False)] == [[2], [0, 1], [3]]


def test_ragged_entry_point_validates_before_any_device_call():
  L = _native.load()
  spec = dict.fromkeys(_native._PARAM_FIELDS, 1.0)   # pylint: disable=protected-access
  B, T = 3, 300
  prm = _native.make_params([spec] * B)
  y = np.zeros((B, T), np.float32)
  m = np.zeros((B, T), np.uint8)

  def create(lengths, ids=None, **kw):
    base = dict(T=T, P=0, has_slope=0, num_warmup=1, num_results=2, num_series=B)
    base.update(kw)
    pb = _native.make_problem(**base)
    Tn, Pn = base["T"], base["P"]
    X = np.zeros((B, Tn, Pn), np.float32) if Pn else None
    ln = None if lengths is None else np.asarray(lengths, np.int32)
    idv = None if ids is None else np.asarray(ids, np.int32)
    h = C.c_void_p()
    rc = L.ci_session_create_ragged(C.byref(pb), None if ln is None else ln.ctypes.data,
                                    None if idv is None else idv.ctypes.data,
                                    np.zeros((B, Tn), np.float32).ctypes.data,
                                    np.zeros((B, Tn), np.uint8).ctypes.data,
                                    None if X is None else X.ctypes.data, prm, C.byref(h))
    assert rc != 0 and not h.value
    return L.ci_last_error().decode()

  assert "series_lengths is NULL" in create(None)
  assert "series_lengths[1] must be >= 3, got 2" in create([300, 2, 280])
  assert "series_lengths[2] = 301 exceeds the stride T=300" in create([300, 280, 301])
  assert "max(series_lengths) = 290, T = 300" in create([290, 280, 270])
  msg = create([300, 256, 280])
  assert "series_lengths[1] = 256 runs 1 steps per thread" in msg and "(300) runs 2" in msg
  assert "num_blocks must be 0, got 1" in create([300, 280, 270], num_seasons=(7,))
  assert "at most 52 design columns, got P=53" in create([300, 280, 270], P=53)
  assert "at most 4096 steps, got T=4097" in create([4097, 4000, 3000], T=4097)
  assert "series_ids[2] must be >= 0, got -4" in create([300, 280, 270], ids=[0, 7, -4])
  # the checks of every session come first
  assert "num_results >= 1" in create([300, 280, 270], num_results=0)
  # through the binding: the same message as a NativeError, and the shape checks of the wrapper
  pb = _native.make_problem(T=T, P=0, has_slope=0, num_warmup=1, num_results=2, num_series=B)
  with pytest.raises(_native.NativeError, match=r"series_lengths\[0\] must be >= 3, got 1"):
    _native.Session.ragged(pb, [1, 300, 280], y, m, None, prm)
  with pytest.raises(ValueError, match="one entry per series"):
    _native.Session.ragged(pb, [300, 280], y, m, None, prm)
  with pytest.raises(ValueError, match="one entry per series"):
    _native.Session.ragged(pb, [300, 280, 270], y, m, None, prm, series_ids=[0, 1])


@pytest.mark.parametrize("with_order", [True, False])
def test_panel_summary_table_equals_the_single_series_rows(with_order):
  """The per-series-window table (own window, own number of observed steps) against `_summary_rows`
  of the single-series code, on synthetic per-draw totals: positive, negative and zero-straddling
  totals, a window with missing observations, a window at the very end of the longest series."""
  rng = np.random.default_rng(5)
  B, N, alpha = 5, 301, 0.1
  lengths = np.array([60, 44, 80, 51, 80])
  T_max = int(lengths.max())
  windows = [(40, 55), (30, 44), (50, 80), (33, 47), (61, 62)]
  observed = np.full((B, T_max), np.nan)
  flags = np.zeros((B, T_max), np.uint8)
  post_mean = rng.normal(size=(B, T_max)) * 3.0 + 50.0
  for b, (w0, w1) in enumerate(windows):
    observed[b, :lengths[b]] = rng.normal(size=lengths[b]) + 50.0
    observed[b, w1:lengths[b]] = np.nan                       # tail: predictions only
    flags[b, w0:lengths[b]] |= 1
    flags[b, w0:w1] |= 2
  observed[1, 33] = np.nan                                    # a hole in the window
  per_draw = rng.normal(size=(B, 2, N)) * 20.0
  per_draw[0, 0] += 3000.0
  per_draw[1, 0] -= 3000.0
  per_draw[2, 0] += 5.0                                       # straddling zero
  per_draw[3, 0] = np.abs(per_draw[3, 0]) + 1.0
  per_draw[4, 0] += 800.0
  quantiles = (alpha / 2.0, 1.0 - alpha / 2.0)
  ranks = lib._summary_ranks(N, quantiles)                    # pylint: disable=protected-access
  dsum = dict(per_draw=per_draw)
  if with_order:
    dsum["per_draw_order"] = np.sort(per_draw, axis=2)[:, :, ranks]
  stats = batch.panel_window_stats(observed, flags, post_mean, lengths)
  names = [f"s{b}" for b in range(B)]
  table = batch.summary_table(names, alpha, ranks, dsum, **stats)
  assert table.shape == (2 * B, 15)
  for b, (w0, w1) in enumerate(windows):
    obs_w, pm_w = observed[b, w0:w1], post_mean[b, w0:w1]
    n_obs = int(np.sum(~np.isnan(obs_w)))
    assert stats["n_win"][b] == w1 - w0 and stats["n_obs"][b] == n_obs
    pred_sum, point_sum = per_draw[b]
    rows, p_value = lib._summary_rows(pm_w, obs_w, pred_sum / (w1 - w0), pred_sum,     # pylint: disable=protected-access
                                      point_sum / n_obs, point_sum, quantiles)
    for col, (avg, cum) in rows.items():
      np.testing.assert_allclose(table.loc[(names[b], "average"), col], avg, rtol=1e-13, atol=0)
      np.testing.assert_allclose(table.loc[(names[b], "cumulative"), col], cum, rtol=1e-13, atol=0)
    np.testing.assert_allclose(table.loc[(names[b], "average"), "p_value"], p_value, rtol=1e-15)
    assert table.loc[(names[b], "average"), "alpha"] == alpha


def test_batch_summary_is_what_the_shared_helper_gives_for_one_window():
  """`CausalImpactBatchAnalysis` (one shared window) builds its table through the same helper as
  the panel container: for an equal-length panel with one period the two tables are identical."""
  T, B, N, alpha = 60, 4, 201, 0.08
  idx = pd.date_range("2021-01-04", periods=T, freq="D")
  frames = []
  for b in range(B):
    y, X = syn.make_raw_series(T, 1, 40 + b, effect=4.0)
    frames.append(pd.DataFrame(np.column_stack([y, X]), index=idx, columns=["y", "x0"]))
  pre, post = (idx[0], idx[39]), (idx[42], idx[57])
  values = np.stack([f.to_numpy(float) for f in frames])
  prep_b = batch.prepare_batch(values, idx, pre, post, True)
  prep_p = batch.prepare_panel(frames, [(pre, post)] * B, True)
  np.testing.assert_array_equal(prep_p.y, prep_b.y)
  np.testing.assert_array_equal(prep_p.design, prep_b.design)
  np.testing.assert_array_equal(prep_p.outcome_mean, prep_b.outcome_mean)
  np.testing.assert_array_equal(prep_p.outcome_sd, prep_b.outcome_sd)
  rng = np.random.default_rng(2)
  means = rng.normal(size=(B, prep_b.y.shape[1])).astype(np.float32)
  per_draw = rng.normal(size=(B, 2, N)) * 20.0 + 900.0
  ranks = lib._summary_ranks(N, (alpha / 2.0, 1.0 - alpha / 2.0))   # pylint: disable=protected-access
  dsum = dict(per_draw=per_draw, per_draw_order=np.sort(per_draw, axis=2)[:, :, ranks])
  names, cols = list("abcd"), ["y", "x0"]
  one = batch.CausalImpactBatchAnalysis(prep_b, names, alpha, means, dsum, ranks, cols, None)
  two = batch.CausalImpactPanelAnalysis(prep_p, names, alpha, means, dsum, ranks, cols, None)
  pd.testing.assert_frame_equal(one.summary, two.summary, check_exact=True)
  assert len(two) == B and two.diagnostics_of(0) is None


def test_panel_refuses_bad_arguments_before_fitting():
  frames, periods = _panel([40, 50], 1)
  with pytest.raises(ValueError, match="sampler must be"):
    ci.fit_causalimpact_panel(frames, periods, inference_options=ci.InferenceOptions(sampler="nuts"))
  with pytest.raises(ValueError, match="one .* per series"):
    ci.fit_causalimpact_panel(frames, periods[:1])
  with pytest.raises(ValueError, match="share the columns"):
    ci.fit_causalimpact_panel([frames[0], frames[1].rename(columns={"x0": "z"})], periods)
  with pytest.raises(ValueError, match="alpha"):
    ci.fit_causalimpact_panel(frames, periods, alpha=1.5)


# ---- the assembler (`batch._assemble`) over a fake launch function: no device, no library ----

_C, _S, _R, _P = 2, 5, 3, 1          # chains, draws per chain, order statistics, design columns
_W, _O = 2, 3                        # windows, placebo origin slots


def _fake_launch(lengths, calls):
  """A launch function that returns what a session would, as a function of the panel position b
  and the step t alone: base(b, t) = 1000 b + t over a series' own steps, arrays at the stride of
  the longest series of the launch, and beyond a series' length what the device leaves there
  (posterior_means 0, order statistics and components NaN).  All five kinds of the record but the
  predictions (None: a kind the fit did not ask for); the window totals and the placebo summary have
  no time axis."""
  lengths = np.asarray(lengths)

  def run(launch):
    calls.append(launch)
    ids = np.asarray(launch[2])
    T = int(lengths[ids].max())
    t = np.arange(T)
    own = t[None, :] < lengths[ids][:, None]                                  # [n, T]
    base = np.where(own, 1000.0 * ids[:, None] + t[None, :], np.nan)
    ranks, chains = np.arange(_R)[None, :, None], np.arange(_C)[None, :, None]
    per_b = ids.astype(np.float64)
    out = dict(posterior_means=np.nan_to_num(base[:, None, :] + 0.25 * chains).astype(np.float32),
               observation_noise_scale=(per_b[:, None, None] + chains + 0.5 * np.arange(_S)).astype(np.float32),
               level_scale=(per_b[:, None, None] - chains - 0.5 * np.arange(_S)).astype(np.float32))
    dsum = dict(value_order=base[:, None, :] + 0.5 * ranks, cum_order=-base[:, None, :] - 0.5 * ranks,
                per_draw=per_b[:, None, None] + np.arange(2 * _C * _S).reshape(1, 2, _C * _S),
                per_draw_order=per_b[:, None, None] + np.arange(2 * _R).reshape(1, 2, _R))
    csum = dict(trend_mean=base + 0.125, trend_order=base[:, None, :] + 2.0 * ranks,
                regression_mean=base - 0.125, regression_order=base[:, None, :] - 2.0 * ranks,
                inclusion_prob=per_b[:, None] + np.zeros((1, _P)),
                weight_mean=-per_b[:, None] + np.zeros((1, _P)),
                weight_order=per_b[:, None, None] + np.arange(_R * _P).reshape(1, _R, _P))
    wsum = dict(per_draw=per_b[:, None, None, None] + np.arange(_W * 2 * _C * _S).reshape(1, _W, 2, _C * _S),
                per_draw_order=per_b[:, None, None, None] - np.arange(_W * 2 * _R).reshape(1, _W, 2, _R))
    plsum = {k: (i + 1) * per_b[:, None] + np.arange(_O)[None, :]
             for i, k in enumerate(lib.SUMMARY_KINDS["placebo"].whole)}
    return out, lib.SummaryRecord(effect=dsum, components=csum, windows=wsum, placebo=plsum)

  return run


def _assert_assembled(got, lengths):
  """Every series' row holds its own values over [0, T_b) and the padding beyond."""
  means, record, diag = got
  dsum, csum, wsum, plsum = record.effect, record.components, record.windows, record.placebo
  assert record.predictions is None
  B, T_max = len(lengths), max(lengths)
  assert wsum["per_draw"].shape == (B, _W, 2, _C * _S) and wsum["per_draw_order"].shape == (B, _W, 2, _R)
  assert set(plsum) == set(lib.SUMMARY_KINDS["placebo"].whole)
  assert all(v.shape == (B, _O) for v in plsum.values())
  assert means.shape == (B, T_max) and means.dtype == np.float32
  assert set(diag) == {"observation_noise_scale", "level_scale"}
  assert all(v.shape == (B, _C, _S) for v in diag.values())
  assert dsum["value_order"].shape == dsum["cum_order"].shape == (B, _R, T_max)
  assert csum["trend_order"].shape == csum["regression_order"].shape == (B, _R, T_max)
  assert csum["inclusion_prob"].shape == csum["weight_mean"].shape == (B, _P)
  assert csum["weight_order"].shape == (B, _R, _P)
  ranks = np.arange(_R)[:, None]
  for b, Tb in enumerate(lengths):
    base = 1000.0 * b + np.arange(Tb)
    np.testing.assert_array_equal(means[b, :Tb], base + 0.125)          # the mean of two chains
    assert (means[b, Tb:] == 0).all()
    np.testing.assert_array_equal(dsum["value_order"][b, :, :Tb], base + 0.5 * ranks)
    np.testing.assert_array_equal(dsum["cum_order"][b, :, :Tb], -base - 0.5 * ranks)
    np.testing.assert_array_equal(csum["trend_mean"][b, :Tb], base + 0.125)
    np.testing.assert_array_equal(csum["trend_order"][b, :, :Tb], base + 2.0 * ranks)
    np.testing.assert_array_equal(csum["regression_mean"][b, :Tb], base - 0.125)
    np.testing.assert_array_equal(csum["regression_order"][b, :, :Tb], base - 2.0 * ranks)
    for over_time in (dsum["value_order"], dsum["cum_order"], csum["trend_mean"], csum["trend_order"],
                      csum["regression_mean"], csum["regression_order"]):
      assert np.isnan(over_time[b, ..., Tb:]).all()
    np.testing.assert_array_equal(dsum["per_draw"][b], b + np.arange(2 * _C * _S).reshape(2, _C * _S))
    np.testing.assert_array_equal(dsum["per_draw_order"][b], b + np.arange(2 * _R).reshape(2, _R))
    np.testing.assert_array_equal(csum["inclusion_prob"][b], np.full(_P, float(b)))
    np.testing.assert_array_equal(csum["weight_mean"][b], np.full(_P, -float(b)))
    np.testing.assert_array_equal(csum["weight_order"][b], b + np.arange(_R * _P).reshape(_R, _P))
    np.testing.assert_array_equal(wsum["per_draw"][b],
                                  b + np.arange(_W * 2 * _C * _S).reshape(_W, 2, _C * _S))
    np.testing.assert_array_equal(wsum["per_draw_order"][b], b - np.arange(_W * 2 * _R).reshape(_W, 2, _R))
    for i, k in enumerate(lib.SUMMARY_KINDS["placebo"].whole):
      np.testing.assert_array_equal(plsum[k][b], (i + 1) * b + np.arange(_O))
    np.testing.assert_array_equal(diag["observation_noise_scale"][b],
                                  b + np.arange(_C)[:, None] + 0.5 * np.arange(_S))
    np.testing.assert_array_equal(diag["level_scale"][b], b - np.arange(_C)[:, None] - 0.5 * np.arange(_S))


@pytest.mark.parametrize("devices", [[0], [0, 1]])
@pytest.mark.parametrize("blocks,route_name,num_groups", [(0, "ragged", 1), (2, "equal_length", 3)])
def test_assembler_puts_every_series_of_a_panel_in_its_row(blocks, route_name, num_groups, devices):
  lengths = (7, 12, 7, 9, 12)
  route = batch.panel_route(float64=False, standardize_data=True, sampler="gibbs",
                            num_seasonal_blocks=blocks, P=_P, lengths=lengths)
  assert route["route"] == route_name and len(route["groups"]) == num_groups
  launches = batch.panel_launches(route, devices)
  if blocks:
    assert [ids for _, _, ids in batch.panel_launches(route, [0])] == [[0], [2], [3], [1], [4]]
  calls = []
  got = batch._assemble(launches, _fake_launch(lengths, calls), len(lengths), max(lengths))   # pylint: disable=protected-access
  assert sorted(calls) == sorted(launches) and len(calls) == len(launches)
  _assert_assembled(got, lengths)


def test_assembler_takes_a_batch_as_one_group_and_does_not_copy_a_whole_launch():
  B, T = 5, 6
  route = dict(route="equal_length", groups=[(T, list(range(B)))])      # what a batch is to the assembler
  results = {}

  def run(launch, inner=_fake_launch([T] * B, [])):
    results[tuple(launch[2])] = inner(launch)
    return results[tuple(launch[2])]

  two = batch.panel_launches(route, [0, 0])
  assert [ids for _, _, ids in two] == [[0, 1, 2], [3, 4]]
  split = batch._assemble(two, run, B, T)                               # pylint: disable=protected-access
  _assert_assembled(split, [T] * B)
  one = batch._assemble(batch.panel_launches(route, [0]), run, B, T)    # pylint: disable=protected-access
  _assert_assembled(one, [T] * B)
  for (kind, a), (_, b) in zip([*split[1].kinds(), ("diag", split[2])], [*one[1].kinds(), ("diag", one[2])]):
    if kind == "predictions":
      assert a is None and b is None
      continue
    assert list(a) == list(b)
    for k in a:
      assert a[k].dtype == b[k].dtype
      np.testing.assert_array_equal(a[k], b[k])
  np.testing.assert_array_equal(split[0], one[0])
  # one launch with all B series in order at full stride: its arrays, not copies of them
  out, whole = results[tuple(range(B))]
  for kind, arrays in whole.kinds():
    assert arrays is None or all(getattr(one[1], kind)[k] is arrays[k] for k in arrays)
  assert all(one[2][k] is out[k] for k in one[2])
  assert not any(np.shares_memory(split[1].effect[k], whole.effect[k]) for k in whole.effect)
