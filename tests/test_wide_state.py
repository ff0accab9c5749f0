"""Seasonal states of 65-256 components (csrc/ci_seasonal_mw.h, the multi-wavefront build of the
sequential seasonal kernel): the widened float64 oracle (tests/wide_oracle.py) on the CPU, per-draw
parity with it on the GPU, the route invariants, an hourly end-to-end fit and the limits."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _model
from causalimpact import _native
from causalimpact import _synthetic as syn
from oracle import ci_oracle as orc

import wide_oracle

MW = _native.FLAG_MULTIWAVE_SEASONAL


def _inputs(T, p, has_slope, seasons, seed=7, edit=None):
  """The inputs of test_gpu_gibbs.py's seasonal per-draw parity: a weekly wave plus noise, and
  masked pre-period steps.  `edit` maps that mask (a copy) to the one used."""
  y, mask, X, _ = syn.make_sampler_inputs(T, p, seed)
  rng = np.random.default_rng(0)
  y = y + 0.8 * np.sin(2 * np.pi * np.arange(T) / 7.0) + 0.1 * rng.normal(size=T)
  if T >= 100:
    mask = mask.copy()
    mask[[2, 3, 40, T // 2]] = True
  if edit is not None:
    mask = np.asarray(edit(mask.copy()), bool)
  spec = orc.default_spec(y, mask, X, has_slope=bool(has_slope), seasons=seasons)
  return y, mask, X, spec


def _dfull(has_slope, seasons):
  return 1 + has_slope + sum(int(s[0]) for s in seasons)


# ---------------------------------------------------------------------------------------------
# CPU: the widened oracle
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,p,has_slope,seasons", [
    (300, 2, 0, ((52, 1),)),                                                       # D = 53
    (250, 0, 1, ((62, 1),)),                                                       # D = 64
    (300, 0, 0, ((4, (2, 1, 1, 1)), (7, 1), (6, ((2, 2, 1, 1, 1, 1), (2, 2, 1, 1, 1, 1))))),
    (120, 4, 1, ((7, 1),)),
])
def test_wide_oracle_reproduces_the_stock_oracle_bit_for_bit(T, p, has_slope, seasons):
  _wide_equals_stock(T, p, has_slope, seasons)


def _gap(a, b):
  """A mask edit: pre-period steps a..b-1 masked as well."""
  def edit(m):
    m[a:b] = True
    return m
  return edit


@pytest.mark.parametrize("T,p,has_slope,seasons,edit", [
    (200, 59, 1, ((7, 1), (12, 2)), None),                     # P = 60: the P > 52 regression block
    (150, 52, 0, ((30, 1),), _gap(20, 70)),                    # P = 53 and a 50-step gap
    (240, 0, 0, ((7, 3), (30, 2)), _gap(30, 75)),              # a 45-step gap over season changes
    (240, 3, 1, ((60, 4),), _gap(41, 90)),                     # ... of a 4-step season, with a slope
])
def test_wide_oracle_reproduces_the_stock_oracle_with_many_columns_and_long_gaps(T, p, has_slope,
                                                                                 seasons, edit):
  """What the BIGP and long-gap GPU cases of test_wide_state_builds.py are compared against."""
  _wide_equals_stock(T, p, has_slope, seasons, edit)


def _wide_equals_stock(T, p, has_slope, seasons, edit=None):
  assert _dfull(has_slope, seasons) <= 64
  y, mask, X, spec = _inputs(T, p, has_slope, seasons, edit=edit)
  kw = dict(num_results=4, num_warmup=0, seed=(2, 6))
  want = orc.fit_gibbs(y, mask, X, spec, **kw)
  got = wide_oracle.fit_gibbs(y, mask, X, spec, **kw)
  assert want.keys() == got.keys()
  for k in want:
    np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_wide_oracle_runs_an_hour_of_week_model():
  T, seasons = 400, ((168, 1),)
  assert _dfull(1, seasons) == 170
  y, mask, X, spec = _inputs(T, 2, 1, seasons)
  with pytest.raises(RuntimeError):          # the stock oracle holds 64 components
    orc.fit_gibbs(y, mask, X, spec, num_results=1, num_warmup=0, seed=(2, 6))
  got = wide_oracle.fit_gibbs(y, mask, X, spec, num_results=4, num_warmup=0, seed=(2, 6))
  for k, v in got.items():
    assert np.isfinite(v).all(), k
  assert got["seasonal"].shape == (4, T, 1)
  assert np.abs(got["seasonal"]).max() > 0


def test_state_wider_than_256_is_refused_before_any_device_call():
  L = _native.load()
  pb = _native.make_problem(T=40, P=0, has_slope=1, num_seasons=(255,), num_warmup=1, num_results=2)
  assert _dfull(1, ((255, 1),)) == 257
  y = np.zeros((1, 40), np.float32)
  m = np.zeros((1, 40), np.uint8)
  sc = np.zeros((1, 40), np.uint8)
  params = _native.make_params([dict(orc.default_spec(y[0] + np.arange(40) * 0.01, m[0].astype(bool), None,
                                                      has_slope=True, seasons=((255, 1),)))])
  out = _native.Outputs()
  rc = L.ci_fit_gibbs(C.byref(pb), y.ctypes.data, m.ctypes.data, None, sc.ctypes.data, params, C.byref(out))
  assert rc != 0
  msg = L.ci_last_error()
  assert b"too wide" in msg and b"257 > 256" in msg


# ---------------------------------------------------------------------------------------------
# GPU: the multi-wavefront kernel
# ---------------------------------------------------------------------------------------------

def _ragged(n):
  """A tuple of tuples of season lengths over two cycles (1 or 2 steps per season)."""
  a = tuple(1 + (s % 2) for s in range(n))
  b = tuple(2 - (s % 3 == 0) for s in range(n))
  return (a, b)


def _mw_name(gws, bigp):
  """Session.kernel_name() of a build of the multi-wavefront kernel."""
  return f"ci::gibbs_seasonal_kernel<{str(bool(gws)).lower()},{str(bool(bigp)).lower()},4> (multi-wave)"


def _gpu_vs_oracle(T, p, has_slope, seasons, flags=0, oracle=None, kernel=None, edit=None):
  """Four iterations of one chain on the device against the oracle, per draw; `kernel` is the
  Session.kernel_name() the case must run on."""
  y, mask, X, spec = _inputs(T, p, has_slope, seasons, edit=edit)
  counts, flg = _model.expand_seasons(seasons, T)
  S = 4
  pb = _native.make_problem(T=T, P=spec["P"], has_slope=has_slope, num_seasons=counts,
                            num_warmup=0, num_results=S, seed=(2, 6), flags=flags)
  s = _native.Session(pb, y[None], mask[None], None if X is None else X[None], flg,
                      _native.make_params([spec]))
  try:
    if kernel is not None:
      assert s.kernel_name() == kernel
    s.run()
    got = s.fetch()
  finally:
    s.close()
  w = (oracle or wide_oracle.fit_gibbs)(y, mask, X, spec, num_results=S, num_warmup=0, seed=(2, 6))
  _assert_draws_match(got, 0, 0, w, has_slope, spec["P"])
  assert got["seasonal_levels"].shape == (1, 1, S, T, len(seasons))
  return got, w


def _assert_draws_match(got, b, c, w, has_slope, P):
  """Series b, chain c of a device fit against one oracle chain, per draw."""
  # the tolerances of test_gpu_gibbs.py::test_seasonal_first_iterations_match_oracle_per_draw
  np.testing.assert_allclose(got["level"][b, c], w["level"], atol=5e-3)
  np.testing.assert_allclose(got["seasonal_levels"][b, c], w["seasonal"], atol=5e-3)
  np.testing.assert_allclose(got["seasonal_drift_scales"][b, c], w["drift_scales"], rtol=2e-2)
  np.testing.assert_allclose(got["observation_noise_scale"][b, c], w["obs_scale"], rtol=5e-3)
  np.testing.assert_allclose(got["level_scale"][b, c], w["level_scale"], rtol=5e-3)
  if has_slope:
    np.testing.assert_allclose(got["slope"][b, c], w["slope"], atol=5e-3)
  if P:
    np.testing.assert_allclose(got["weights"][b, c], w["weights"], atol=5e-3)
  np.testing.assert_allclose(got["posterior_trajectories"][b, c], w["trajectories"], atol=1e-2)
  np.testing.assert_allclose(got["posterior_means"][b, c], w["pred_mean"], atol=5e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("T,p,has_slope,seasons", [
    (400, 2, 1, ((168, 1),)),                        # hour-of-week + trend: D = 170, P = 3
    (300, 0, 0, ((7, 1), (60, 2))),                  # D = 68
    (400, 19, 0, ((24, 1), (52, 3))),                # D = 77, P = 20: the LDS regression block
    (500, 1, 0, ((80, _ragged(80)),)),               # ragged tuple-of-tuples steps, one wide block
    (600, 2, 1, ((254, 1),)),                        # D = 256: the top of the range
])
def test_wide_state_first_iterations_match_the_widened_oracle_per_draw(T, p, has_slope, seasons):
  assert 64 < _dfull(has_slope, seasons) <= 256
  # every one of these series is too long for LDS: the arrays over time live in the workspace
  _gpu_vs_oracle(T, p, has_slope, seasons, kernel=_mw_name(True, False))


@pytest.mark.gpu
@pytest.mark.parametrize("T,p,has_slope,seasons", [
    (300, 3, 0, ((52, 1),)),                                                       # D = 53
    (250, 0, 1, ((62, 1),)),                                                       # D = 64
    (300, 0, 0, ((4, (2, 1, 1, 1)), (7, 1), (6, ((2, 2, 1, 1, 1, 1), (2, 2, 1, 1, 1, 1))))),
])
def test_multiwave_flag_on_narrow_states_matches_the_oracle_per_draw(T, p, has_slope, seasons):
  _gpu_vs_oracle(T, p, has_slope, seasons, flags=MW, oracle=orc.fit_gibbs)


def _fit_170(num_chains, chain_offset=0, T=400, S=6):
  seasons = ((168, 1),)
  y, mask, X, spec = _inputs(T, 2, 1, seasons)
  counts, flg = _model.expand_seasons(seasons, T)
  pb = _native.make_problem(T=T, P=spec["P"], has_slope=1, num_seasons=counts, num_warmup=3,
                            num_results=S, num_chains=num_chains, chain_offset=chain_offset, seed=(4, 9))
  return _native.fit_gibbs(pb, y[None], mask[None], X[None], flg, _native.make_params([spec]))


_KEYS = ("observation_noise_scale", "level_scale", "seasonal_drift_scales", "weights", "level",
         "slope", "seasonal_levels", "posterior_trajectories", "posterior_means")


@pytest.mark.gpu
def test_wide_state_chains_do_not_depend_on_the_launch():
  eight = _fit_170(8)
  one = _fit_170(1)
  shard = _fit_170(3, chain_offset=5)
  for k in _KEYS:
    np.testing.assert_array_equal(one[k][0, 0], eight[k][0, 0], err_msg=k)
    np.testing.assert_array_equal(shard[k][0], eight[k][0, 5:8], err_msg=k)
  assert not np.array_equal(eight["level"][0, 0], eight["level"][0, 1])


def _hourly_frames(B, weeks_pre=8, weeks_post=1, effect=0.0, seed=0):
  T = 168 * (weeks_pre + weeks_post)
  idx = pd.date_range("2024-01-01", periods=T, freq="h")
  hw = np.arange(T) % 168
  pattern = 2.0 * np.sin(2 * np.pi * hw / 24.0) + 1.0 * (hw // 24 >= 5) + 0.5 * np.cos(2 * np.pi * hw / 168.0)
  pattern = pattern - pattern[:168].mean()
  frames = []
  for b in range(B):
    rng = np.random.default_rng(seed + b)
    x = 10.0 + np.cumsum(rng.normal(0, 0.05, T))
    y = 5.0 + 0.8 * x + pattern + rng.normal(0, 0.3, T)
    y[168 * weeks_pre:] += effect
    frames.append(pd.DataFrame({"y": y, "x": x}, index=idx))
  pre = (idx[0], idx[168 * weeks_pre - 1])
  post = (idx[168 * weeks_pre], idx[-1])
  return frames, pre, post, pattern


@pytest.mark.gpu
def test_wide_state_batch_equals_separate_fits():
  frames, pre, post, _ = _hourly_frames(3, weeks_pre=3, weeks_post=1, effect=1.0, seed=40)
  kw = dict(seed=8, inference_options=ci.InferenceOptions(num_results=60, num_warmup_steps=20),
            model_options=ci.ModelOptions(seasons=[ci.Seasons(num_seasons=168)]))
  got = ci.fit_causalimpact_batch(frames, pre, post, shared_streams=True, **kw)
  for b, f in enumerate(frames):
    one = ci.fit_causalimpact(f, pre, post, **kw)
    np.testing.assert_allclose(got.summary.loc[b].to_numpy(float), one.summary.to_numpy(float),
                               rtol=2e-5, atol=1e-7)


@pytest.mark.gpu
def test_hour_of_week_model_end_to_end():
  frames, pre, post, pattern = _hourly_frames(1, effect=1.5, seed=3)
  df = frames[0]
  res = ci.fit_causalimpact(df, pre, post, seed=1,
                            inference_options=ci.InferenceOptions(num_chains=8),
                            model_options=ci.ModelOptions(seasons=[ci.Seasons(num_seasons=168)]))
  for name in ("series", "summary"):
    frame = getattr(res, name).select_dtypes("number")
    assert np.isfinite(frame.to_numpy(float)[~np.isnan(frame.to_numpy(float))]).all()
  sl = np.asarray(res.posterior_samples.seasonal_levels)
  assert np.isfinite(sl).all()
  n_pre = 168 * 8
  est = sl.mean(axis=0)[:n_pre, 0]
  assert np.corrcoef(est, pattern[:n_pre])[0, 1] > 0.95
  assert res.summary.loc["average", "p_value"] < 0.05
  text = ci.summary(res)
  assert "Posterior tail-area probability" in text
  assert len(ci.summary(res, output_format="report")) > 0


@pytest.mark.gpu
def test_wide_state_limits_on_the_other_paths():
  frames, pre, post, _ = _hourly_frames(1, weeks_pre=2, weeks_post=1)
  df = frames[0]
  mo = ci.ModelOptions(seasons=[ci.Seasons(num_seasons=168)])
  with pytest.raises(Exception, match="dtype=float64"):
    ci.fit_causalimpact(df, pre, post, model_options=mo,
                        data_options=ci.DataOptions(dtype=np.float64),
                        inference_options=ci.InferenceOptions(num_results=10))
  with pytest.raises(Exception, match="hmc"):
    ci.fit_causalimpact(df, pre, post, model_options=mo,
                        inference_options=ci.InferenceOptions(num_results=10, sampler="hmc"))
  with pytest.raises(Exception, match="257 > 256"):
    ci.fit_causalimpact(df, pre, post, model_options=ci.ModelOptions(seasons=[ci.Seasons(num_seasons=256)]),
                        inference_options=ci.InferenceOptions(num_results=10))


@pytest.mark.gpu
def test_float64_and_hmc_take_64_components_and_refuse_65():
  """The one-wavefront limits of the float64 and HMC paths, at their edge."""
  frames, pre, post, _ = _hourly_frames(1, weeks_pre=1, weeks_post=1)
  df = frames[0]
  at_64 = ci.ModelOptions(seasons=[ci.Seasons(num_seasons=63)])
  at_65 = ci.ModelOptions(seasons=[ci.Seasons(num_seasons=64)])
  f64 = ci.DataOptions(dtype=np.float64)
  res = ci.fit_causalimpact(df, pre, post, model_options=at_64, data_options=f64,
                            inference_options=ci.InferenceOptions(num_results=10))
  assert np.isfinite(np.asarray(res.posterior_samples.seasonal_levels)).all()
  with pytest.raises(Exception, match=r"65 > 64 \(dtype=float64"):
    ci.fit_causalimpact(df, pre, post, model_options=at_65, data_options=f64,
                        inference_options=ci.InferenceOptions(num_results=10))
  hmc = ci.InferenceOptions(num_results=10, num_warmup_steps=10, sampler="hmc")
  res = ci.fit_causalimpact(df, pre, post, model_options=at_64, inference_options=hmc)
  assert np.isfinite(np.asarray(res.posterior_samples.seasonal_levels)).all()
  with pytest.raises(Exception, match=r"65 > 64 \(the log-likelihood and sampler=\"hmc\""):
    ci.fit_causalimpact(df, pre, post, model_options=at_65, inference_options=hmc)
