"""Batched HMC: B series x C chains of the hmc_kernel in one launch (ci_ll_session_create_batch).

Low level: series b of a batch is bit for bit the one-series session on series b (shared streams)
or on its series key (default streams), whatever the batch is split into, and the on-device summary
equals `summarize_draws` on the fetched trajectories.  Public API: `fit_causalimpact_batch(
sampler="hmc")` equals `fit_causalimpact(sampler="hmc")` per series on both of its routes."""
import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _hmc
from causalimpact import _model
from causalimpact import _native
from causalimpact import _synthetic as syn
from causalimpact import batch
from causalimpact import causalimpact_lib as lib

pytestmark = pytest.mark.gpu

SEED = (3, 4)
FIELDS = ("level", "slope", "posterior_trajectories", "posterior_means", "observation_noise_scale",
          "level_scale", "slope_scale", "weights")


def _series(B, T, P, seed=20):
  """B standardised series [B, T] (pre-period 70 %), designs [B, T, P] (P - 1 covariates and the
  intercept; None for P = 0) and their priors."""
  ys, ms, Xs, specs = [], [], [], []
  for b in range(B):
    y, mask, X, _ = syn.make_sampler_inputs(T, max(P - 1, 1), seed + b)
    X = X[:, :P] if P else None
    ys.append(y)
    ms.append(mask)
    Xs.append(X)
    specs.append(_model.series_params(y, mask, X))
  return np.stack(ys), np.stack(ms), (np.stack(Xs) if P else None), specs


def _batch_fit(y, mask, X, specs, *, has_slope, prior, C, W, S, NL, series_offset=0, shared=True):
  B, T = y.shape
  P = 0 if X is None else X.shape[2]
  pb = _native.make_problem(T=T, P=P, has_slope=has_slope, num_warmup=0, num_results=1, num_series=B,
                            seed=SEED, series_offset=series_offset,
                            flags=_native.FLAG_SHARED_SERIES_STREAMS if shared else 0)
  sess = _native.BatchLogLikSession(pb, _native.make_params(specs), y, mask, X)
  try:
    sess.hmc_run(num_chains=C, num_warmup=W, num_results=S, num_leapfrog=NL, seed=SEED, prior=prior)
    draws, acc, eps, arrs = sess.hmc_fetch()
    name = sess.kernel_name()
  finally:
    sess.close()
  return draws, acc, eps, arrs, name


def _single_fit(y, mask, X, spec, *, has_slope, prior, C, W, S, NL, seed=SEED):
  T = y.shape[0]
  P = 0 if X is None else X.shape[1]
  pb = _native.make_problem(T=T, P=P, has_slope=has_slope, num_warmup=0, num_results=1, seed=seed)
  sess = _native.LogLikSession(pb, _native.make_params([spec]), y, mask, X, max_evals=8)
  try:
    sess.hmc_run(num_chains=C, num_warmup=W, num_results=S, num_leapfrog=NL, seed=seed, prior=prior)
    draws, acc, eps, arrs = sess.hmc_fetch()
    name = sess.kernel_name()
  finally:
    sess.close()
  return draws, acc, eps, arrs, name


def _assert_series_equal(batch_fit, b, single_fit, has_slope):
  draws, acc, eps, arrs, name = batch_fit
  d1, a1, e1, o1, n1 = single_fit
  assert name == n1
  np.testing.assert_array_equal(draws[b], d1)
  np.testing.assert_array_equal(acc[b], a1)
  np.testing.assert_array_equal(eps[b], e1)
  for k in FIELDS:
    if k == "slope" and not has_slope:
      continue
    np.testing.assert_array_equal(arrs[k][b], o1[k][0], err_msg=k)


# P = 0, 10 and 60 (the build sized for 128 columns); T = 100 (L = 1), 1000 (L = 4) and 4096
# (L = 16); both priors, both trends
CASES = [
    (100, 0, "slab", False),
    (100, 10, "horseshoe", True),
    (1000, 10, "slab", True),
    (4096, 10, "horseshoe", False),
    (4096, 0, "slab", True),
    (300, 60, "slab", False),
    (300, 60, "horseshoe", True),
]


@pytest.mark.parametrize("T,P,prior,has_slope", CASES)
def test_batch_series_equal_single_series_sessions_bit_for_bit(T, P, prior, has_slope):
  B, kw = 5, dict(has_slope=has_slope, prior=prior, C=2, W=30, S=12, NL=4)
  y, mask, X, specs = _series(B, T, P)
  got = _batch_fit(y, mask, X, specs, **kw)
  assert got[0].shape == (B, 2, 12, 3 + P) and got[1].shape == (B, 2)
  if P > 52:
    assert got[4].endswith(",wide>")
  for b in range(B):
    one = _single_fit(y[b], mask[b], None if X is None else X[b], specs[b], **kw)
    _assert_series_equal(got, b, one, has_slope)
  assert np.all(np.isfinite(got[3]["posterior_means"]))
  # different data, different draws
  assert not np.array_equal(got[0][0], got[0][1])


def test_default_streams_key_each_series_and_splits_do_not_matter():
  B, T, P = 5, 200, 4
  kw = dict(has_slope=True, prior="slab", C=2, W=30, S=10, NL=4)
  y, mask, X, specs = _series(B, T, P, seed=40)
  whole = _batch_fit(y, mask, X, specs, shared=False, **kw)
  for b in range(B):
    key = _native.series_stream_key(SEED, b)
    one = _single_fit(y[b], mask[b], X[b], specs[b], seed=key, **kw)
    _assert_series_equal(whole, b, one, True)
  # two half-batches that keep the series ids equal the whole batch
  lo = _batch_fit(y[:2], mask[:2], X[:2], specs[:2], shared=False, series_offset=0, **kw)
  hi = _batch_fit(y[2:], mask[2:], X[2:], specs[2:], shared=False, series_offset=2, **kw)
  for i in range(3):
    part = np.concatenate([lo[i], hi[i]], axis=0)
    np.testing.assert_array_equal(part, whole[i])
  for k in FIELDS:
    np.testing.assert_array_equal(np.concatenate([lo[3][k], hi[3][k]], axis=0), whole[3][k], err_msg=k)
  # identical twins get different draws on their own keys
  twins = _batch_fit(np.stack([y[1], y[1]]), np.stack([mask[1], mask[1]]), np.stack([X[1], X[1]]),
                     [specs[1]] * 2, shared=False, **kw)
  assert not np.array_equal(twins[0][0], twins[0][1])


def test_hmc_summarize_equals_summarize_draws():
  B, T, P, C, S = 3, 150, 3, 2, 40
  y, mask, X, specs = _series(B, T, P, seed=60)
  pb = _native.make_problem(T=T, P=P, has_slope=False, num_warmup=0, num_results=1, num_series=B,
                            seed=SEED)
  sess = _native.BatchLogLikSession(pb, _native.make_params(specs), y, mask, X)
  rng = np.random.default_rng(1)
  scale, shift = rng.uniform(0.5, 2.0, B), rng.normal(size=B)
  observed = rng.normal(size=(B, T))
  flags = np.zeros(T, np.uint8)
  flags[100:] = 1
  flags[105:140] |= 2
  ranks = lib._summary_ranks(C * S, (0.05, 0.95))   # pylint: disable=protected-access
  try:
    sess.hmc_run(num_chains=C, num_warmup=20, num_results=S, num_leapfrog=4, seed=SEED)
    _, _, _, arrs = sess.hmc_fetch(["posterior_trajectories"])
    got = sess.summarize(scale, shift, observed, flags, ranks)
  finally:
    sess.close()
  tr = arrs["posterior_trajectories"]
  for b in range(B):
    want = _native.summarize_draws(tr[b].reshape(C * S, T), scale[b], shift[b], observed[b], flags,
                                   ranks)
    for k, v in want.items():
      np.testing.assert_array_equal(got[k][b], v, err_msg=k)


def test_batch_refuses_single_series_calls():
  y, mask, X, specs = _series(2, 60, 2)
  pb = _native.make_problem(T=60, P=2, has_slope=False, num_warmup=0, num_results=1, num_series=2)
  sess = _native.BatchLogLikSession(pb, _native.make_params(specs), y, mask, X)
  try:
    with pytest.raises(_native.NativeError, match="one series per session"):
      sess.evaluate(np.ones((1, 5)))
    with pytest.raises(_native.NativeError, match="one series per session"):
      sess.draw_latents(np.ones((1, 5)), SEED)
  finally:
    sess.close()


# ---- public API ----

def _frames(B, T, p, seed=0):
  idx = pd.date_range("2021-01-04", periods=T, freq="D")
  out = []
  for b in range(B):
    y, X = syn.make_raw_series(T, p, seed + b, effect=5.0 + b)
    out.append(pd.DataFrame(np.column_stack([y, X]), index=idx,
                            columns=["y"] + [f"x{j}" for j in range(p)]))
  out[1].iloc[[3, 17], 0] = np.nan          # missing pre-period outcomes
  return out


def _assert_equal_fits(got, b, one, name):
  np.testing.assert_allclose(got.summary.loc[name].to_numpy(float), one.summary.to_numpy(float),
                             rtol=2e-5, atol=1e-7)
  mine = got[b]
  assert list(mine.series.columns) == list(one.series.columns)
  num = [c for c in one.series.columns if one.series[c].dtype.kind == "f"]
  np.testing.assert_allclose(mine.series[num].to_numpy(float), one.series[num].to_numpy(float),
                             rtol=2e-5, atol=1e-6, equal_nan=True)
  assert ci.summary(mine) == ci.summary(one)


@pytest.mark.parametrize("prior", ["slab", "horseshoe"])
def test_hmc_batch_equals_separate_fits(prior):
  T, B = 100, 4
  frames = _frames(B, T, 2)
  idx = frames[0].index
  pre, post = (idx[0], idx[69]), (idx[72], idx[95])
  opts = ci.InferenceOptions(num_results=60, num_warmup_steps=40, num_chains=2, sampler="hmc",
                             hmc_prior=prior)
  names = [f"geo{b}" for b in range(B)]
  got = ci.fit_causalimpact_batch(frames, pre, post, alpha=0.1, seed=5, inference_options=opts,
                                  names=names, shared_streams=True)
  assert type(got) is batch.CausalImpactBatchAnalysis and got.summary.shape == (2 * B, 15)
  for b, f in enumerate(frames):
    one = ci.fit_causalimpact(f, pre, post, alpha=0.1, seed=5, inference_options=opts)
    _assert_equal_fits(got, b, one, names[b])
  assert set(got.diagnostics) == {"split_rhat", "ess_bulk", "ess_tail"}
  if prior == "horseshoe":
    return
  # default streams: series 0 still equals its single fit, identical twins differ, diagnostics
  ind = ci.fit_causalimpact_batch(frames, pre, post, alpha=0.1, seed=5, inference_options=opts,
                                  names=names)
  np.testing.assert_allclose(ind.summary.loc["geo0"].to_numpy(float),
                             got.summary.loc["geo0"].to_numpy(float), rtol=2e-5, atol=1e-7)
  assert not np.allclose(ind.summary.loc["geo3"].to_numpy(float),
                         got.summary.loc["geo3"].to_numpy(float), rtol=1e-6)
  assert set(ind.diagnostics_of(2)) == {"split_rhat", "ess_bulk", "ess_tail"}
  assert np.isfinite(ind.diagnostics_of(2)["split_rhat"]["observation_noise_scale"])
  twins = ci.fit_causalimpact_batch([frames[1], frames[1]], pre, post, alpha=0.1, seed=5,
                                    inference_options=opts)
  assert not np.allclose(twins.summary.loc[0].to_numpy(float), twins.summary.loc[1].to_numpy(float),
                         rtol=1e-6)
  # sharding over two devices (here: device 0 twice) and launches split under a small HBM budget
  # change nothing
  two = ci.fit_causalimpact_batch(frames, pre, post, alpha=0.1, seed=5, names=names,
                                  inference_options=ci.InferenceOptions(
                                      num_results=60, num_warmup_steps=40, num_chains=2,
                                      sampler="hmc", devices=[0, 0]))
  pd.testing.assert_frame_equal(two.summary, ind.summary)
  saved = _hmc.HMC_BATCH_HBM_BYTES
  try:
    _hmc.HMC_BATCH_HBM_BYTES = _hmc.hmc_batch_bytes_per_series(T, 3, 2, 60) * 2   # 2 per launch
    split = ci.fit_causalimpact_batch(frames, pre, post, alpha=0.1, seed=5, inference_options=opts,
                                      names=names)
  finally:
    _hmc.HMC_BATCH_HBM_BYTES = saved
  pd.testing.assert_frame_equal(split.summary, ind.summary)
  for b in range(B):
    pd.testing.assert_frame_equal(split[b].series, ind[b].series)


@pytest.mark.parametrize("route", ["seasonal", "vi"])
def test_hmc_batch_series_by_series_routes_equal_separate_fits(route):
  T, B = 112, 3
  frames = _frames(B, T, 1, seed=30)
  idx = frames[0].index
  for b, f in enumerate(frames):
    f["y"] += 3.0 * np.sin(2 * np.pi * (np.arange(T) + b) / 7.0)
  pre, post = (idx[0], idx[83]), (idx[84], idx[-1])
  opts = ci.InferenceOptions(num_results=40, num_warmup_steps=30, num_chains=1, sampler="hmc",
                             hmc_init="vi" if route == "vi" else "gibbs")
  mo = ci.ModelOptions(seasons=[ci.Seasons(num_seasons=7)]) if route == "seasonal" else ci.ModelOptions()
  got = ci.fit_causalimpact_batch(frames, pre, post, seed=8, inference_options=opts, model_options=mo,
                                  shared_streams=True)
  assert isinstance(got, batch.PerSeriesBatchAnalysis)
  for b, f in enumerate(frames):
    one = ci.fit_causalimpact(f, pre, post, seed=8, inference_options=opts, model_options=mo)
    _assert_equal_fits(got, b, one, b)
  # default streams: series b on the key of series id b
  ind = ci.fit_causalimpact_batch(frames, pre, post, seed=8, inference_options=opts, model_options=mo)
  one = ci.fit_causalimpact(frames[2], pre, post, seed=_native.series_stream_key(lib._sanitize_seed(8), 2),   # pylint: disable=protected-access
                            inference_options=opts, model_options=mo)
  _assert_equal_fits(ind, 2, one, 2)


def test_hmc_batch_full_size():
  # cfg5's shape (512 series, T = 500, 5 covariates, 1 chain, 15 leapfrog steps) with few draws
  B, T, p = 512, 500, 5
  rng = np.random.default_rng(3)
  X = rng.normal(size=(B, T, p))
  y = X @ rng.normal(size=p) + np.cumsum(rng.normal(scale=0.1, size=(B, T)), axis=1)
  y[:, 350:] += 2.0
  v = np.concatenate([y[:, :, None], X], axis=2)
  got = ci.fit_causalimpact_batch(v, (0, 349), (350, T - 1), seed=1,
                                  inference_options=ci.InferenceOptions(
                                      num_results=20, num_warmup_steps=20, sampler="hmc"))
  assert got.summary.shape == (2 * B, 15)
  assert np.isfinite(got.summary.drop(columns=["p_value", "alpha"]).to_numpy(float)).all()
  assert got.diagnostics is None
