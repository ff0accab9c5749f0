"""ci_session_summarize_components on the device, at session level: order statistics, means and
inclusion counts of the trend, every seasonal block, the regression term and the weights against
numpy written here, from the draws fetched from the same session.

T = 70 crosses one 64-step tile with a remainder; C = 2, S = 37 gives N = 74 draws, the same on the
draw axis."""
import functools

import numpy as np
import pytest

from causalimpact import _model
from causalimpact import _native
from causalimpact import _synthetic as syn

pytestmark = pytest.mark.gpu

SCALE, SHIFT = 3.7, -12.25
QUANTILE_RANKS = [1, 2, 36, 71, 72]          # the ranks of a 95 % band over 74 draws, and the median


def _series(T, P, seed, has_slope, K):
  """Sampler inputs of one series with P design columns (the intercept is the last one)."""
  y, mask, X, _ = syn.standardize_for_sampler(*syn.make_raw_series(T, max(P - 1, 0), seed), int(0.7 * T))
  if P == 1:
    X = np.ones((T, 1))
  if K:
    y = y + 0.8 * np.sin(2 * np.pi * np.arange(T) / 7.0)
  spec = _model.series_params(np.where(mask, np.nan, y), mask, X, has_slope=has_slope,
                              num_seasonal_blocks=K)
  return y, mask, X, spec


def _pad(arrs, T, fill):
  out = np.full((len(arrs), T) + arrs[0].shape[1:], fill, arrs[0].dtype)
  for b, a in enumerate(arrs):
    out[b, :a.shape[0]] = a
  return out


def _open(lengths, P, has_slope, seasons, C=2, S=37, ragged=False, seed=(5, 9)):
  """(session, X [B, T, P] float32 as the session holds it or None, stride)."""
  K = len(seasons)
  series = [_series(T, P, 40 + 7 * b + P, has_slope, K) for b, T in enumerate(lengths)]
  T = max(lengths)
  if ragged and K:
    T = (T + 3) & ~3
  pb = _native.make_problem(T=T, P=P, has_slope=has_slope, num_warmup=3, num_results=S, num_chains=C,
                            num_series=len(lengths), seed=seed,
                            num_seasons=_model.expand_seasons(seasons, 1)[0])
  y, mask = _pad([s[0] for s in series], T, np.nan), _pad([s[1] for s in series], T, True)
  X = None if P == 0 else _pad([s[2] for s in series], T, 7.5)     # (padding rows are never read)
  par = _native.make_params([s[3] for s in series])
  sc = _model.expand_seasons(seasons, T)[1]
  if ragged:
    sess = _native.Session.ragged(pb, lengths, y, mask, X, par, season_change=sc if K else None)
  else:
    sess = _native.Session(pb, y, mask, X, sc, par)
  return sess, None if X is None else X.astype(np.float32), T


def _reference(draws, X, b, scale, shift, ranks, Tb):
  """numpy on the fetched draws of series b, over its first Tb steps: the definitions of
  include/causalimpact_amd.h.  {name: (mean, order)} with order [R, .]."""
  def stats(m):          # [N, X]
    return m.mean(axis=0), np.sort(m, axis=0)[ranks], np.abs(m).max(axis=0)

  pool = lambda a: a[b].reshape((a.shape[1] * a.shape[2],) + a.shape[3:])    # [C, S, ...] -> [N, ...]
  out = {"trend": stats(pool(draws["level"]).astype(np.float64)[:, :Tb] * scale + shift)}
  seas = pool(draws["seasonal_levels"]).astype(np.float64)
  for k in range(seas.shape[-1]):
    out[f"seasonal{k}"] = stats(seas[:, :Tb, k] * scale)
  w = pool(draws["weights"]).astype(np.float64)
  if w.shape[1]:
    acc = np.zeros((w.shape[0], Tb))
    for j in range(w.shape[1]):
      acc += X[b, :Tb, j].astype(np.float64)[None, :] * w[:, j, None]
    out["regression"] = stats(acc * scale)
    out["weights"] = stats(w)
    out["count"] = np.count_nonzero(w, axis=0)
  return out


def _check(got, ref, b, N, Tb, K, P, scale_b=None, shift_b=None, stride=None):
  """Order statistics equal, means within N 2^-52 max|x| of numpy's, inclusion counts exact; with
  `stride`: the padding convention beyond Tb."""
  def close(mean, want, peak, what):
    err = np.abs(mean - want)
    print(f"{what}: largest mean error {err.max():.3e}, smallest bound {(N * 2.0**-52 * peak).min():.3e}")
    assert (err <= N * 2.0**-52 * peak).all(), what

  pairs = [("trend", got["trend_mean"][b], got["trend_order"][b])]
  pairs += [(f"seasonal{k}", got["seasonal_mean"][b, k], got["seasonal_order"][b, k]) for k in range(K)]
  if P:
    pairs.append(("regression", got["regression_mean"][b], got["regression_order"][b]))
  for name, mean, order in pairs:
    want_mean, want_order, peak = ref[name]
    np.testing.assert_array_equal(order[:, :Tb], want_order, err_msg=name)
    close(mean[:Tb], want_mean, peak, name)
    if stride is not None and stride > Tb:
      fill = shift_b if name == "trend" else 0.0     # every latent reads 0 beyond the series' length
      assert (mean[Tb:] == fill).all() and (order[:, Tb:] == fill).all(), name
  if P:
    want_mean, want_order, peak = ref["weights"]
    np.testing.assert_array_equal(got["weight_order"][b], want_order)
    close(got["weight_mean"][b], want_mean, peak, "weights")
    np.testing.assert_array_equal(got["inclusion_prob"][b], ref["count"] / N)
    np.testing.assert_array_equal(np.rint(got["inclusion_prob"][b] * N).astype(np.int64), ref["count"])
  else:
    assert not any(k in got for k in ("regression_mean", "weight_order", "inclusion_prob"))
  if not K:
    assert "seasonal_mean" not in got


@functools.lru_cache(maxsize=None)
def _run(lengths, P, has_slope, seasons, C=2, S=37, ragged=False, ranks=tuple(QUANTILE_RANKS),
         scale=SCALE, shift=SHIFT):
  """One session: its draws, its component summary (all outputs, then a few), its design."""
  sess, X, T = _open(list(lengths), P, has_slope, seasons, C, S, ragged)
  try:
    sess.run()
    draws = sess.fetch(["level", "seasonal_levels", "weights", "posterior_means"])
    scale = np.asarray(scale, np.float64) if np.ndim(scale) else scale
    shift = np.asarray(shift, np.float64) if np.ndim(shift) else shift
    full = sess.summarize_components(scale, shift, list(ranks))
    some = sess.summarize_components(scale, shift, list(ranks),
                                     want=["trend_order"] + (["weight_mean"] if P else []))
    return draws, full, some, X, T, sess.kernel_name()
  finally:
    sess.close()


def _assert_partial_call_agrees(full, some, P):
  """Outputs passed as NULL are skipped without error; the others do not change."""
  assert sorted(some) == sorted(["trend_order"] + (["weight_mean"] if P else []))
  for k, v in some.items():
    np.testing.assert_array_equal(v, full[k], err_msg=k)


@pytest.mark.parametrize("P,has_slope,seasons", [
    (3, False, ()),                  # trend model
    (3, True, ()),                   # ... with local_linear_trend
    (3, False, ((7, 1),)),           # trend + Seasons(7): the one-block (time-parallel) route
    (2, False, ((4, 1), (3, 1))),    # two blocks: the general seasonal route, stride-2 gather
    (0, False, ()),                  # no covariates: regression and weight outputs skipped
    (0, False, ((7, 1),)),
    (17, False, ()),                 # the first width on the workgroup-wide regression block
])
def test_components_equal_numpy_on_the_fetched_draws(P, has_slope, seasons):
  draws, full, some, X, T, name = _run((70,), P, has_slope, seasons)
  print("kernel:", name)
  N, K = 74, len(seasons)
  assert full["trend_order"].shape == (1, len(QUANTILE_RANKS), 70)
  ref = _reference(draws, X, 0, SCALE, SHIFT, QUANTILE_RANKS, 70)
  _check(full, ref, 0, N, 70, K, P)
  _assert_partial_call_agrees(full, some, P)
  if P:
    assert full["weight_order"].shape == (1, len(QUANTILE_RANKS), P)
  if K:
    assert full["seasonal_order"].shape == (1, K, len(QUANTILE_RANKS), 70)


def test_rows_longer_than_16384_draws_take_the_radix_select():
  """C = 2, S = 8200: N = 16400 > 16384 rows go through summ_select_kernel."""
  C, S, T = 2, 8200, 20
  ranks = (0, 409, 410, 8199, 15989, 15990, 16399)
  draws, full, some, X, _, _ = _run((T,), 1, False, (), C=C, S=S, ranks=ranks)
  ref = _reference(draws, X, 0, SCALE, SHIFT, list(ranks), T)
  _check(full, ref, 0, C * S, T, 0, 1)
  _assert_partial_call_agrees(full, some, 1)


def test_other_scales_and_shifts():
  """scale = 1, shift = 0 (a raw-scale outcome), and a small scale under a large offset."""
  for scale, shift in ((1.0, 0.0), (0.015625, 1e6)):
    draws, full, _, X, _, _ = _run((70,), 3, False, ((7, 1),), scale=scale, shift=shift)
    _check(full, _reference(draws, X, 0, scale, shift, QUANTILE_RANKS, 70), 0, 74, 70, 1, 3)


@pytest.mark.parametrize("seasons", [(), ((7, 1),)])
def test_ragged_sessions_use_every_series_own_length(seasons):
  """Lengths 70, 130 and 200 in one launch, each series with its own scale and shift: the
  assertions of the ordinary session per series over [0, T_b); beyond T_b every latent reads 0, so
  the trend is the shift and the seasonal and regression terms are 0 (the design's padding rows,
  7.5 here, are not read)."""
  lengths, P, K = (70, 130, 200), 3, len(seasons)
  scale, shift = (3.7, 0.5, 2.0), (-12.25, 4.0, 0.0)
  draws, full, some, X, T, name = _run(lengths, P, False, seasons, ragged=True, scale=scale, shift=shift)
  print("kernel:", name)
  assert "ragged" in name and T == 200
  for b, Tb in enumerate(lengths):
    ref = _reference(draws, X, b, scale[b], shift[b], QUANTILE_RANKS, Tb)
    _check(full, ref, b, 74, Tb, K, P, scale[b], shift[b], stride=T)
  _assert_partial_call_agrees(full, some, P)


def test_component_means_add_up_to_the_posterior_mean():
  """trend + seasonal blocks + regression, means over the draws, against scale * (mean over chains
  of posterior_means) + shift.  The sampler accumulates posterior_means in float32, so the distance
  is measured on the reference side -- the same sum from numpy components of the fetched draws --
  and the device may be four times as far (its float64 means differ from numpy's by the rounding
  bound of a sum only).  Both distances are printed; no measured value is recorded here yet."""
  P, seasons = 2, ((4, 1), (3, 1))
  draws, full, _, X, _, _ = _run((70,), P, False, seasons)
  ref = _reference(draws, X, 0, SCALE, SHIFT, QUANTILE_RANKS, 70)
  target = draws["posterior_means"][0].astype(np.float64).mean(axis=0) * SCALE + SHIFT
  ref_sum = ref["trend"][0] + ref["seasonal0"][0] + ref["seasonal1"][0] + ref["regression"][0]
  dev_sum = (full["trend_mean"][0] + full["seasonal_mean"][0].sum(axis=0) + full["regression_mean"][0])
  ref_diff, dev_diff = np.abs(ref_sum - target).max(), np.abs(dev_sum - target).max()
  print(f"identity: reference side {ref_diff:.3e}, device {dev_diff:.3e}")
  assert ref_diff > 0 and dev_diff <= 4 * ref_diff


def test_errors_are_reported_before_any_device_work():
  sess, _, _ = _open([70], 3, False, ())
  try:
    with pytest.raises(_native.NativeError, match="needs a finished ci_session_run"):
      sess.summarize_components(1.0, 0.0, [0, 73])
    sess.run()
    with pytest.raises(_native.NativeError, match=r"rank 74 out of range \[0, 74\)"):
      sess.summarize_components(1.0, 0.0, [0, 74])
    with pytest.raises(_native.NativeError, match="rank -1 out of range"):
      sess.summarize_components(1.0, 0.0, [-1])
    assert sess.summarize_components(1.0, 0.0, [0, 73])["trend_order"].shape == (1, 2, 70)
  finally:
    sess.close()
