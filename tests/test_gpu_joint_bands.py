"""ci_session_summarize_paths / ci_ll_session_summarize_paths on the device -- the moments of the
prediction's and the cumulative effect's paths over sub-windows, and every draw's largest
standardised excursion -- against `_native.path_excursions_host` on the trajectories fetched from the
same session.

center within 1e-10 * max_n |x[n, t]| and spread within 1e-10 relative: the device adds the draws in
its own order, a summation error of at most N * 2^-53 = 7e-12 for N <= 65536.  GIVEN the device's
center and spread, excursion, excursion_order, observed_excursion, at and exceed are the host loop's
bit for bit.

T = 67 is one 64-step tile and a remainder with rows that are not 16-byte aligned, T = 72 the float4
loads; C = 2, S = 35 gives N = 70 draws: one draw tile and a second of 6 rows."""
import functools
import warnings

import numpy as np
import pytest

from causalimpact import _model
from causalimpact import _native
from causalimpact import batch
from causalimpact import _synthetic as syn

pytestmark = pytest.mark.gpu

RANKS = [0, 34, 65, 66, 69]
SCALE, SHIFT = (3.7, -0.5, 2.0), (-12.25, 4.0, 0.0)
# (first, count): the post-period, across the tile edge, the last step, an empty window, two that
# overlap; the observations of steps 52 and 62 are missing
WINDOWS = ((40, 27), (60, 7), (66, 1), (55, 0), (45, 10), (50, 12))
BITWISE = ("excursion", "excursion_order", "observed_excursion", "at", "exceed")


def _series(T, P, seed, seasons):
  y, mask, X, _ = syn.standardize_for_sampler(*syn.make_raw_series(T, P - 1, seed), int(0.7 * T))
  if seasons:
    y = y + 0.8 * np.sin(2 * np.pi * np.arange(T) / 7.0)
  spec = _model.series_params(np.where(mask, np.nan, y), mask, X, num_seasonal_blocks=len(seasons))
  return y, mask, X, spec


def _pad(arrs, T, fill):
  out = np.full((len(arrs), T) + arrs[0].shape[1:], fill, arrs[0].dtype)
  for b, a in enumerate(arrs):
    out[b, :a.shape[0]] = a
  return out


def _open(lengths, seasons=(), ragged=False, C_=2, S=35, P=2):
  series = [_series(T, P, 40 + 7 * b, seasons) for b, T in enumerate(lengths)]
  T = max(lengths)
  if ragged and seasons:
    T = (T + 3) & ~3
  pb = _native.make_problem(T=T, P=P, has_slope=False, num_warmup=3, num_results=S, num_chains=C_,
                            num_series=len(lengths), seed=(5, 9),
                            num_seasons=_model.expand_seasons(seasons, 1)[0])
  y, mask = _pad([s[0] for s in series], T, np.nan), _pad([s[1] for s in series], T, True)
  X = _pad([s[2] for s in series], T, 7.5)                  # (padding rows are never read)
  par = _native.make_params([s[3] for s in series])
  sc = _model.expand_seasons(seasons, T)[1]
  if ragged:
    return _native.Session.ragged(pb, list(lengths), y, mask, X, par, season_change=sc if seasons else None), T
  return _native.Session(pb, y, mask, X, sc, par), T


def _observed(B, T, holes):
  obs = np.random.default_rng(17).normal(size=(B, T)) * 3.0 + 10.0
  for b, steps in enumerate(holes):
    obs[b, list(steps)] = np.nan
  return obs


def _tables(windows):
  return (np.array([[f for f, _ in ws] for ws in windows], np.int32),
          np.array([[c for _, c in ws] for ws in windows], np.int32))


@functools.lru_cache(maxsize=None)
def _run(lengths, windows, holes, seasons=(), ragged=False, C_=2, S=35):
  """One session: its fetched trajectories [B, N, T], `summarize_paths` of the per-series `windows`,
  and the inputs."""
  sess, T = _open(lengths, seasons, ragged, C_, S)
  B = len(lengths)
  try:
    sess.run()
    traj = sess.fetch(["posterior_trajectories"])["posterior_trajectories"].reshape(B, C_ * S, T)
    obs = _observed(B, T, holes)
    first, count = _tables(windows)
    got = sess.summarize_paths(SCALE[:B], SHIFT[:B], obs, first, count, RANKS)
    return traj, got, obs, first, count, sess.kernel_name()
  finally:
    sess.close()


def _check(run, what, scale=SCALE, shift=SHIFT):
  traj, got, obs, first, count, name = run
  B, N, T = traj.shape
  W = first.shape[1]
  print(f"{what}: kernel {name}, trajectories {traj.shape}, windows {W}")
  assert traj.dtype == np.float32
  assert set(got) == set(_native.PATH_OUTPUTS)
  assert got["center"].shape == got["spread"].shape == (B, W, 2, T)
  assert got["excursion"].shape == (B, W, 2, N) and got["excursion_order"].shape == (B, W, 2, len(RANKS))
  assert got["at"].dtype == got["exceed"].dtype == np.int32
  own = _native.path_excursions_host(traj, scale[:B], shift[:B], obs, first, count, RANKS)
  # 1. the moments, to the summation error of N draws
  for k in ("center", "spread"):
    np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(own[k]), err_msg=k)
  with np.errstate(all="ignore"), warnings.catch_warnings():
    warnings.simplefilter("ignore", RuntimeWarning)                     # (steps outside a window: all NaN)
    big = np.nanmax(np.abs(own["x"]), axis=3)                           # [B, W, 2, T]
  there = ~np.isnan(own["center"])
  err = np.abs(got["center"] - own["center"])[there]
  print(f"  center: max error {err.max():.3e} of the bound {(1e-10 * big[there]).min():.3e} .. ")
  assert (err <= 1e-10 * big[there]).all()
  rel = (np.abs(got["spread"] - own["spread"]) / own["spread"])[there]
  print(f"  spread: max relative error {rel.max():.3e}")
  assert (rel <= 1e-10).all()
  # 2. everything else from the device's own moments, bit for bit
  want = _native.path_excursions_host(traj, scale[:B], shift[:B], obs, first, count, RANKS,
                                      center=got["center"], spread=got["spread"])
  for k in BITWISE:
    np.testing.assert_array_equal(got[k], want[k], err_msg=k)
  # 3. the conventions
  empty = count == 0
  assert (got["excursion"][empty] == 0.0).all() and (got["excursion_order"][empty] == 0.0).all()
  assert np.isnan(got["observed_excursion"][empty]).all()
  assert (got["at"][empty] == -1).all() and (got["exceed"][empty] == 0).all()
  assert np.isnan(got["center"][empty]).all() and np.isnan(got["spread"][empty]).all()
  assert not np.isnan(got["excursion"]).any()
  for b in range(B):
    for w in range(W):
      f, c = first[b, w], count[b, w]
      has = ~np.isnan(obs[b, f:f + c])
      outside = np.ones(T, bool)
      outside[f:f + c] = False
      assert np.isnan(got["center"][b, w][:, outside]).all()
      assert not np.isnan(got["center"][b, w, 0, f:f + c]).any()
      np.testing.assert_array_equal(np.isnan(got["center"][b, w, 1, f:f + c]), ~has)
      if has.any():
        assert (got["at"][b, w] >= f).all() and (got["at"][b, w] < f + c).all()
        assert (got["excursion"][b, w] > 0.0).all()
      else:
        assert (got["at"][b, w] == -1).all() and (got["excursion"][b, w] == 0.0).all()
  return got, own


HOLES = ((52, 62),) * 3


def test_single_fit_with_unaligned_rows():
  run = _run((67,), (WINDOWS,), HOLES[:1])
  got, own = _check(run, "T = 67")
  # the cumulative path at the window's last step is the window's point_sum, bit for bit
  totals = _native.window_totals_host(run[0], SCALE[:1], SHIFT[:1], run[2], run[3], run[4])
  for w, (f, c) in enumerate(WINDOWS):
    if c:
      np.testing.assert_array_equal(own["x"][0, w, 1, :, f + c - 1], totals[0, w, 1])


def test_single_fit_with_aligned_rows():
  _check(_run((72,), (((40, 32),) + WINDOWS[1:],), HOLES[:1]), "T = 72")


def test_batch_with_windows_per_series_and_one_without_any_observation():
  windows = (WINDOWS, ((45, 20), (64, 3), (0, 67), (50, 0), (60, 5), (66, 1)),
             ((50, 4), (40, 27), (63, 2), (41, 1), (50, 4), (44, 0)))
  holes = ((52, 62), (45,), (50, 51, 52, 53, 60))            # series 2, windows 0 and 4: no observation
  got, _ = _check(_run((67, 67, 67), windows, holes), "B = 3")
  assert (got["at"][2, 0] == -1).all() and np.isnan(got["observed_excursion"][2, 0]).all()


def test_ragged_trend_panel():
  """Lengths 50, 130 and 300: a ragged session holds series of one steps-per-thread class
  (`batch.steps_class`), so the panel is two launches, as `fit_causalimpact_panel` cuts it."""
  lengths = (50, 130, 300)
  windows = (((35, 15), (40, 3)), ((90, 40), (60, 70)), ((200, 100), (120, 180)))
  holes = ((37,), (95, 128), (250, 255))
  classes = {}
  for b, T in enumerate(lengths):
    classes.setdefault(batch.steps_class(T), []).append(b)
  assert sorted(classes.values()) == [[0, 1], [2]]
  for ids in classes.values():
    run = _run(tuple(lengths[b] for b in ids), tuple(windows[b] for b in ids), tuple(holes[b] for b in ids),
               ragged=True)
    assert "ragged" in run[-1] and run[0].shape[2] == max(lengths[b] for b in ids)
    _check(run, f"ragged trend {[lengths[b] for b in ids]}")


def test_ragged_seasonal_panel():
  windows = (((42, 18), (59, 1)), ((98, 42), (60, 70)))
  run = _run((60, 140), windows, ((45,), (100, 139)), seasons=((7, 1),), ragged=True)
  assert "ragged" in run[-1] and run[0].shape[2] == 140
  _check(run, "ragged seasonal")


def test_one_launch_hmc_batch():
  B, T, C_, S = 2, 67, 2, 35
  series = [_series(T, 2, 40 + 7 * b, ()) for b in range(B)]
  pb = _native.make_problem(T=T, P=2, has_slope=False, num_warmup=0, num_results=1, num_series=B, seed=(3, 4))
  sess = _native.BatchLogLikSession(pb, _native.make_params([s[3] for s in series]),
                                    np.stack([s[0] for s in series]), np.stack([s[1] for s in series]),
                                    np.stack([s[2] for s in series]))
  obs = _observed(B, T, HOLES[:B])
  first, count = _tables((WINDOWS,) * B)
  try:
    with pytest.raises(_native.NativeError, match="needs a finished ci_ll_session_hmc_run"):
      sess.summarize_paths(SCALE[:B], SHIFT[:B], obs, first, count, RANKS)
    sess.hmc_run(num_chains=C_, num_warmup=10, num_results=S, num_leapfrog=4, seed=(3, 4))
    traj = sess.hmc_fetch()[3]["posterior_trajectories"].reshape(B, C_ * S, T)
    got = sess.summarize_paths(SCALE[:B], SHIFT[:B], obs, first, count, RANKS)
    name = sess.kernel_name()
  finally:
    sess.close()
  _check((traj, got, obs, first, count, name), "HMC batch")


def test_three_chunks_equal_one():
  """The limit of the call's device memory made so small that every series is a chunk of its own."""
  lengths, windows = (67, 67, 67), (WINDOWS,) * 3
  one = _run(lengths, windows, HOLES)[1]
  sess, T = _open(lengths)
  N, (first, count) = 70, _tables(windows)
  obs = _observed(3, T, HOLES)
  # the doubles of a series' windows (include/causalimpact_amd.h) and the tables of the call
  per_series = sum(c * (2 * N + 4) + 2 * N + 20 for _, c in WINDOWS) * 8
  tables = (3 * T + 6) * 8 + 2 * first.size * 4 + (first.size + 1) * 8 + 8 * 4
  try:
    sess.run()
    whole = sess.summarize_paths(SCALE, SHIFT, obs, first, count, RANKS, max_bytes=1 << 30)
    cut = sess.summarize_paths(SCALE, SHIFT, obs, first, count, RANKS, max_bytes=tables + per_series + 64)
    with pytest.raises(_native.NativeError, match=r"window 0 of series 0: .* the limit is"):
      sess.summarize_paths(SCALE, SHIFT, obs, first, count, RANKS, max_bytes=tables + 1000)
  finally:
    sess.close()
  assert whole.pop("num_chunks") == 1 and cut.pop("num_chunks") == 3
  for k in _native.PATH_OUTPUTS:
    np.testing.assert_array_equal(cut[k], whole[k], err_msg=k)
    np.testing.assert_array_equal(one[k], whole[k], err_msg=k)


def test_every_refusal_is_an_error_before_any_device_work():
  fn = _native.load().ci_session_summarize_paths
  sess, T = _open((67,))
  one, obs = np.ones(1), np.zeros((1, T))
  ranks = np.asarray([0, 69], np.int32)
  out = np.zeros((1, 65, 2, 2))

  def raw(first, count, num_windows=None, num_ranks=2, scale=one):
    first, count = np.asarray(first, np.int32), np.asarray(count, np.int32)
    rc = fn(sess._h, None if scale is None else scale.ctypes.data, one.ctypes.data, obs.ctypes.data,   # pylint: disable=protected-access
            first.size if num_windows is None else num_windows, first.ctypes.data, count.ctypes.data,
            num_ranks, ranks.ctypes.data, None, None, None, out.ctypes.data, None, None, None)
    return rc, _native.load().ci_last_error().decode()

  try:
    with pytest.raises(_native.NativeError, match="needs a finished ci_session_run"):
      sess.summarize_paths(1.0, 0.0, obs, [40], [27], [0, 69])
    sess.run()
    rc, msg = raw([40], [27], scale=None)
    assert rc != 0 and "NULL argument" in msg
    for num_windows in (0, 65):
      rc, msg = raw(np.zeros(65), np.zeros(65), num_windows=num_windows)
      assert rc != 0 and f"num_windows must be in [1, 64], got {num_windows}" in msg
    rc, msg = raw([40, -1], [27, 3])
    assert rc != 0 and "window 1 of series 0" in msg and "negative" in msg
    rc, msg = raw([40, 50], [27, 18])
    assert rc != 0 and "window 1 of series 0" in msg and "beyond the session's 67 steps" in msg
    for num_ranks in (0, 9):
      rc, msg = raw([40], [27], num_ranks=num_ranks)
      assert rc != 0 and f"num_ranks must be in [1, 8], got {num_ranks}" in msg
    with pytest.raises(_native.NativeError, match=r"rank 70 out of range \[0, 70\)"):
      sess.summarize_paths(1.0, 0.0, obs, [40], [27], [0, 70])
    # ... and the session is as usable as before: some of the outputs alone
    got = sess.summarize_paths(1.0, 0.0, obs, [0], [67], [0, 69], want=("excursion_order", "exceed"))
    assert list(got) == ["excursion_order", "exceed"] and got["excursion_order"].shape == (1, 1, 2, 2)
  finally:
    sess.close()
