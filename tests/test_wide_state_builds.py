"""Every build of the multi-wavefront seasonal kernel (csrc/ci_seasonal_mw.h,
gibbs_seasonal_kernel<GWS, BIGP, 4>) per draw against the widened float64 oracle
(tests/wide_oracle.py): the four builds, the LDS bound of the 17-52-column regression block, the
per-step branches of the filter at the edges of the series and the mask, many iterations with
flipping inclusions, and the bits that must not depend on the launch.  Every GPU case checks the
kernel it runs on (Session.kernel_name()), so that a change of routing cannot move it quietly."""
import numpy as np
import pytest

from causalimpact import _model
from causalimpact import _native

import wide_oracle
from test_wide_state import _dfull, _gpu_vs_oracle, _inputs, _mw_name, _assert_draws_match, _KEYS

WS = _native.FLAG_SEASONAL_WORKSPACE
LDS_MAX = 160 * 1024            # the session's LDS limit per chain
LDS_ARRAYS_MAX = 150 * 1024     # ... below which the arrays over time stay in LDS
MAXP = 52                       # ci_kernels.h: wider designs take the BIGP build


def _mw_lds_bytes(T, P, seasons, has_slope, gws):
  """ci::make_slayout(..., nwv = 4).total (csrc/ci_seasonal.h), restated: the LDS a chain of the
  multi-wavefront kernel takes, with the arrays over time in LDS (gws = 0) or in the workspace.
  Pinned by test_lds_refusals_name_the_restated_layout and by the kernel names at the T edge."""
  K = len(seasons)
  D = _dfull(has_slope, seasons)
  dred = D - K
  o = 0

  def take(nbytes):
    nonlocal o
    o += (nbytes + 15) & ~15

  def padded(e):            # sweep_padded
    return (e + 1023) & ~1023

  TS = (T + 3) & ~3
  Tf = 4 * TS
  Pp, Kp = max(P, 1), max(K, 1)
  bigp = P > MAXP
  big = P > 16 and not bigp
  take(16 if bigp else 8 * Pp * Pp)                          # xtx
  take(16 if bigp else 8 * Pp * Pp)                          # omega
  take(8 * (Pp + 4))                                         # bvec
  take(8 * padded((Pp + 1) ** 2) if big else 16)             # aug0
  take(8 * padded(Pp * Pp) if big else 16)                   # pri0
  take(8 * Pp * Pp if big else 16)                           # chol
  for nb in (8, 8, 4, 4, 4):                                 # zv, uperm, nz, perm, idx
    take(nb * Pp if big else 16)
  take(4 * (D * (D + 1) // 2))                               # the packed triangle
  take(4 * (256 + 96))                                       # the step area (MW_LDS_FLOATS)
  take(4 * (dred + 1))
  take(4 * (dred + 1))
  take(4 * 8)
  take(4 * max(Pp, 16))
  if gws:
    return o
  for nb in (Tf, Tf, Tf if has_slope else 16, Tf, Tf, Tf, Tf, Tf if has_slope else 16, Tf,
             Tf * Kp, Tf * Kp, Tf * Kp, 4 * T * D, 4 * T * D, TS, TS, TS * Kp):
    take(nb)
  return o


def _longest_in_lds(p, has_slope, seasons):
  """The longest series whose arrays over time the session keeps in LDS."""
  P = p + 1 if p else 0
  T = 3
  while _mw_lds_bytes(T + 1, P, seasons, has_slope, 0) <= LDS_ARRAYS_MAX:
    T += 1
  return T


def _largest_p_in_lds(has_slope, seasons):
  """The most design columns (17-52) whose regression block fits LDS next to the triangle."""
  return max(P for P in range(17, MAXP + 1) if _mw_lds_bytes(300, P, seasons, has_slope, 1) <= LDS_MAX)


def _session(T, p, has_slope, seasons, flags=0, edit=None, **kw):
  y, mask, X, spec = _inputs(T, p, has_slope, seasons, edit=edit)
  counts, flg = _model.expand_seasons(seasons, T)
  kw = dict(dict(num_warmup=0, num_results=4, seed=(2, 6)), **kw)
  pb = _native.make_problem(T=T, P=spec["P"], has_slope=has_slope, num_seasons=counts, flags=flags, **kw)
  return _native.Session(pb, y[None], mask[None], None if X is None else X[None], flg,
                         _native.make_params([spec]))


def _kernel_of(T, p, has_slope, seasons, flags=0):
  s = _session(T, p, has_slope, seasons, flags)
  try:
    return s.kernel_name()
  finally:
    s.close()


def _fit(T, p, has_slope, seasons, flags=0, kernel=None, **kw):
  s = _session(T, p, has_slope, seasons, flags, **kw)
  try:
    if kernel is not None:
      assert s.kernel_name() == kernel
    s.run()
    return s.fetch()
  finally:
    s.close()


# ---------------------------------------------------------------------------------------------
# CPU: the restated layout at the documented edges
# ---------------------------------------------------------------------------------------------

def test_restated_layout_gives_the_documented_lds_edges():
  assert _largest_p_in_lds(1, ((254, 1),)) == 21            # D = 256
  assert _largest_p_in_lds(0, ((7, 1), (192, 1))) == 43     # D = 200
  assert _largest_p_in_lds(1, ((168, 1),)) == 46            # D = 170
  assert _largest_p_in_lds(0, ((24, 1), (124, 1))) == 52    # D = 149: every P
  assert _largest_p_in_lds(0, ((24, 1), (125, 1))) == 51    # D = 150
  # P <= 16 and P >= 53 keep no O(P^2) array in LDS: every D <= 256 fits
  for P in (0, 16, 53, 512):
    assert _mw_lds_bytes(300, P, ((254, 1),), 1, 1) <= LDS_MAX


# ---------------------------------------------------------------------------------------------
# GPU: the four builds, per draw
# ---------------------------------------------------------------------------------------------

_LL_CASES = [                                     # (p, has_slope, seasons): arrays in LDS
    (2, 0, ((7, 1), (60, 2))),                     # D = 68
    (4, 1, ((7, 1), (52, 7), (12, 28))),           # D = 73, three blocks
]


@pytest.mark.gpu
@pytest.mark.parametrize("p,has_slope,seasons", _LL_CASES)
def test_arrays_in_lds_build_matches_the_oracle_at_its_longest_series(p, has_slope, seasons):
  """<false,false,4>: the longest series that keeps its arrays in LDS, and one step more moves
  them to the workspace."""
  assert 64 < _dfull(has_slope, seasons) <= 80
  T = _longest_in_lds(p, has_slope, seasons)
  assert 100 <= T <= 300, T
  assert _kernel_of(T + 1, p, has_slope, seasons) == _mw_name(True, False)
  _gpu_vs_oracle(T, p, has_slope, seasons, kernel=_mw_name(False, False))


@pytest.mark.gpu
@pytest.mark.parametrize("T,p,has_slope,seasons,gws", [
    (120, 52, 1, ((7, 1), (60, 1)), False),         # D = 69, P = 53: the first BIGP width
    (140, 119, 0, ((66, 1),), False),               # D = 67, P = 120
    (300, 52, 0, ((24, 1), (52, 3)), True),         # D = 77, P = 53
    (302, 120, 1, ((168, 1),), True),               # D = 170, P = 121
    (203, 511, 1, ((254, 1),), True),               # D = 256, P = 512: the C-ABI maximum
])
def test_bigp_builds_match_the_oracle_per_draw(T, p, has_slope, seasons, gws):
  """<false,true,4> and <true,true,4>: the regression block in the workspace, behind the arrays
  over time (GWS) or at the start of the chain's slice."""
  assert p + 1 > MAXP and 64 < _dfull(has_slope, seasons) <= 256
  _gpu_vs_oracle(T, p, has_slope, seasons, kernel=_mw_name(gws, True))


# ---------------------------------------------------------------------------------------------
# GPU: the LDS bound of the 17-52-column regression block
# ---------------------------------------------------------------------------------------------

_EDGE_CASES = [                                   # (has_slope, seasons) at D = 256, 200, 170, 130
    (1, ((254, 1),)),
    (0, ((7, 1), (192, 1))),
    (1, ((168, 1),)),
    (0, ((24, 1), (105, 1))),
]


@pytest.mark.gpu
@pytest.mark.parametrize("has_slope,seasons", _EDGE_CASES)
def test_largest_lds_regression_block_next_to_the_triangle_matches_the_oracle(has_slope, seasons):
  P = _largest_p_in_lds(has_slope, seasons)
  _gpu_vs_oracle(300, P - 1, has_slope, seasons, kernel=_mw_name(True, False))


@pytest.mark.gpu
@pytest.mark.parametrize("has_slope,seasons,P", [
    (1, ((254, 1),), 22),
    (0, ((7, 1), (192, 1)), 44),
    (1, ((168, 1),), 47),
    (0, ((24, 1), (125, 1)), 52),                  # D = 150: the first state that not every P fits
])
def test_lds_refusals_name_the_restated_layout(has_slope, seasons, P):
  """One column more than fits is refused when the session is created -- nothing is launched --
  with the existing error, and the bytes it names are the restated layout's."""
  need = _mw_lds_bytes(300, P, seasons, has_slope, 1)
  assert need > LDS_MAX
  with pytest.raises(_native.NativeError, match=f"needs {need} bytes of LDS per chain"):
    _session(300, P - 1, has_slope, seasons)
  # one column fewer is accepted
  assert _kernel_of(300, P - 2, has_slope, seasons) == _mw_name(True, False)


@pytest.mark.gpu
def test_a_149_component_state_takes_every_lds_regression_block():
  assert _dfull(0, ((24, 1), (124, 1))) == 149
  assert _kernel_of(300, MAXP - 1, 0, ((24, 1), (124, 1))) == _mw_name(True, False)


# ---------------------------------------------------------------------------------------------
# GPU: the filter's per-step branches at the edges of the series and of the mask
# ---------------------------------------------------------------------------------------------

def _gap(a, b):
  def edit(m):
    m[a:b] = True
    return m
  return edit


def _first_missing(m):
  m[0] = True
  return m


def _all_observed_after(m):
  """The post-period observed (the last step observed; no forecast tail), a few steps masked."""
  m[:] = False
  m[[5, 6, 77]] = True
  return m


_EIGHT = ((7, 1), (12, 2), (5, 3), (9, 1), (11, 4), (6, 1), (8, 2), (10, 5))   # 68 components


@pytest.mark.gpu
@pytest.mark.parametrize("T,p,has_slope,seasons,flags,edit", [
    (301, 2, 0, ((64, 1),), 0, None),                     # D = 65, T % 4 = 1
    (302, 0, 1, ((63, 1),), 0, None),                     # D = 65, T % 4 = 2
    (303, 3, 1, ((7, 1), (82, 1)), 0, None),              # D = 91, T % 4 = 3
    (3, 0, 0, ((70, 1),), WS, None),                      # the shortest series
    (6, 1, 1, ((7, 1), (60, 1)), WS, None),
    (9, 0, 0, ((7, 2), (120, 1)), WS, None),
    (300, 2, 1, ((80, 1),), 0, _first_missing),
    (300, 2, 0, ((7, 3), (60, 2)), 0, _gap(30, 75)),      # masked steps with no change: no barrier
    (300, 2, 1, ((66, 4),), 0, _gap(41, 90)),             # the same gap with a slope
    (301, 2, 0, ((7, 3), (60, 2)), 0, _all_observed_after),
    (301, 2, 1, ((66, 4),), 0, None),                     # ... next to the forecast tail
    (300, 2, 1, _EIGHT, 0, None),                         # 8 blocks, D = 70
    (301, 2, 0, ((255, 1),), 0, None),                    # D = 256 without a slope
    (301, 0, 1, ((254, 1),), 0, _gap(50, 90)),            # ... and with one
])
def test_series_and_mask_edges_on_the_workspace_build_match_the_oracle(T, p, has_slope, seasons,
                                                                       flags, edit):
  assert 64 < _dfull(has_slope, seasons) <= 256
  _gpu_vs_oracle(T, p, has_slope, seasons, flags=flags, edit=edit, kernel=_mw_name(True, False))


# ---------------------------------------------------------------------------------------------
# GPU: many iterations with flipping inclusions
# ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("T,p,has_slope,seasons,bigp", [
    (300, 19, 0, ((24, 1), (52, 3)), False),        # D = 77, P = 20 (17-52: the LDS block)
    (260, 59, 1, ((7, 1), (61, 2)), True),          # D = 70, P = 60
])
def test_wide_state_follows_the_oracle_over_many_iterations(T, p, has_slope, seasons, bigp):
  """40 iterations after a warm-up: the previous sigma^2 in the weight adjustment, the drift scales
  wave 0 publishes, both routes of the regression draw (accepted flips and none) -- every draw
  the oracle's, with the tolerances of test_gpu_gibbs.py's
  test_workgroup_wide_regression_block_follows_the_oracle_over_many_iterations."""
  W, S = 4, 36
  y, mask, X, spec = _inputs(T, p, has_slope, seasons)
  got = _fit(T, p, has_slope, seasons, kernel=_mw_name(True, bigp), num_warmup=W, num_results=S)
  w = wide_oracle.fit_gibbs(y, mask, X, spec, num_results=S, num_warmup=W, seed=(2, 6))
  incl_dev, incl_orc = got["weights"][0, 0] != 0, w["weights"] != 0
  np.testing.assert_array_equal(incl_dev, incl_orc)
  changes = int((incl_orc[1:] != incl_orc[:-1]).any(axis=1).sum())
  assert 0 < changes < S - 1, changes            # both routes of the weights draw were taken
  np.testing.assert_allclose(got["weights"][0, 0], w["weights"], atol=2e-2)
  np.testing.assert_allclose(got["observation_noise_scale"][0, 0], w["obs_scale"], rtol=2e-2)
  np.testing.assert_allclose(got["posterior_means"][0, 0], w["pred_mean"], atol=2e-2)
  np.testing.assert_allclose(got["seasonal_drift_scales"][0, 0], w["drift_scales"], rtol=2e-2)
  np.testing.assert_allclose(got["level"][0, 0], w["level"], atol=2e-2)
  np.testing.assert_allclose(got["seasonal_levels"][0, 0], w["seasonal"], atol=2e-2)


# ---------------------------------------------------------------------------------------------
# GPU: what must not change the bits
# ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("p,has_slope,seasons", [
    (2, 0, ((7, 1), (60, 2))),
    (52, 1, ((7, 1), (60, 1))),                      # P = 53
])
def test_workspace_flag_on_a_wide_state_that_fits_lds_gives_the_same_bits(p, has_slope, seasons):
  """Mirrors test_gpu_gibbs.py::test_seasonal_kernel_with_arrays_in_hbm_equals_the_lds_variant."""
  T = min(150, _longest_in_lds(p, has_slope, seasons))
  bigp = p + 1 > MAXP
  kw = dict(num_warmup=3, num_results=5, num_chains=2, seed=(3, 3))
  lds = _fit(T, p, has_slope, seasons, kernel=_mw_name(False, bigp), **kw)
  ws = _fit(T, p, has_slope, seasons, flags=WS, kernel=_mw_name(True, bigp), **kw)
  for k, v in lds.items():
    np.testing.assert_array_equal(ws[k], v, err_msg=k)


@pytest.mark.gpu
def test_bigp_batch_equals_single_series_fits_and_each_series_its_oracle():
  T, p, has_slope, seasons = 260, 59, 1, ((7, 1), (62, 1))      # D = 71, P = 60
  B, C, S = 3, 2, 4
  ins = [_inputs(T, p, has_slope, seasons, seed=7 + b) for b in range(B)]
  counts, flg = _model.expand_seasons(seasons, T)
  kw = dict(T=T, P=p + 1, has_slope=has_slope, num_seasons=counts, num_warmup=0, num_results=S,
            num_chains=C, seed=(2, 6))
  pb = _native.make_problem(num_series=B, **kw)
  s = _native.Session(pb, np.stack([i[0] for i in ins]), np.stack([i[1] for i in ins]),
                      np.stack([i[2] for i in ins]), flg, _native.make_params([i[3] for i in ins]))
  try:
    assert s.kernel_name() == _mw_name(True, True)
    s.run()
    batch = s.fetch()
  finally:
    s.close()
  for b, (y, mask, X, spec) in enumerate(ins):
    one = _native.fit_gibbs(_native.make_problem(series_offset=b, **kw), y[None], mask[None], X[None],
                            flg, _native.make_params([spec]))
    for k in _KEYS:
      np.testing.assert_array_equal(batch[k][b], one[k][0], err_msg=f"{k} series {b}")
    for c in range(C):
      w = wide_oracle.fit_gibbs(y, mask, X, spec, num_results=S, num_warmup=0,
                                seed=_native.series_stream_key((2, 6), b), chain=c)
      _assert_draws_match(batch, b, c, w, has_slope, spec["P"])
  assert not np.array_equal(batch["weights"][0, 0], batch["weights"][1, 0])


@pytest.mark.gpu
def test_more_chains_than_compute_units_give_the_bits_of_one_chain_runs():
  """300 workgroups of 256 threads on 256 CUs: the launch runs in several rounds."""
  T, p, has_slope, seasons = 200, 2, 1, ((168, 1),)               # D = 170
  kw = dict(num_warmup=1, num_results=2, seed=(4, 9))
  many = _fit(T, p, has_slope, seasons, kernel=_mw_name(True, False), num_chains=300, **kw)
  for c in (0, 1, 255, 256, 299):
    one = _fit(T, p, has_slope, seasons, kernel=_mw_name(True, False), num_chains=1, chain_offset=c, **kw)
    for k in _KEYS:
      np.testing.assert_array_equal(many[k][0, c], one[k][0, 0], err_msg=f"{k} chain {c}")
  assert not np.array_equal(many["level"][0, 0], many["level"][0, 299])
