"""Batched HMC fits (ci_ll_session_create_batch, ci_ll_session_hmc_summarize): the entry points are
declared, bound and exported, the batch session refuses bad input before any device call, and
`fit_causalimpact_batch(sampler="hmc")` picks its route as documented.  (No compute: no GPU.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from causalimpact import _hmc
from causalimpact import _native
from causalimpact import batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ci_ll_session_create_batch", "ci_ll_session_hmc_summarize")


def test_new_symbols_are_declared_bound_and_exported():
  hdr = open(os.path.join(ROOT, "include", "causalimpact_amd.h")).read()
  hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
  lib = C.CDLL(_native.LIB_PATH)
  for name in NEW:
    assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert name in _native.exported_symbols(), name
    assert hasattr(lib, name), name
    assert getattr(_native.load(), name).argtypes, name


def _spec(**kw):
  sp = dict.fromkeys(_native._PARAM_FIELDS, 1.0)   # pylint: disable=protected-access
  sp.update(kw)
  return sp


def _create(pb, params, y, mask, X, max_evals=1, out=True):
  h = C.c_void_p()
  rc = _native.load().ci_ll_session_create_batch(
      C.byref(pb) if pb is not None else None, params,
      None if y is None else y.ctypes.data, None if mask is None else mask.ctypes.data,
      None if X is None else X.ctypes.data, max_evals, C.byref(h) if out else None)
  assert not h, "a session was created"
  return rc, _native.load().ci_last_error().decode()


def _inputs(B, T, P):
  y = np.zeros((B, T), np.float32)
  m = np.zeros((B, T), np.uint8)
  X = np.zeros((B, T, P), np.float32) if P else None
  return y, m, X


def test_create_batch_refuses_invalid_input_before_any_device_call():
  B, T = 3, 40
  prm = _native.make_params([_spec()] * B)
  y, m, X = _inputs(B, T, 2)

  def pb(**kw):
    a = dict(T=T, P=2, has_slope=0, num_warmup=0, num_results=1, num_series=B)
    a.update(kw)
    return _native.make_problem(**a)

  rc, msg = _create(pb(num_seasons=(7,)), prm, y, m, X)
  assert rc != 0 and "seasonal blocks are not supported" in msg
  yl, ml, Xl = _inputs(B, 4097, 2)
  rc, msg = _create(pb(T=4097), prm, yl, ml, Xl)
  assert rc != 0 and "T must be <= 4096, got 4097" in msg
  y1, m1, X1 = _inputs(B, T, 129)
  rc, msg = _create(pb(P=129), prm, y1, m1, X1)
  assert rc != 0 and "P must be <= 128, got 129" in msg
  rc, msg = _create(pb(num_series=0), prm, y, m, X)
  assert rc != 0 and "num_series must be >= 1, got 0" in msg
  for args in ((None, prm, y, m, X), (pb(), None, y, m, X), (pb(), prm, None, m, X),
               (pb(), prm, y, None, X)):
    rc, msg = _create(*args)
    assert rc != 0 and "must not be NULL" in msg
  rc, msg = _create(pb(), prm, y, m, X, out=False)
  assert rc != 0 and "must not be NULL" in msg
  rc, msg = _create(pb(), prm, y, m, None)
  assert rc != 0 and "X is NULL but P=2" in msg
  for bad in (0.0, -1.0, float("inf"), float("nan")):
    prm_bad = _native.make_params([_spec(), _spec(weights_prior_scale=bad), _spec()])
    rc, msg = _create(pb(), prm_bad, y, m, X)
    assert rc != 0 and "params[1].weights_prior_scale must be positive and finite" in msg
  yn = y.copy()
  yn[2, 5] = np.nan
  rc, msg = _create(pb(), prm, yn, m, X)
  assert rc != 0 and "y[2, 5] is not finite but unmasked" in msg
  rc, msg = _create(pb(), prm, y, m, X, max_evals=0)
  assert rc != 0 and "max_evals must be >= 1" in msg


def test_batch_session_wrapper_checks_the_init_shape_before_running():
  # the shape check of init_theta is host-side: [B, C, dim] for a batched session
  sess = _native.BatchLogLikSession.__new__(_native.BatchLogLikSession)
  sess.B, sess.P, sess.D, sess.K, sess._h = 4, 2, 1, 0, C.c_void_p()   # pylint: disable=protected-access
  with pytest.raises(ValueError, match=r"init_theta must be \[4, 3, 4\]"):
    sess.hmc_run(num_chains=3, num_warmup=1, num_results=1, init_theta=np.zeros((3, 4)))


ONE, PER = "one_launch", "per_series"


@pytest.mark.parametrize("kw,want", [
    (dict(), ONE),
    (dict(P=0), ONE),
    (dict(P=128), ONE),
    (dict(T=4096), ONE),
    (dict(T=3), ONE),
    (dict(num_seasonal_blocks=1), PER),
    (dict(num_seasonal_blocks=2, P=0), PER),
    (dict(T=4097), PER),
    (dict(P=129), PER),
    (dict(hmc_init="vi"), PER),
    (dict(float64=True), PER),
    (dict(standardize_data=False), PER),
    (dict(float64=True, standardize_data=False, T=5000), PER),
])
def test_hmc_batch_route(kw, want):
  a = dict(float64=False, standardize_data=True, num_seasonal_blocks=0, T=500, P=6, hmc_init="gibbs")
  a.update(kw)
  assert batch.hmc_batch_route(**a) == want


def test_hmc_batch_launches_split_under_the_hbm_budget():
  per = _hmc.hmc_batch_bytes_per_series(500, 6, 1, 1000)
  assert per >= 1000 * 500 * (3 * 4 + 2 * 8)              # level, slope, trajectory, summary scratch
  assert _hmc.series_per_launch(500, 6, 1, 1000, budget=10 * per) == 10
  assert _hmc.series_per_launch(500, 6, 1, 1000, budget=10 * per - 1) == 9
  assert _hmc.series_per_launch(500, 6, 1, 1000, budget=1) == 1
  assert _hmc.series_per_launch(3, 0, 1, 1, budget=1 << 40) == 65535
  # the cfg5 shape is one launch under the default budget
  assert _hmc.series_per_launch(500, 6, 1, 1000) >= 512


def test_batch_refuses_an_unknown_sampler():
  import causalimpact as ci   # pylint: disable=import-outside-toplevel
  v = np.random.default_rng(0).normal(size=(2, 30, 2))
  with pytest.raises(ValueError, match="sampler must be"):
    ci.fit_causalimpact_batch(v, (0, 19), (20, 29),
                              inference_options=ci.InferenceOptions(sampler="nuts"))
