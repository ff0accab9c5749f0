"""ctypes binding of the C-ABI in include/causalimpact_amd.h.

This is the only place the host package touches native code.  There is no CPU
fallback: if lib/libcausalimpact_amd.so is missing or no MI355X is visible the
calls raise (the reference's hot path, causalimpact_lib.py:345-395, is replaced
by these entry points and by nothing else).
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, Optional, Sequence

import numpy as np

ABI_VERSION = 5
MAX_BLOCKS = 8
MAX_SUMMARY_RANKS = 8   # == ci::SUMM_MAX_RANKS (csrc/ci_summary.h)
# the output arrays of ci_session_summarize_components, in argument order
COMPONENT_OUTPUTS = ("trend_mean", "trend_order", "seasonal_mean", "seasonal_order",
                     "regression_mean", "regression_order", "inclusion_prob", "weight_mean",
                     "weight_order")
# the output arrays of ci_session_summarize_predictions, in argument order
PREDICTION_OUTPUTS = ("forecast_mean", "forecast_order", "variance_mean", "pit_mean", "loglik")
# the output arrays of ci_session_summarize_placebo, in argument order
PLACEBO_OUTPUTS = ("predicted_mean", "spread_mean", "pit_mean")
# the output arrays of ci_session_simulate_placebo, in argument order
PLACEBO_SIM_OUTPUTS = ("predicted_mean", "spread_mean", "below", "total_order", "totals")
SITE_PLACEBO_SIM = 18   # == ci::SITE_PLACEBO_SIM (csrc/ci_rng.h)
# the outcome link of a session's summaries (== CI_LINK_*): value = z, exp(z), expm1(z)
LINK_IDENTITY, LINK_LOG, LINK_LOG1P = 0, 1, 2
_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG_ROOT, "lib", "libcausalimpact_amd.so")

_PARAM_FIELDS = (
    "level_conc", "level_scale", "level_ub", "slope_conc", "slope_scale", "slope_ub",
    "obs_conc", "obs_scale", "obs_ub", "drift_conc", "drift_scale", "drift_ub",
    "nonzero_prob", "init_level_loc", "init_level_scale", "init_slope_scale",
    "init_seasonal_scale", "obs_scale0", "level_scale0", "slope_scale0")


class SeriesParams(C.Structure):
  _fields_ = ([(f, C.c_double) for f in _PARAM_FIELDS] + [("drift_scale0", C.c_double * MAX_BLOCKS)]
              + [("weights_prior_scale", C.c_double)])


class Problem(C.Structure):
  _fields_ = [
      ("abi_version", C.c_int32), ("T", C.c_int32), ("P", C.c_int32), ("has_slope", C.c_int32),
      ("num_blocks", C.c_int32), ("num_seasons", C.c_int32 * MAX_BLOCKS),
      ("num_warmup", C.c_int32), ("num_results", C.c_int32), ("num_chains", C.c_int32),
      ("chain_offset", C.c_int32), ("num_series", C.c_int32), ("seed", C.c_uint32 * 2),
      ("device", C.c_int32), ("flags", C.c_int32), ("series_offset", C.c_int32),
      ("reserved", C.c_int32)]


_OUT_FIELDS = ("observation_noise_scale", "level_scale", "slope_scale", "seasonal_drift_scales",
               "weights", "level", "slope", "seasonal_levels", "posterior_means",
               "posterior_trajectories")


class Outputs(C.Structure):
  _fields_ = [(f, C.c_void_p) for f in _OUT_FIELDS]


class HmcOptions(C.Structure):
  _fields_ = [
      ("num_chains", C.c_int32), ("chain_offset", C.c_int32), ("num_warmup", C.c_int32),
      ("num_results", C.c_int32), ("num_leapfrog", C.c_int32), ("prior", C.c_int32),
      ("target_accept", C.c_double), ("initial_step_size", C.c_double),
      ("horseshoe_scale", C.c_double), ("seed", C.c_uint32 * 2)]


HMC_PRIORS = {"slab": 0, "horseshoe": 1}   # == CI_HMC_PRIOR_*


class NativeError(RuntimeError):
  pass


_lib = None


def load():
  """Loads the HIP library; raises NativeError when it has not been built."""
  global _lib
  if _lib is not None:
    return _lib
  if not os.path.exists(LIB_PATH):
    raise NativeError(
        f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(there is no CPU fallback for the Gibbs hot path)")
  L = C.CDLL(LIB_PATH)
  L.ci_last_error.restype = C.c_char_p
  L.ci_abi_version.restype = C.c_int
  L.ci_device_count.argtypes = [C.POINTER(C.c_int)]
  L.ci_series_stream_key.argtypes = [C.POINTER(C.c_uint32), C.c_int32, C.POINTER(C.c_uint32)]
  L.ci_series_stream_key.restype = None
  L.ci_device_synchronize.argtypes = [C.c_int]
  L.ci_fit_gibbs.argtypes = [C.POINTER(Problem), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.POINTER(SeriesParams), C.POINTER(Outputs)]
  L.ci_fit_gibbs_f64.argtypes = [C.POINTER(Problem), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.POINTER(SeriesParams), C.POINTER(Outputs)]
  L.ci_fit_gibbs_f64_kernel_ms.argtypes = [C.POINTER(C.c_float)]
  L.ci_fit_gibbs_f64_route.argtypes = [C.POINTER(Problem), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
  L.ci_session_create.argtypes = [C.POINTER(Problem), C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.POINTER(SeriesParams), C.POINTER(C.c_void_p)]
  L.ci_session_create_ragged.argtypes = [C.POINTER(Problem), C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.POINTER(SeriesParams),
                                         C.POINTER(C.c_void_p)]
  L.ci_session_create_ragged_seasonal.argtypes = [C.POINTER(Problem), C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.POINTER(SeriesParams), C.POINTER(C.c_void_p)]
  for name in ("ci_session_create_from_draws", "ci_session_create_from_draws_f64"):
    if hasattr(L, name):                               # (additive: a library built before it lacks it)
      getattr(L, name).argtypes = ([C.POINTER(Problem)] + [C.c_void_p] * 4 + [C.POINTER(SeriesParams)] +
                                   [C.c_void_p] * 5 + [C.POINTER(C.c_void_p)])
  L.ci_session_run.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
  L.ci_session_fetch.argtypes = [C.c_void_p, C.POINTER(Outputs)]
  L.ci_session_algorithmic_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
  L.ci_session_destroy.argtypes = [C.c_void_p]
  L.ci_session_profile.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
  L.ci_session_summarize.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]
  L.ci_session_summarize_components.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                C.c_void_p] + [C.c_void_p] * 9
  if hasattr(L, "ci_session_summarize_predictions"):   # (additive: a library built before it lacks it)
    L.ci_session_summarize_predictions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                   C.c_void_p] + [C.c_void_p] * 5
  if hasattr(L, "ci_session_summarize_placebo"):       # (additive, likewise)
    L.ci_session_summarize_placebo.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                               C.c_void_p, C.c_void_p] + [C.c_void_p] * 3
  if hasattr(L, "ci_session_summarize_predictions_blocks"):   # (additive, likewise)
    L.ci_session_summarize_predictions_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                          C.c_void_p] + [C.c_void_p] * 5
  if hasattr(L, "ci_session_summarize_placebo_blocks"):       # (additive, likewise)
    L.ci_session_summarize_placebo_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                      C.c_void_p, C.c_void_p] + [C.c_void_p] * 3
  for name in ("ci_session_summarize_placebo_horizons", "ci_test_session_summarize_placebo_horizons"):
    if hasattr(L, name):                               # (additive, likewise)
      getattr(L, name).argtypes = ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                    C.c_void_p] + [C.c_void_p] * 3 +
                                   ([C.c_int64, C.c_void_p] if name.startswith("ci_test_") else []))
  for name in ("ci_session_simulate_placebo", "ci_session_simulate_placebo_blocks",
               "ci_test_session_simulate_placebo"):
    if hasattr(L, name):                               # (additive, likewise)
      test = name.startswith("ci_test_")
      getattr(L, name).argtypes = ([C.c_void_p] + ([C.c_int32] if test else []) +
                                   [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                    C.c_void_p, C.c_int32, C.c_void_p] + [C.c_void_p] * 5 +
                                   ([C.c_int64, C.c_void_p] if test else []))
  if hasattr(L, "ci_session_pool_placebo"):            # (additive, likewise)
    L.ci_session_pool_placebo.argtypes = ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 3 +
                                          [C.c_int32] + [C.c_void_p] * 8)
  for name in ("ci_session_pool_placebo_blocks", "ci_test_session_pool_placebo_blocks"):
    if hasattr(L, name):                               # (additive, likewise)
      getattr(L, name).argtypes = ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 3 +
                                   [C.c_int32] + [C.c_void_p] * 8 +
                                   ([C.c_int32] if name.startswith("ci_test_") else []))
  for name in ("ci_session_pool_placebo_horizons", "ci_session_pool_placebo_horizons_blocks",
               "ci_test_session_pool_placebo_horizons"):
    if hasattr(L, name):                               # (additive, likewise)
      test = name.startswith("ci_test_")
      getattr(L, name).argtypes = ([C.c_void_p] + ([C.c_int32] if test else []) +
                                   [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 3 + [C.c_int32, C.c_void_p,
                                    C.c_int32, C.c_void_p] + [C.c_void_p] * 6 +
                                   ([C.c_int32, C.c_void_p] if test else []))
  for name in ("ci_session_pool_simulated_placebo", "ci_session_pool_simulated_placebo_blocks",
               "ci_test_session_pool_simulated_placebo"):
    if hasattr(L, name):                               # (additive, likewise)
      test = name.startswith("ci_test_")
      getattr(L, name).argtypes = ([C.c_void_p] + ([C.c_int32] if test else []) +
                                   [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 3 + [C.c_int32] +
                                   [C.c_void_p] * 2 + [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] +
                                   [C.c_void_p] * 5 + ([C.c_int32] if test else []))
  if hasattr(L, "ci_session_set_link"):                # (additive, likewise)
    L.ci_session_set_link.argtypes = [C.c_void_p, C.c_int32]
    L.ci_session_value_mean.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
  for name in ("ci_session_summarize_windows", "ci_ll_session_summarize_windows"):
    if hasattr(L, name):                               # (additive: a library built before it lacks it)
      getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_void_p]
  for name in ("ci_session_summarize_paths", "ci_ll_session_summarize_paths",
               "ci_test_session_summarize_paths"):
    if hasattr(L, name):                               # (additive, likewise)
      getattr(L, name).argtypes = ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p] + [C.c_void_p] * 7 +
                                   ([C.c_int64, C.c_void_p] if name.startswith("ci_test_") else []))
  for name in ("ci_summarize_draw_paths_f64", "ci_test_summarize_draw_paths_f64"):
    if hasattr(L, name):                               # (additive, likewise)
      getattr(L, name).argtypes = ([C.c_int32] * 4 + [C.c_void_p] * 4 + [C.c_int32, C.c_void_p, C.c_void_p,
                                                                         C.c_int32, C.c_void_p] +
                                   [C.c_void_p] * 7 +
                                   ([C.c_int64, C.c_void_p] if name.startswith("ci_test_") else []))
  for pool_fn in (L.ci_session_pool_trajectories, L.ci_ll_session_pool_trajectories):
    pool_fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                        C.c_void_p, C.c_void_p, C.c_void_p]
  if hasattr(L, "ci_session_pool_event_trajectories"):   # (additive: a library built before it lacks it)
    L.ci_session_pool_event_trajectories.argtypes = [
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
        C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
  L.ci_summarize_draws.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_double,
                                   C.c_double, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
  L.ci_summarize_draws_f64.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_double,
                                   C.c_double, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
  L.ci_kalman_loglik.argtypes = [C.POINTER(Problem), C.POINTER(SeriesParams), C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
  L.ci_ll_session_create.argtypes = [C.POINTER(Problem), C.POINTER(SeriesParams), C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
  L.ci_ll_session_create2.argtypes = [C.POINTER(Problem), C.POINTER(SeriesParams), C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                      C.POINTER(C.c_void_p)]
  L.ci_ll_session_eval.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
  L.ci_ll_session_draw_latents.argtypes = [C.c_void_p, C.c_int32, C.c_void_p,
                                           C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
  L.ci_ll_session_destroy.argtypes = [C.c_void_p]
  L.ci_ll_session_hmc_run.argtypes = [C.c_void_p, C.POINTER(HmcOptions), C.c_void_p,
                                      C.POINTER(C.c_float)]
  L.ci_ll_session_hmc_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(Outputs)]
  L.ci_ll_session_algorithmic_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
  L.ci_ll_session_create_batch.argtypes = [C.POINTER(Problem), C.POINTER(SeriesParams), C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
  L.ci_ll_session_hmc_summarize.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]
  L.ci_pool_trim.argtypes = []
  L.ci_host_alloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
  L.ci_host_free.argtypes = [C.c_void_p]
  L.ci_session_run_streamed.argtypes = [C.c_void_p, C.POINTER(Outputs), C.c_int32,
                                        C.POINTER(C.c_float)]
  L.ci_session_kernel_name.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
  L.ci_ll_session_kernel_name.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
  L.ci_test_rng.argtypes = [C.c_int, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32,
                            C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
  L.ci_test_dk_draw.argtypes = [C.POINTER(Problem), C.POINTER(SeriesParams), C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p,
                                C.c_uint32, C.c_void_p]
  if L.ci_abi_version() != ABI_VERSION:
    raise NativeError(f"ABI mismatch: library {L.ci_abi_version()}, binding {ABI_VERSION}")
  _lib = L
  return L


def exported_symbols() -> Sequence[str]:
  """Every entry point include/causalimpact_amd.h declares."""
  return ("ci_last_error", "ci_abi_version", "ci_device_count", "ci_series_stream_key", "ci_device_synchronize", "ci_pool_trim", "ci_host_alloc",
          "ci_host_free", "ci_fit_gibbs", "ci_fit_gibbs_f64", "ci_fit_gibbs_f64_kernel_ms",
          "ci_fit_gibbs_f64_route",
          "ci_session_create", "ci_session_create_ragged", "ci_session_create_ragged_seasonal",
          "ci_session_create_from_draws", "ci_session_create_from_draws_f64", "ci_session_run", "ci_session_run_streamed", "ci_session_fetch",
          "ci_session_algorithmic_bytes", "ci_session_kernel_name", "ci_session_destroy",
          "ci_session_profile", "ci_ll_session_kernel_name",
          "ci_session_summarize", "ci_session_summarize_components",
          "ci_session_summarize_predictions", "ci_session_summarize_placebo",
          "ci_session_summarize_placebo_horizons", "ci_test_session_summarize_placebo_horizons",
          "ci_session_summarize_predictions_blocks", "ci_session_summarize_placebo_blocks", "ci_summarize_draws", "ci_summarize_draws_f64",
          "ci_summarize_draw_paths_f64",
          "ci_session_summarize_windows", "ci_ll_session_summarize_windows",
          "ci_session_summarize_paths", "ci_ll_session_summarize_paths",
          "ci_session_pool_trajectories", "ci_ll_session_pool_trajectories",
          "ci_session_pool_event_trajectories", "ci_session_pool_placebo",
          "ci_session_pool_placebo_blocks",
          "ci_session_pool_placebo_horizons", "ci_session_pool_placebo_horizons_blocks",
          "ci_session_pool_simulated_placebo", "ci_session_pool_simulated_placebo_blocks",
          "ci_session_simulate_placebo", "ci_session_simulate_placebo_blocks",
          "ci_session_set_link", "ci_session_value_mean",
          "ci_kalman_loglik", "ci_ll_session_create", "ci_ll_session_create2", "ci_ll_session_eval",
          "ci_ll_session_draw_latents", "ci_ll_session_hmc_run", "ci_ll_session_hmc_fetch",
          "ci_ll_session_algorithmic_bytes", "ci_ll_session_destroy", "ci_ll_session_create_batch",
          "ci_ll_session_hmc_summarize",
          "ci_comm_unique_id", "ci_comm_create", "ci_comm_info", "ci_comm_set_timeout", "ci_comm_barrier",
          "ci_comm_all_reduce", "ci_comm_all_gather", "ci_comm_session_all_gather",
          "ci_comm_ll_session_all_gather", "ci_comm_destroy", "ci_test_rng",
          "ci_test_dk_draw", "ci_test_session_summarize_paths", "ci_test_summarize_draw_paths_f64",
          "ci_test_session_simulate_placebo", "ci_test_session_pool_placebo_blocks",
          "ci_test_session_pool_simulated_placebo", "ci_test_session_pool_placebo_horizons")


def _check(rc: int):
  if rc != 0:
    raise NativeError(load().ci_last_error().decode("utf-8", "replace"))


def _symbol(lib, name: str):
  """The entry point `name` of the loaded library."""
  fn = getattr(lib, name, None)
  if fn is None:
    raise NativeError(f"the loaded library has no {name}: rebuild it")
  return fn


def _per_series(name: str, value, B: int, dtype=np.float64) -> np.ndarray:
  """`value`, a scalar or one entry per series, as a contiguous [B] array of `dtype`."""
  a = np.asarray(value)
  if a.shape not in ((), (B,)):
    raise ValueError(f"`{name}` must be a scalar or have one entry per series ({B}), got shape {a.shape}")
  return np.ascontiguousarray(np.broadcast_to(a, (B,)), dtype=dtype)


def _origin_plan(origins, horizon, B: int):
  """(origins [B, O] int32, horizon [B] int32) of `Session.summarize_placebo` and `simulate_placebo`:
  origins [B, O], or [O] for one series; horizon a scalar or [B]."""
  org = np.asarray(origins)
  if org.ndim == 1 and B == 1:
    org = org[None]
  if org.ndim != 2 or org.shape[0] != B:
    raise ValueError(f"`origins` must be [{B}, O], got shape {org.shape}")
  return np.ascontiguousarray(org, dtype=np.int32), _per_series("horizon", horizon, B, np.int32)


MAX_PLACEBO_HORIZONS = 64   # max_horizons of ci_session_summarize_placebo_horizons


def horizon_table(horizons, B: int, owner: str = "series") -> np.ndarray:
  """horizons [B, K] int32 of `Session.summarize_placebo_horizons`, from [B, K] or -- the same row for
  every series -- [K].  The rules the C entry checks, checked here first (ValueError, series and slot
  named): 1 <= K <= 64, every row with at least one horizon, each >= 1, strictly ascending, -1
  (unused) only at the end of the row.  `Session.pool_placebo_horizons` has one row per group
  (owner="group": what the messages call a row's owner)."""
  hz = np.asarray(horizons)
  if hz.ndim == 1:
    hz = np.broadcast_to(hz, (B,) + hz.shape)
  if hz.ndim != 2 or hz.shape[0] != B:
    raise ValueError(f"`horizons` must be [{B}, K] or [K], got shape {np.shape(horizons)}")
  if not np.issubdtype(hz.dtype, np.integer):
    if not (np.issubdtype(hz.dtype, np.floating) and np.all(hz == np.floor(hz))):
      raise ValueError(f"`horizons` must hold integers, got dtype {hz.dtype}")
  K = hz.shape[1]
  if not 1 <= K <= MAX_PLACEBO_HORIZONS:
    raise ValueError(f"`horizons` must have 1 to {MAX_PLACEBO_HORIZONS} slots per {owner}, got {K}")
  hz = np.ascontiguousarray(hz, dtype=np.int32)
  for b in range(B):
    row = hz[b]
    used = int(np.count_nonzero(row != -1))
    if used == 0:
      raise ValueError(f"horizons[{b}] holds no horizon: every {owner} needs at least one")
    for i in range(K):
      h = int(row[i])
      if h == -1:
        continue
      if h < 1:
        raise ValueError(f"horizons[{b}, {i}] must be at least 1, or -1 (unused), got {h}")
      if i >= used or (i > 0 and h <= int(row[i - 1])):
        raise ValueError(f"horizons[{b}] must be strictly ascending with the unused slots (-1) at the end "
                         f"(slot {i} holds {h})")
  return hz


def series_stream_key(seed, series_id: int):
  """(k0, k1): the Philox key of series `series_id` of a batch fitted with `seed` -- a
  single-series fit (device or oracle) with seed = this key reproduces that series' draws."""
  s = (C.c_uint32 * 2)(*[int(v) & 0xFFFFFFFF for v in seed_pair(seed)])
  k = (C.c_uint32 * 2)()
  load().ci_series_stream_key(s, int(series_id), k)
  return (int(k[0]), int(k[1]))


def device_count() -> int:
  n = C.c_int(0)
  _check(load().ci_device_count(C.byref(n)))
  return n.value


def device_synchronize(device: int = 0):
  """Waits for all work queued on `device` (ci_device_synchronize)."""
  _check(load().ci_device_synchronize(int(device)))


def pool_trim():
  """Returns the device buffers parked by finished sessions to the driver (ci_pool_trim)."""
  _check(load().ci_pool_trim())


def seed_pair(seed):
  """int s -> (0, s); pairs pass through (causalimpact_lib.py:535-539)."""
  if isinstance(seed, (int, np.integer)):
    return (0, int(seed) & 0xFFFFFFFF)
  a, b = seed
  return (int(a) & 0xFFFFFFFF, int(b) & 0xFFFFFFFF)


def make_params(specs: Sequence[Dict]) -> "C.Array":
  """ci_series_params[len(specs)] -- every member is a double, so the table is filled as one
  [n, 29] float64 block (a batch of 512 series: 15k ctypes attribute writes otherwise)."""
  n, nf = len(specs), len(_PARAM_FIELDS)
  buf = np.zeros((n, nf + MAX_BLOCKS + 1), np.float64)
  for i, sp in enumerate(specs):
    buf[i, :nf] = [sp[f] for f in _PARAM_FIELDS]
    d0 = sp.get("drift_scale0", ())
    if len(d0):
      buf[i, nf:nf + len(d0)] = d0
    buf[i, nf + MAX_BLOCKS] = sp.get("weights_prior_scale", 1.0)
  arr = (SeriesParams * n)()
  assert C.sizeof(arr) == buf.nbytes
  C.memmove(arr, buf.ctypes.data, buf.nbytes)
  return arr


FLAG_SEQUENTIAL_SEASONAL = 1   # == CI_FLAG_SEQUENTIAL_SEASONAL
FLAG_SHARED_SERIES_STREAMS = 2  # == CI_FLAG_SHARED_SERIES_STREAMS
FLAG_FOUR_WAVES = 4             # == CI_FLAG_FOUR_WAVES
FLAG_SEASONAL_WORKSPACE = 8     # == CI_FLAG_SEASONAL_WORKSPACE
FLAG_NO_CLUSTER = 16            # == CI_FLAG_NO_CLUSTER
FLAG_TEST_DROP_HELPER = 32      # == CI_FLAG_TEST_DROP_HELPER
FLAG_CLUSTER_SEASONAL = 64      # == CI_FLAG_CLUSTER_SEASONAL
FLAG_MULTIWAVE_SEASONAL = 128   # == CI_FLAG_MULTIWAVE_SEASONAL


def make_problem(*, T, P, has_slope, num_seasons=(), num_warmup, num_results, num_chains=1,
                 chain_offset=0, num_series=1, seed=(0, 0), device=0, flags=0,
                 series_offset=0) -> Problem:
  pb = Problem()
  pb.abi_version = ABI_VERSION
  pb.T, pb.P, pb.has_slope = int(T), int(P), int(bool(has_slope))
  pb.num_blocks = len(num_seasons)
  for k, n in enumerate(num_seasons):
    pb.num_seasons[k] = int(n)
  pb.num_warmup, pb.num_results = int(num_warmup), int(num_results)
  pb.num_chains, pb.chain_offset, pb.num_series = int(num_chains), int(chain_offset), int(num_series)
  s = seed_pair(seed)
  pb.seed[0], pb.seed[1] = s
  pb.device = int(device)
  pb.flags = int(flags)
  pb.series_offset = int(series_offset)
  return pb


def _stage_inputs(pb: Problem, y, mask, X, season_change):
  B, T, P, K = pb.num_series, pb.T, pb.P, pb.num_blocks
  mask8 = np.ascontiguousarray(np.asarray(mask, dtype=bool).reshape(B, T).astype(np.uint8))
  y32 = np.asarray(y, dtype=np.float32).reshape(B, T)
  y32 = np.ascontiguousarray(np.where(mask8 != 0, np.float32(0), y32))
  X32 = None
  if P > 0:
    X32 = np.ascontiguousarray(np.asarray(X, dtype=np.float32).reshape(B, T, P))
  sc = None
  if K > 0 and season_change is not None:
    sc = np.ascontiguousarray(np.asarray(season_change, dtype=np.uint8).reshape(K, T))
  return y32, mask8, X32, sc


def summarize_draws(trajectories, scale, shift, observed, flags, ranks, device=0):
  """ci_summarize_draws / ci_summarize_draws_f64: on-device summary of host-resident [draws, T]
  trajectories -- float64 draws (the float64 kernels) are summarised as float64, anything else as
  float32."""
  f64 = np.asarray(trajectories).dtype == np.float64
  tr = np.ascontiguousarray(trajectories, dtype=np.float64 if f64 else np.float32)
  N, T = tr.shape
  obs = np.ascontiguousarray(observed, dtype=np.float64).reshape(T)
  fl = np.ascontiguousarray(flags, dtype=np.uint8).reshape(T)
  rk = np.ascontiguousarray(ranks, dtype=np.int32)
  vo = np.empty((rk.size, T), np.float64)
  co = np.empty((rk.size, T), np.float64)
  pd_ = np.empty((2, N), np.float64)
  do = np.empty((2, rk.size), np.float64)
  fn = load().ci_summarize_draws_f64 if f64 else load().ci_summarize_draws
  _check(fn(int(device), N, T, tr.ctypes.data, float(scale), float(shift),
            obs.ctypes.data, fl.ctypes.data, int(rk.size), rk.ctypes.data,
            vo.ctypes.data, co.ctypes.data, pd_.ctypes.data, do.ctypes.data))
  return dict(value_order=vo, cum_order=co, per_draw=pd_, per_draw_order=do)


def link_values_host(z, link) -> np.ndarray:
  """The outcome link in numpy, float64: z itself (LINK_IDENTITY), np.exp(z) (LINK_LOG) or
  np.expm1(z) (LINK_LOG1P), z = trajectory * scale + shift in two roundings.  No clamp: an overflow
  is inf.  The definition the device's `value` under `Session.set_link` is compared with."""
  z = np.asarray(z, np.float64)
  if link == LINK_IDENTITY:
    return z
  if link not in (LINK_LOG, LINK_LOG1P):
    raise ValueError(f"unknown link {link!r}: LINK_IDENTITY = 0, LINK_LOG = 1, LINK_LOG1P = 2")
  with np.errstate(over="ignore"):
    return np.exp(z) if link == LINK_LOG else np.expm1(z)


def groups_csr(groups, num_series: int):
  """The sparse weight table of `pool_trajectories` in CSR form: (offsets [G + 1] int32, members
  int32, weights float64).  groups: a sequence with one entry per group, each a mapping {position
  of a series in the session: weight} or a sequence of positions (weight 1).  Members are sorted
  by position and those of zero weight left out; a group may be empty.  ValueError for a position
  outside [0, num_series), a repeated member or a weight that is not finite."""
  offsets, members, weights = [0], [], []
  for g, group in enumerate(groups):
    items = group.items() if hasattr(group, "items") else [(b, 1.0) for b in group]
    items = sorted((int(b), float(w)) for b, w in items)
    for i, (b, w) in enumerate(items):
      if not 0 <= b < num_series:
        raise ValueError(f"group {g}: member {b} is outside [0, {num_series})")
      if i and b == items[i - 1][0]:
        raise ValueError(f"group {g}: member {b} is listed twice")
      if not np.isfinite(w):
        raise ValueError(f"group {g}: the weight of member {b} is not finite")
      if w != 0.0:
        members.append(b)
        weights.append(w)
    offsets.append(len(members))
  return (np.asarray(offsets, np.int32), np.asarray(members, np.int32),
          np.asarray(weights, np.float64))


def pool_host(trajectories, scale, shift, groups, init=None) -> np.ndarray:
  """What `pool_trajectories` computes, in numpy: trajectories [B, N, T] (any float type), scale,
  shift [B], groups as for `groups_csr`; returns [G, N, T] float64.  One rounding per operation,
  members in ascending order -- the loop of include/causalimpact_amd.h -- so it is the definition the
  device is compared with, and the accumulator of the batch routes that fit series by series."""
  tr = np.asarray(trajectories)
  B = tr.shape[0]
  offsets, members, weights = groups_csr(groups, B)
  sc = np.broadcast_to(np.asarray(scale, np.float64), (B,))
  sh = np.broadcast_to(np.asarray(shift, np.float64), (B,))
  out = (np.zeros((len(offsets) - 1,) + tr.shape[1:], np.float64) if init is None
         else np.array(init, np.float64).reshape((len(offsets) - 1,) + tr.shape[1:]))
  for g in range(len(offsets) - 1):
    for k in range(offsets[g], offsets[g + 1]):
      b = members[k]
      out[g] = out[g] + weights[k] * (tr[b].astype(np.float64) * sc[b] + sh[b])
  return out


def _entry_csr(groups, num_series: int):
  """`groups` as (offsets, members, weights): the tables themselves, or what `groups_csr` takes."""
  if isinstance(groups, tuple) and len(groups) == 3 and isinstance(groups[0], np.ndarray):
    return groups
  return groups_csr(groups, num_series)


def philox4x32_10_host(counter, key) -> np.ndarray:
  """Philox4x32-10 of csrc/ci_rng.h in numpy: counter [..., 4] and key [..., 2] (broadcast against
  each other over the leading axes), unsigned 32-bit words; returns the four output words [..., 4]
  as uint32."""
  ctr = np.asarray(counter, np.uint64) & np.uint64(0xFFFFFFFF)
  k = np.asarray(key, np.uint64) & np.uint64(0xFFFFFFFF)
  shape = np.broadcast_shapes(ctr.shape[:-1], k.shape[:-1])
  c0, c1, c2, c3 = (np.broadcast_to(ctr[..., i], shape).copy() for i in range(4))
  k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
  m32, sh32 = np.uint64(0xFFFFFFFF), np.uint64(32)
  for _ in range(10):
    p0 = np.uint64(0xD2511F53) * c0
    p1 = np.uint64(0xCD9E8D57) * c2
    c0, c1, c2, c3 = (p1 >> sh32) ^ c1 ^ k0, p1 & m32, (p0 >> sh32) ^ c3 ^ k1, p0 & m32
    k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
  return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def normals_host(key, chain, iteration, site: int, sub, idx) -> np.ndarray:
  """`normal_d` of csrc/ci_rng.h in vectorised numpy: the float64 Box-Muller normal of element `idx`
  of (site, sub) in iteration `iteration` of chain `chain` under the Philox key `key` (k0, k1) --
  counter (idx >> 2, site | sub << 8, iteration, chain), component idx & 3.  chain, iteration, sub
  and idx broadcast against each other.  The angle is 2 pi rev through cos and sin, as the oracle
  takes it (the device uses sincospi: the same value to a few ulp)."""
  chain, iteration, sub, idx = np.broadcast_arrays(*(np.asarray(v, np.uint64) for v in (chain, iteration, sub, idx)))
  counter = np.stack([idx >> np.uint64(2), np.uint64(int(site)) | (sub << np.uint64(8)), iteration, chain], axis=-1)
  words = philox4x32_10_host(counter, np.asarray([int(key[0]), int(key[1])], np.uint64)).astype(np.float64)
  hi = (idx & np.uint64(2)) != 0
  ra = np.where(hi, words[..., 2], words[..., 0])
  rb = np.where(hi, words[..., 3], words[..., 1])
  u1 = (ra + 0.5) * (1.0 / 4294967296.0)
  rev = rb * (1.0 / 4294967296.0)
  rad = np.sqrt(-2.0 * np.log(u1))
  angle = (2.0 * np.pi) * rev
  return np.where((idx & np.uint64(1)) != 0, rad * np.sin(angle), rad * np.cos(angle))


def row_means_host(M) -> np.ndarray:
  """The mean of every row of M [..., N] as the row-statistics kernel takes it
  (csrc/ci_components.h): lane l of 64 adds the values l, l + 64, .. ascending from 0.0, the 64 sums
  are combined by a butterfly (partners 32, 16, .., 1 apart), and the result is divided by N."""
  M = np.asarray(M, np.float64)
  N = M.shape[-1]
  pad = (-N) % 64
  padded = np.concatenate([M, np.zeros(M.shape[:-1] + (pad,))], axis=-1) if pad else M
  lanes = np.zeros(M.shape[:-1] + (64,))
  for chunk in range(padded.shape[-1] // 64):                     # (a padded 0.0 leaves a sum unchanged)
    lanes = lanes + padded[..., 64 * chunk:64 * chunk + 64]
  for off in (32, 16, 8, 4, 2, 1):
    lanes = lanes + lanes[..., np.arange(64) ^ off]
  return lanes[..., 0] / np.float64(N)


def placebo_terms_host(mean, variance, counted, scale, shift):
  """What one entry adds to a pooled placebo forecast, on the data scale: (s, v) from the per-draw C,
  V [O, N] and cnt [O] of `causalimpact_lib._placebo_summary_host(per_draw=True)` --
  s = C * scale + cnt * shift (separate roundings), v = (V * scale) * scale, both 0 where cnt == 0.
  At several horizons (`horizons=`): C, V [O, K, N] and cnt [O, K], likewise."""
  C_, V_ = np.asarray(mean, np.float64), np.asarray(variance, np.float64)
  cnt = np.asarray(counted, np.float64).reshape(C_.shape[:-1] + (1,))
  scale, shift = np.float64(scale), np.float64(shift)
  some = cnt > 0
  return np.where(some, C_ * scale + cnt * shift, 0.0), np.where(some, (V_ * scale) * scale, 0.0)


def pool_placebo_host(sums, variances, groups, init=None) -> np.ndarray:
  """What `Session.pool_placebo` accumulates, in numpy: sums, variances [K, O, N] -- per entry of the
  group table, in its order, the s and v of `placebo_terms_host` -- and groups: the (offsets, members,
  weights) of `groups_csr`, or what it takes (the entries are then the members of non-zero weight,
  group after group, ascending).  Returns acc [G, O, 2, N] float64:
    acc[g, :, 0] = init[g, :, 0] + sum over the group's entries k, ascending, of w_k * s_k
    acc[g, :, 1] = init[g, :, 1] + sum over the same entries of (w_k * w_k) * v_k
  one rounding per operation -- the loop of include/causalimpact_amd.h.  Given every member's draw the
  pooled sum is N(S, U) IF the members are independent of each other; that is the assumption the
  pooled placebo tests."""
  s_, v_ = np.asarray(sums, np.float64), np.asarray(variances, np.float64)
  if s_.ndim != 3 or s_.shape != v_.shape:
    raise ValueError(f"`sums` and `variances` must both be [K, O, N], got {s_.shape} and {v_.shape}")
  offsets, _, weights = _entry_csr(groups, np.iinfo(np.int32).max)
  G = len(offsets) - 1
  if offsets[G] != s_.shape[0]:
    raise ValueError(f"the groups have {offsets[G]} entries, `sums` has {s_.shape[0]}")
  shape = (G, s_.shape[1], 2, s_.shape[2])
  out = np.zeros(shape, np.float64) if init is None else np.array(init, np.float64).reshape(shape)
  for g in range(G):
    for k in range(offsets[g], offsets[g + 1]):
      w = np.float64(weights[k])
      out[g, :, 0] = out[g, :, 0] + w * s_[k]
      out[g, :, 1] = out[g, :, 1] + (w * w) * v_[k]
  return out


_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def pool_placebo_horizons_host(sums, variances, groups, init=None) -> np.ndarray:
  """What `Session.pool_placebo_horizons` accumulates, in numpy: sums, variances [E, O, K, N] -- per
  entry of the group table the s and v of `placebo_terms_host` at the K checkpoints of its group's
  horizon row, 0 in the unused slots -- and groups as for `pool_placebo_host`.  Returns acc
  [G, O, K, 2, N]: `pool_placebo_host` over the O * K slots, so acc[:, :, k] is its result for column k
  and `init` [G, O, K, 2, N] continues it bit for bit."""
  s_, v_ = np.asarray(sums, np.float64), np.asarray(variances, np.float64)
  if s_.ndim != 4 or s_.shape != v_.shape:
    raise ValueError(f"`sums` and `variances` must both be [E, O, K, N], got {s_.shape} and {v_.shape}")
  E, O, K, N = s_.shape
  if init is not None:
    init = np.asarray(init, np.float64).reshape(-1, O * K, 2, N)
  acc = pool_placebo_host(s_.reshape(E, O * K, N), v_.reshape(E, O * K, N), groups, init)
  return acc.reshape(acc.shape[0], O, K, 2, N)


def finish_placebo_horizons_host(acc, seen) -> Dict[str, np.ndarray]:
  """The finishing step of `Session.pool_placebo_horizons` in numpy: acc [G, O, K, 2, N], seen [G, O, K]
  -> predicted_mean, spread_mean, pit_mean [G, O, K]: `finish_placebo_host` over the O * K slots."""
  acc = np.asarray(acc, np.float64)
  G, O, K, _, N = acc.shape
  res = finish_placebo_host(acc.reshape(G, O * K, 2, N), np.asarray(seen, np.float64).reshape(G, O * K))
  return {k: v.reshape(G, O, K) for k, v in res.items()}


def finish_placebo_host(acc, seen) -> Dict[str, np.ndarray]:
  """The finishing step of `Session.pool_placebo` in numpy: acc [G, O, 2, N] (S, U), seen [G, O] the
  pooled observed sums -> predicted_mean, spread_mean, pit_mean [G, O], the means over the draws of
  SUM = S, SPREAD = U + e^2, PIT = 0.5 erfc(-e / sqrt(2 U)) with e = seen - S; 0 where U == 0."""
  acc = np.asarray(acc, np.float64)
  S, U = acc[:, :, 0], acc[:, :, 1]
  some = U != 0.0
  with np.errstate(invalid="ignore", divide="ignore"):
    e = np.asarray(seen, np.float64)[:, :, None] - S
    spread = np.where(some, U + e * e, 0.0)
    pit = np.where(some, 0.5 * _erfc(np.where(some, -e / np.sqrt(2.0 * np.where(some, U, 1.0)), 0.0)), 0.0)
  # (draws first: the mean adds them in ascending order, as `_placebo_summary_host` takes its means)
  mean = lambda x: np.ascontiguousarray(np.moveaxis(x, 2, 0)).mean(axis=0)   # pylint: disable=unnecessary-lambda-assignment
  return dict(predicted_mean=mean(np.where(some, S, 0.0)), spread_mean=mean(spread), pit_mean=mean(pit))


def pool_simulated_placebo_host(totals, groups, init=None) -> np.ndarray:
  """What `Session.pool_simulated_placebo` accumulates, in numpy: totals [K, O, N] -- per entry of the
  group table, in its order, the simulated totals of its member at the entry's origins and the
  group's horizon (0 where nothing is counted) -- and groups as for `pool_placebo_host`.  Returns acc
  [G, O, N] float64:
    acc[g] = init[g] + sum over the group's entries k, ascending, of w_k * totals[k]
  one rounding per operation -- the loop of include/causalimpact_amd.h."""
  t_ = np.asarray(totals, np.float64)
  if t_.ndim != 3:
    raise ValueError(f"`totals` must be [K, O, N], got {t_.shape}")
  offsets, _, weights = _entry_csr(groups, np.iinfo(np.int32).max)
  G = len(offsets) - 1
  if offsets[G] != t_.shape[0]:
    raise ValueError(f"the groups have {offsets[G]} entries, `totals` has {t_.shape[0]}")
  shape = (G,) + t_.shape[1:]
  out = np.zeros(shape, np.float64) if init is None else np.array(init, np.float64).reshape(shape)
  for g in range(G):
    for k in range(offsets[g], offsets[g + 1]):
      out[g] = out[g] + np.float64(weights[k]) * t_[k]
  return out


def finish_simulated_placebo_host(acc, seen, counted, ranks=()) -> Dict[str, np.ndarray]:
  """The finishing step of `Session.pool_simulated_placebo` in numpy: acc [G, O, N] the pooled
  simulated totals, seen [G, O] the pooled observed totals, counted [G, O] the member-steps every
  window counts -> the statistics of `simulate_placebo` over the rows of acc: predicted_mean (as
  `row_means_host`), spread_mean (the mean of (acc - seen)^2), below (#{n: acc <= seen}) [G, O] and
  total_order [G, R, O]; spread_mean and below 0 where counted == 0 (acc is 0.0 there)."""
  acc = np.asarray(acc, np.float64)
  some = np.asarray(counted) > 0
  seen = np.where(some, np.nan_to_num(np.asarray(seen, np.float64)), 0.0)
  dev = acc - seen[..., None]
  return dict(predicted_mean=row_means_host(acc),
              spread_mean=np.where(some, row_means_host(dev * dev), 0.0),
              below=np.where(some, np.count_nonzero(acc <= seen[..., None], axis=-1), 0).astype(np.float64),
              total_order=np.ascontiguousarray(np.moveaxis(np.sort(acc, axis=-1)[..., list(ranks)], -1, -2)))


def _pool_call(fn, handle, B: int, N: int, T: int, scale, shift, groups, init, event=False,
               out_stride=None) -> np.ndarray:
  """The call every session's `pool_trajectories` and `pool_event_trajectories` (event=True: the
  tables of `event_groups_csr` and rows of out_stride columns) make."""
  sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, np.float64), (B,)))
  sh = np.ascontiguousarray(np.broadcast_to(np.asarray(shift, np.float64), (B,)))
  csr = (event_groups_csr if event else groups_csr)(groups, B)
  G, stride = csr[0].size - 1, _event_stride(csr[4], out_stride) if event else T
  tables = [a.ctypes.data for a in csr] + ([stride] if event else [])
  if init is not None:
    init = np.ascontiguousarray(init, dtype=np.float64)
    if init.shape != (G, N, stride):
      raise ValueError(f"`init` must be {[G, N, stride]}, got {list(init.shape)}")
  big = G * N * stride * 8 > (1 << 20)
  out = pinned_empty((G, N, stride), np.float64) if big else np.empty((G, N, stride), np.float64)
  _check(fn(handle, sc.ctypes.data, sh.ctypes.data, G, *tables, _ptr(init), out.ctypes.data))
  return out


def event_groups_csr(groups, num_series: int):
  """The tables of `pool_event_trajectories`: (offsets [G + 1], members, weights, first, width).
  groups: one (members, width) pair per group, members a mapping {position of a series in the
  session: (weight, first)} -- `first` the step of that series that lands in column 0 of the group --
  and width the number of columns of the group.  The first three arrays are `groups_csr`'s (members
  ascending, those of zero weight left out, the same refusals); first int32 is parallel to members,
  width int32 [G]."""
  groups = [(dict(members), int(width)) for members, width in groups]
  offsets, members, weights = groups_csr(
      [{b: w for b, (w, _) in group.items()} for group, _ in groups], num_series)
  first = [int(groups[g][0][int(b)][1]) for g in range(len(groups))
           for b in members[offsets[g]:offsets[g + 1]]]
  return (offsets, members, weights, np.asarray(first, np.int32),
          np.asarray([width for _, width in groups], np.int32))


def _event_stride(width, out_stride) -> int:
  stride = int(width.max()) if out_stride is None else int(out_stride)
  if width.size and (width.min() < 1 or width.max() > stride):
    raise ValueError(f"every width must be in [1, out_stride = {stride}], got {width.tolist()}")
  return stride


def pool_event_host(trajectories, scale, shift, groups, init=None, out_stride=None) -> np.ndarray:
  """What `pool_event_trajectories` computes, in numpy: trajectories [B, N, T] (any float type),
  scale, shift [B], groups as for `event_groups_csr`; returns [G, N, out_stride] float64 (out_stride:
  the widest group by default).  out[g][:, :width] = init[g][:, :width] + the sum over the members,
  ascending, of weight * (trajectory[:, first : first + width] * scale + shift), one rounding per
  operation; the columns beyond a group's width are 0.0.  The definition the device is compared
  with."""
  tr = np.asarray(trajectories)
  B = tr.shape[0]
  offsets, members, weights, first, width = event_groups_csr(groups, B)
  stride = _event_stride(width, out_stride)
  sc = np.broadcast_to(np.asarray(scale, np.float64), (B,))
  sh = np.broadcast_to(np.asarray(shift, np.float64), (B,))
  out = np.zeros((width.size, tr.shape[1], stride), np.float64)
  for g, W in enumerate(width):
    if init is not None:
      out[g, :, :W] = np.asarray(init, np.float64)[g, :, :W]
    for k in range(offsets[g], offsets[g + 1]):
      b, f = members[k], first[k]
      if f < 0 or f + W > tr.shape[2]:
        raise ValueError(f"group {g}: member {b} from step {f} over {W} columns leaves [0, {tr.shape[2]})")
      out[g, :, :W] = out[g, :, :W] + weights[k] * (tr[b, :, f:f + W].astype(np.float64) * sc[b] + sh[b])
  return out


def window_totals_host(trajectories, scale, shift, observed, first, count) -> np.ndarray:
  """What `summarize_windows` computes, as a plain loop: trajectories [B, N, T] (float32 or float64),
  scale, shift scalars or [B], observed [T] or [B, T] (NaN = no observation), first, count [W] or
  [B, W] in steps.  Returns per_draw [B, W, 2, N] float64: for every series, window and draw the sum
  over the window's steps, ascending, of value = trajectory * scale + shift (two roundings) and of
  -(value - observed) with the NaN steps skipped; count = 0 gives 0.0.  One rounding per operation,
  in the order of include/causalimpact_amd.h -- so it is the definition the device is compared with,
  and the route of the fits whose draws are pooled on the host."""
  tr = np.asarray(trajectories)
  if tr.ndim != 3:
    raise ValueError(f"`trajectories` must be [B, N, T], got shape {tr.shape}")
  B, N, T = tr.shape
  sc = np.broadcast_to(np.asarray(scale, np.float64), (B,))
  sh = np.broadcast_to(np.asarray(shift, np.float64), (B,))
  obs = np.broadcast_to(np.asarray(observed, np.float64), (B, T))
  fi = np.asarray(first, np.int64)
  fi = np.broadcast_to(fi, (B,) + fi.shape[-1:])
  co = np.broadcast_to(np.asarray(count, np.int64), fi.shape)
  W = fi.shape[1]
  out = np.zeros((B, W, 2, N), np.float64)
  for b in range(B):
    for w in range(W):
      f, c = int(fi[b, w]), int(co[b, w])
      if f < 0 or c < 0 or f + c > T:
        raise ValueError(f"window {w} of series {b}: steps {f} .. {f + c - 1} leave [0, {T})")
      pred_sum, point_sum = np.zeros(N, np.float64), np.zeros(N, np.float64)
      for t in range(f, f + c):
        v = tr[b, :, t].astype(np.float64) * sc[b] + sh[b]
        pred_sum = pred_sum + v
        point = -(v - obs[b, t])
        point_sum = np.where(point == point, point_sum + point, point_sum)
      out[b, w, 0], out[b, w, 1] = pred_sum, point_sum
  return out


def _windows_call(fn, handle, B: int, N: int, T: int, scale, shift, observed, first, count, ranks,
                  want_draws: bool) -> Dict[str, np.ndarray]:
  """The call every session's `summarize_windows` makes."""
  sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, np.float64), (B,)))
  sh = np.ascontiguousarray(np.broadcast_to(np.asarray(shift, np.float64), (B,)))
  obs = np.ascontiguousarray(np.broadcast_to(np.asarray(observed, np.float64), (B, T)))
  fi = np.asarray(first, np.int32)
  if fi.ndim not in (1, 2) or (fi.ndim == 2 and fi.shape[0] != B):
    raise ValueError(f"`first` must be [W] or [{B}, W], got shape {fi.shape}")
  fi = np.ascontiguousarray(np.broadcast_to(fi, (B, fi.shape[-1])))
  co = np.asarray(count, np.int32)
  if co.shape not in (fi.shape, fi.shape[1:]):
    raise ValueError(f"`count` must have the shape of `first`, got {co.shape}")
  co = np.ascontiguousarray(np.broadcast_to(co, fi.shape))
  rk = np.ascontiguousarray(ranks, dtype=np.int32).reshape(-1)
  W = fi.shape[1]
  pd_ = np.empty((B, W, 2, N), np.float64) if want_draws else None
  do = np.empty((B, W, 2, rk.size), np.float64)
  _check(fn(handle, sc.ctypes.data, sh.ctypes.data, obs.ctypes.data, W, fi.ctypes.data, co.ctypes.data,
            int(rk.size), rk.ctypes.data, _ptr(pd_), do.ctypes.data))
  out = dict(per_draw_order=do)
  if want_draws:
    out["per_draw"] = pd_
  return out


PATH_OUTPUTS = ("center", "spread", "excursion", "excursion_order", "observed_excursion", "at", "exceed")


def path_excursions_host(trajectories, scale, shift, observed, first, count, ranks=None, center=None,
                         spread=None) -> Dict[str, np.ndarray]:
  """What `summarize_paths` computes, as a plain loop (the definitions of ci_session_summarize_paths,
  include/causalimpact_amd.h): trajectories [B, N, T] (float32 or float64), scale, shift scalars or
  [B], observed [T] or [B, T] (NaN = no observation), first, count [W] or [B, W] in steps.  For every
  series, window and path k (0: the prediction against the observations; 1: the running sum of the
  point effects against 0.0) the moments over the draws center, spread [B, W, 2, T] (NaN outside the
  window and, for path 1, at the steps without an observation), every draw's largest standardised
  excursion over the counted steps -- those with an observation and spread > 0 -- excursion
  [B, W, 2, N], observed_excursion [B, W, 2] (NaN: no counted step), at [B, W, 2] (its first step, -1:
  none), exceed [B, W, 2] = #{n: excursion >= observed_excursion}, excursion_order [B, W, 2, R] with
  `ranks`, and x [B, W, 2, N, T], the paths themselves (NaN outside the window).  center=, spread=
  [B, W, 2, T]: the second stage from these moments instead of its own -- given the device's, every
  other array is the device's bit for bit; its own moments add the draws in numpy's order.  It is the
  definition the device is compared with, and the route of the fits whose draws are pooled on the
  host."""
  tr = np.asarray(trajectories)
  if tr.ndim != 3:
    raise ValueError(f"`trajectories` must be [B, N, T], got shape {tr.shape}")
  B, N, T = tr.shape
  sc = np.broadcast_to(np.asarray(scale, np.float64), (B,))
  sh = np.broadcast_to(np.asarray(shift, np.float64), (B,))
  obs = np.broadcast_to(np.asarray(observed, np.float64), (B, T))
  fi = np.asarray(first, np.int64)
  fi = np.broadcast_to(fi, (B,) + fi.shape[-1:])
  co = np.broadcast_to(np.asarray(count, np.int64), fi.shape)
  W = fi.shape[1]
  given = center is not None
  if given != (spread is not None):
    raise ValueError("`center` and `spread` go together")
  out = dict(center=np.full((B, W, 2, T), np.nan), spread=np.full((B, W, 2, T), np.nan),
             excursion=np.zeros((B, W, 2, N)), observed_excursion=np.full((B, W, 2), np.nan),
             at=np.full((B, W, 2), -1, np.int32), exceed=np.zeros((B, W, 2), np.int32),
             x=np.full((B, W, 2, N, T), np.nan))
  with np.errstate(invalid="ignore", divide="ignore"):
    for b in range(B):
      for w in range(W):
        f, c = int(fi[b, w]), int(co[b, w])
        if f < 0 or c < 0 or f + c > T:
          raise ValueError(f"window {w} of series {b}: steps {f} .. {f + c - 1} leave [0, {T})")
        point_sum = np.zeros(N, np.float64)
        for t in range(f, f + c):
          v = tr[b, :, t].astype(np.float64) * sc[b] + sh[b]
          point = -(v - obs[b, t])
          point_sum = np.where(point == point, point_sum + point, point_sum)
          out["x"][b, w, 0, :, t], out["x"][b, w, 1, :, t] = v, point_sum
        for k in range(2):
          x, best, seen, where = out["x"][b, w, k], np.zeros(N, np.float64), np.nan, -1
          for t in range(f, f + c):
            has_obs = obs[b, t] == obs[b, t]
            if given:
              ce, sp = np.float64(center[b, w, k, t]), np.float64(spread[b, w, k, t])
            else:
              ce = x[:, t].sum() / N
              dev = x[:, t] - ce
              sp = np.sqrt((dev * dev).sum() / np.float64(N - 1)) if N > 1 else np.float64(np.nan)
              if k == 0 or has_obs:
                out["center"][b, w, k, t], out["spread"][b, w, k, t] = ce, sp
            if not has_obs or not sp > 0.0:
              continue
            z = np.abs(x[:, t] - ce) / sp
            best = np.where(z > best, z, best)
            zo = np.abs((0.0 if k else obs[b, t]) - ce) / sp
            if where < 0 or zo > seen:
              seen, where = zo, t
          if given:
            out["center"][b, w, k], out["spread"][b, w, k] = center[b, w, k], spread[b, w, k]
          out["excursion"][b, w, k], out["observed_excursion"][b, w, k] = best, seen
          out["at"][b, w, k], out["exceed"][b, w, k] = where, np.count_nonzero(best >= seen)
  if ranks is not None:
    rk = np.asarray(ranks, np.int64).reshape(-1)
    out["excursion_order"] = np.sort(out["excursion"], axis=-1)[..., rk]
  return out


_NO_SESSION = object()          # `_paths_call`'s handle for an entry that has no session


def _paths_call(fn, handle, B: int, N: int, T: int, scale, shift, observed, first, count, ranks,
                want, extra=()) -> Dict[str, np.ndarray]:
  """The call every session's `summarize_paths` makes; want: the `PATH_OUTPUTS` to return."""
  sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, np.float64), (B,)))
  sh = np.ascontiguousarray(np.broadcast_to(np.asarray(shift, np.float64), (B,)))
  obs = np.ascontiguousarray(np.broadcast_to(np.asarray(observed, np.float64), (B, T)))
  fi = np.asarray(first, np.int32)
  if fi.ndim not in (1, 2) or (fi.ndim == 2 and fi.shape[0] != B):
    raise ValueError(f"`first` must be [W] or [{B}, W], got shape {fi.shape}")
  fi = np.ascontiguousarray(np.broadcast_to(fi, (B, fi.shape[-1])))
  co = np.asarray(count, np.int32)
  if co.shape not in (fi.shape, fi.shape[1:]):
    raise ValueError(f"`count` must have the shape of `first`, got {co.shape}")
  co = np.ascontiguousarray(np.broadcast_to(co, fi.shape))
  rk = np.ascontiguousarray(ranks, dtype=np.int32).reshape(-1)
  W = fi.shape[1]
  unknown = set(want) - set(PATH_OUTPUTS)
  if unknown:
    raise ValueError(f"unknown path outputs {sorted(unknown)}")
  shapes = dict(center=(B, W, 2, T), spread=(B, W, 2, T), excursion=(B, W, 2, N),
                excursion_order=(B, W, 2, rk.size), observed_excursion=(B, W, 2), at=(B, W, 2),
                exceed=(B, W, 2))
  arrs = {k: np.empty(shapes[k], np.int32 if k in ("at", "exceed") else np.float64)
          for k in PATH_OUTPUTS if k in want}
  args = (sc.ctypes.data, sh.ctypes.data, obs.ctypes.data, W, fi.ctypes.data, co.ctypes.data,
          int(rk.size), rk.ctypes.data, *[_ptr(arrs.get(k)) for k in PATH_OUTPUTS], *extra)
  _check(fn(*args) if handle is _NO_SESSION else fn(handle, *args))
  return arrs


def summarize_draw_paths(draws, scale, shift, observed, first, count, ranks, want=PATH_OUTPUTS, device=0,
                         max_bytes=None) -> Dict[str, np.ndarray]:
  """`Session.summarize_paths` for float64 draws [G, N, T] that are on the host and belong to no
  session -- the pooled draws of groups of series -- on device `device`
  (ci_summarize_draw_paths_f64; first pass: path_values_f64_kernel of csrc/ci_paths.h, the other passes
  the session route's own).  scale, shift: scalars or [G] (pooled draws are on the data scale: 1.0,
  0.0); observed [T] or [G, T]; first, count [W] or [G, W]; want: the `PATH_OUTPUTS` to return, the
  group axis in front.  `path_excursions_host` is the same in numpy.  max_bytes (tests): the limit of
  the call's device memory in place of the library's (ci_test_summarize_draw_paths_f64); the result
  then has "num_chunks" too."""
  name = "ci_summarize_draw_paths_f64" if max_bytes is None else "ci_test_summarize_draw_paths_f64"
  fn = _symbol(load(), name)
  dr = np.ascontiguousarray(draws, dtype=np.float64)
  if dr.ndim != 3:
    raise ValueError(f"`draws` must be [G, N, T], got shape {dr.shape}")
  G, N, T = dr.shape
  chunks = C.c_int32(0)
  head = lambda *rest: fn(int(device), G, N, T, dr.ctypes.data, *rest)   # pylint: disable=unnecessary-lambda-assignment
  out = _paths_call(head, _NO_SESSION, G, N, T, scale, shift, observed, first, count, ranks, want,
                    () if max_bytes is None else (int(max_bytes), C.addressof(chunks)))
  if max_bytes is not None:
    out["num_chunks"] = chunks.value
  return out


class _PinnedBlock:
  """Owner of one ci_host_alloc buffer: returned to the library's pool when the last numpy view
  of it is collected."""

  def __init__(self, nbytes: int):
    self.ptr = C.c_void_p()
    _check(load().ci_host_alloc(C.byref(self.ptr), max(int(nbytes), 1)))
    self.nbytes = int(nbytes)

  def __del__(self):
    try:
      if self.ptr:
        load().ci_host_free(self.ptr)
        self.ptr = C.c_void_p()
    except Exception:  # pylint: disable=broad-except
      pass


def pinned_empty(shape, dtype=np.float32) -> np.ndarray:
  """An uninitialised numpy array in pinned host memory (ci_host_alloc): device-to-host copies
  into it run at PCIe rate and overlap the fit (`Session.run_streamed`)."""
  dtype = np.dtype(dtype)
  n = int(np.prod(shape, dtype=np.int64))
  block = _PinnedBlock(n * dtype.itemsize)
  buf = (C.c_char * max(n * dtype.itemsize, 1)).from_address(block.ptr.value)
  buf._pinned_owner = block   # keeps the allocation alive as long as any view of `buf`
  return np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)


def output_shapes(pb: Problem) -> Dict[str, tuple]:
  """Shapes of the members of ci_outputs for this problem (chain-major, per device)."""
  B, C_, S, T, P, K = pb.num_series, pb.num_chains, pb.num_results, pb.T, pb.P, pb.num_blocks
  return dict(
      observation_noise_scale=(B, C_, S), level_scale=(B, C_, S), slope_scale=(B, C_, S),
      seasonal_drift_scales=(B, C_, S, K), weights=(B, C_, S, P), level=(B, C_, S, T),
      slope=(B, C_, S, T), seasonal_levels=(B, C_, S, T, K), posterior_means=(B, C_, T),
      posterior_trajectories=(B, C_, S, T))


def _alloc_outputs(pb: Problem, want: Optional[Sequence[str]] = None, pinned: bool = False):
  shapes = output_shapes(pb)
  out, arrs = Outputs(), {}
  for name, shp in shapes.items():
    if want is not None and name not in want:
      continue
    a = pinned_empty(shp) if (pinned and int(np.prod(shp)) > 0) else np.zeros(shp, dtype=np.float32)
    arrs[name] = a
    setattr(out, name, a.ctypes.data if a.size else None)
  return out, arrs


def _ptr(a):
  return None if a is None else a.ctypes.data


def fit_gibbs(pb: Problem, y, mask, X, season_change, params, want=None) -> Dict[str, np.ndarray]:
  """One-shot upload -> W+S Gibbs iterations for B*C chains -> download."""
  L = load()
  y32, mask8, X32, sc = _stage_inputs(pb, y, mask, X, season_change)
  out, arrs = _alloc_outputs(pb, want)
  _check(L.ci_fit_gibbs(C.byref(pb), _ptr(y32), _ptr(mask8), _ptr(X32), _ptr(sc), params,
                        C.byref(out)))
  return arrs


def fit_gibbs_f64(pb: Problem, y, mask, X, season_change, params, want=None) -> Dict[str, np.ndarray]:
  """The float64 fit (ci_fit_gibbs_f64): every input and result array float64, any model."""
  L = load()
  B, T, P, K = pb.num_series, pb.T, pb.P, pb.num_blocks
  mask8 = np.ascontiguousarray(np.asarray(mask, dtype=bool).reshape(B, T).astype(np.uint8))
  y64 = np.ascontiguousarray(np.where(mask8 != 0, 0.0, np.asarray(y, np.float64).reshape(B, T)))
  X64 = np.ascontiguousarray(np.asarray(X, np.float64).reshape(B, T, P)) if P > 0 else None
  sc = (np.ascontiguousarray(np.asarray(season_change, dtype=np.uint8).reshape(K, T))
        if K > 0 else None)
  out, arrs = Outputs(), {}
  for name, shp in output_shapes(pb).items():
    if want is not None and name not in want:
      continue
    a = np.zeros(shp, dtype=np.float64)
    arrs[name] = a
    setattr(out, name, a.ctypes.data if a.size else None)
  _check(L.ci_fit_gibbs_f64(C.byref(pb), _ptr(y64), _ptr(mask8), _ptr(X64), _ptr(sc), params,
                            C.byref(out)))
  return arrs


def fit_gibbs_f64_kernel_ms() -> float:
  """Duration of the sampling kernel of this thread's last fit_gibbs_f64 (HIP events)."""
  ms = C.c_float()
  _check(load().ci_fit_gibbs_f64_kernel_ms(C.byref(ms)))
  return float(ms.value)


def fit_gibbs_f64_route(pb: Problem) -> Dict[str, int]:
  """The route fit_gibbs_f64 takes for `pb` (ci_fit_gibbs_f64_route; host arithmetic, no device):
  global_ws / reg_lds -- arrays over time / regression block in the HBM workspace or in LDS,
  trend_kernel -- eight-wavefront trend kernel or the sequential one, lds_bytes of the launch.
  Raises what the fit would raise for a shape it refuses."""
  gws, reg, trend, lds = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
  _check(load().ci_fit_gibbs_f64_route(C.byref(pb), C.byref(gws), C.byref(reg), C.byref(trend),
                                       C.byref(lds)))
  return dict(global_ws=gws.value, reg_lds=reg.value, trend_kernel=trend.value, lds_bytes=lds.value)


class Session:
  """Device-resident fit (inputs and outputs live in HBM between run() calls)."""

  # the kinds of `causalimpact_lib.SummaryRecord` this session takes on the device
  summaries = ("effect", "components", "predictions", "windows", "placebo", "paths")

  def __init__(self, pb: Problem, y, mask, X, season_change, params):
    self._lib = load()
    self.pb = pb
    y32, mask8, X32, sc = _stage_inputs(pb, y, mask, X, season_change)
    self._h = C.c_void_p()
    _check(self._lib.ci_session_create(C.byref(pb), _ptr(y32), _ptr(mask8), _ptr(X32), _ptr(sc),
                                       params, C.byref(self._h)))

  @classmethod
  def ragged(cls, pb: Problem, lengths, y, mask, X, params, series_ids=None,
             season_change=None) -> "Session":
    """ci_session_create_ragged: B trend series with their own lengths in one launch.  pb.T is the
    row stride (= max(lengths)) of y, mask [B, T] and X [B, T, P]; rows beyond a series' length are
    padding (never read).  series_ids [B]: the series ids the random streams are keyed by (default
    pb.series_offset + b).  fetch() returns [.., T] arrays that are 0 beyond each length.
    With `season_change` [1, T]: ci_session_create_ragged_seasonal -- trend plus one block of 2-7
    seasons; pb.T is then max(lengths) rounded up to a multiple of 4."""
    self = cls.__new__(cls)
    self._lib = load()
    self.pb = pb
    self.lengths = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
    if self.lengths.size != pb.num_series:
      raise ValueError(f"`lengths` must have one entry per series ({pb.num_series}), got {self.lengths.size}")
    ids = None
    if series_ids is not None:
      ids = np.ascontiguousarray(series_ids, dtype=np.int32).reshape(-1)
      if ids.size != pb.num_series:
        raise ValueError(f"`series_ids` must have one entry per series ({pb.num_series}), got {ids.size}")
    self._h = C.c_void_p()
    y32, mask8, X32, _ = _stage_inputs(pb, y, mask, X, None)
    if season_change is not None:
      sc = np.ascontiguousarray(np.asarray(season_change, dtype=np.uint8).reshape(-1, pb.T))
      _check(self._lib.ci_session_create_ragged_seasonal(C.byref(pb), _ptr(self.lengths), _ptr(ids),
                                                         _ptr(y32), _ptr(mask8), _ptr(X32), _ptr(sc),
                                                         params, C.byref(self._h)))
      return self
    _check(self._lib.ci_session_create_ragged(C.byref(pb), _ptr(self.lengths), _ptr(ids), _ptr(y32),
                                              _ptr(mask8), _ptr(X32), params, C.byref(self._h)))
    return self

  def run(self) -> float:
    """Runs all W+S iterations; returns the Gibbs kernel's duration in ms (HIP events)."""
    ms = C.c_float(0)
    _check(self._lib.ci_session_run(self._h, C.byref(ms)))
    return float(ms.value)

  def fetch(self, want=None) -> Dict[str, np.ndarray]:
    out, arrs = _alloc_outputs(self.pb, want)
    _check(self._lib.ci_session_fetch(self._h, C.byref(out)))
    return arrs

  def run_streamed(self, want=None, chunk_draws: int = 125, pinned: bool = True, into=None):
    """Runs the fit and copies the results to the host WHILE it runs (ci_session_run_streamed).
    Returns (kernel_ms, arrays); the arrays live in pinned memory unless pinned=False.  `into`
    re-uses the (Outputs, arrays) pair of an earlier call instead of allocating."""
    out, arrs = into if into is not None else _alloc_outputs(self.pb, want, pinned=pinned)
    ms = C.c_float(0)
    _check(self._lib.ci_session_run_streamed(self._h, C.byref(out), int(chunk_draws), C.byref(ms)))
    self._last_streamed = (out, arrs)
    return float(ms.value), arrs

  def algorithmic_bytes(self) -> float:
    b = C.c_double(0)
    _check(self._lib.ci_session_algorithmic_bytes(self._h, C.byref(b)))
    return float(b.value)

  def kernel_name(self) -> str:
    buf = C.create_string_buffer(128)
    _check(self._lib.ci_session_kernel_name(self._h, buf, 128))
    return buf.value.decode()

  def profile(self, enable=True):
    """Enables per-phase cycle counters for the next run(); returns the previous run's."""
    cyc = np.zeros(32, np.int64)
    _check(self._lib.ci_session_profile(self._h, int(enable), cyc.ctypes.data))
    return cyc

  def set_link(self, link: int):
    """The outcome link of this session's summaries from now on (ci_session_set_link): LINK_IDENTITY
    (the default), LINK_LOG or LINK_LOG1P.  `summarize`, `summarize_windows`, `summarize_paths`,
    `pool_trajectories`, `pool_event_trajectories` and `value_mean` then form value = link(trajectory
    * scale + shift) (`link_values_host`) draw by draw and keep their definitions on top of it;
    `summarize_components`, `summarize_predictions`, `summarize_placebo` and `pool_placebo` describe
    the model and ignore it."""
    _check(_symbol(self._lib, "ci_session_set_link")(self._h, int(link)))

  def value_mean(self, scale, shift) -> np.ndarray:
    """The mean over the N pooled draws of value[b, n, t] under the session's link
    (ci_session_value_mean), [B, T] float64 with the series axis kept; scale, shift: scalars or [B].
    Under a link the sampler's `posterior_means` mapped through (scale, shift) is not this mean."""
    fn = _symbol(self._lib, "ci_session_value_mean")
    B, T = self.pb.num_series, self.pb.T
    sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, np.float64), (B,)))
    sh = np.ascontiguousarray(np.broadcast_to(np.asarray(shift, np.float64), (B,)))
    out = np.empty((B, T), np.float64)
    _check(fn(self._h, sc.ctypes.data, sh.ctypes.data, out.ctypes.data))
    return out

  def summarize(self, scale, shift, observed, flags, ranks) -> Dict[str, np.ndarray]:
    """On-device order statistics / running effect sums of the pooled predictive draws of every
    series (ci_session_summarize).  scale, shift: scalars or [B]; observed, flags: [T] or [B,T].
    Returns value_order [B,R,T], cum_order [B,R,T], per_draw [B,2,N], per_draw_order [B,2,R]
    (leading axis dropped when the session holds one series)."""
    B, T, N = self.pb.num_series, self.pb.T, self.pb.num_chains * self.pb.num_results
    sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, np.float64), (B,)))
    sh = np.ascontiguousarray(np.broadcast_to(np.asarray(shift, np.float64), (B,)))
    obs = np.ascontiguousarray(np.broadcast_to(np.asarray(observed, np.float64), (B, T)))
    fl = np.ascontiguousarray(np.broadcast_to(np.asarray(flags, np.uint8), (B, T)))
    rk = np.ascontiguousarray(ranks, dtype=np.int32)
    # big batches: the result blocks in pinned host memory from the library's pool (512 series: 24 MB
    # -- pageable destinations cost the copies a staging pass and the arrays their first-touch faults)
    big = B * max(rk.size * T, 2 * N) * 8 > (1 << 20)
    empty = (lambda shp: pinned_empty(shp, np.float64)) if big else (lambda shp: np.empty(shp, np.float64))
    vo = empty((B, rk.size, T))
    co = empty((B, rk.size, T))
    pd_ = empty((B, 2, N))
    do = np.empty((B, 2, rk.size), np.float64)
    _check(self._lib.ci_session_summarize(self._h, sc.ctypes.data, sh.ctypes.data, obs.ctypes.data,
                                          fl.ctypes.data, int(rk.size), rk.ctypes.data,
                                          vo.ctypes.data, co.ctypes.data, pd_.ctypes.data,
                                          do.ctypes.data))
    if B == 1:
      vo, co, pd_, do = vo[0], co[0], pd_[0], do[0]
    return dict(value_order=vo, cum_order=co, per_draw=pd_, per_draw_order=do)

  def summarize_components(self, scale, shift, ranks, want=None) -> Dict[str, np.ndarray]:
    """On-device means and order statistics, over the pooled draws, of the trend, every seasonal
    block, the regression term and the regression weights of every series
    (ci_session_summarize_components).  scale, shift: scalars or [B], as for `summarize`; ranks: 1
    to 8 order statistics.  Returns float64 arrays that keep the series axis: trend_mean [B,T],
    trend_order [B,R,T]; with K seasonal blocks seasonal_mean [B,K,T], seasonal_order [B,K,R,T]; with
    P design columns regression_mean [B,T], regression_order [B,R,T], inclusion_prob [B,P],
    weight_mean [B,P], weight_order [B,R,P].  `want`: the names to compute (default: all that the
    model has); the others are skipped on the device too."""
    pb = self.pb
    B, T, P, K = pb.num_series, pb.T, pb.P, pb.num_blocks
    rk = np.ascontiguousarray(ranks, dtype=np.int32).reshape(-1)
    if not 1 <= rk.size <= MAX_SUMMARY_RANKS:
      raise ValueError(f"`ranks` must hold 1 to {MAX_SUMMARY_RANKS} order statistics, got {rk.size}")
    sc, sh = _per_series("scale", scale, B), _per_series("shift", shift, B)
    R = rk.size
    shapes = dict(trend_mean=(B, T), trend_order=(B, R, T))
    if K > 0:
      shapes.update(seasonal_mean=(B, K, T), seasonal_order=(B, K, R, T))
    if P > 0:
      shapes.update(regression_mean=(B, T), regression_order=(B, R, T), inclusion_prob=(B, P),
                    weight_mean=(B, P), weight_order=(B, R, P))
    if want is not None:
      unknown = [k for k in want if k not in COMPONENT_OUTPUTS]
      if unknown:
        raise ValueError(f"unknown component outputs {unknown}: choose from {list(COMPONENT_OUTPUTS)}")
      shapes = {k: v for k, v in shapes.items() if k in want}
    arrs = {k: np.empty(v, np.float64) for k, v in shapes.items()}
    _check(self._lib.ci_session_summarize_components(
        self._h, sc.ctypes.data, sh.ctypes.data, int(R), rk.ctypes.data,
        *[_ptr(arrs.get(k)) for k in COMPONENT_OUTPUTS]))
    return arrs

  def summarize_predictions(self, scale, shift, ranks, want=None,
                            _entry="ci_session_summarize_predictions") -> Dict[str, np.ndarray]:
    """On-device one-step-ahead prediction errors of every fit (ci_session_summarize_predictions):
    for every pooled draw the Kalman filter of that draw's model over the observed series, in
    float64 (`causalimpact_lib._prediction_summary_host` is the same definition in numpy).  scale,
    shift: scalars or [B], as for `summarize`; ranks: 1 to 8 order statistics.  Returns float64 arrays
    that keep the series axis: forecast_mean [B,T], forecast_order [B,R,T], variance_mean [B,T],
    pit_mean [B,T] (0 at the masked steps), loglik [B,N].  `want`: the names to compute (default:
    all); the others are skipped on the device too."""
    fn = _symbol(self._lib, _entry)
    pb = self.pb
    B, T, N = pb.num_series, pb.T, pb.num_chains * pb.num_results
    rk = np.ascontiguousarray(ranks, dtype=np.int32).reshape(-1)
    sc, sh = _per_series("scale", scale, B), _per_series("shift", shift, B)
    shapes = dict(forecast_mean=(B, T), forecast_order=(B, rk.size, T), variance_mean=(B, T),
                  pit_mean=(B, T), loglik=(B, N))
    if want is not None:
      unknown = [k for k in want if k not in PREDICTION_OUTPUTS]
      if unknown:
        raise ValueError(f"unknown prediction outputs {unknown}: choose from {list(PREDICTION_OUTPUTS)}")
      shapes = {k: v for k, v in shapes.items() if k in want}
    arrs = {k: np.empty(v, np.float64) for k, v in shapes.items()}
    _check(fn(self._h, sc.ctypes.data, sh.ctypes.data, int(rk.size), rk.ctypes.data,
              *[_ptr(arrs.get(k)) for k in PREDICTION_OUTPUTS]))
    return arrs

  def summarize_predictions_blocks(self, scale, shift, ranks, want=None) -> Dict[str, np.ndarray]:
    """`summarize_predictions` for any block list whose state has at most 64 components
    (ci_session_summarize_predictions_blocks: a group of lanes per filter): same arguments, same
    outputs, same `want`.  Ragged sessions stay with `summarize_predictions`."""
    return self.summarize_predictions(scale, shift, ranks, want,
                                      _entry="ci_session_summarize_predictions_blocks")

  def summarize_placebo(self, scale, shift, origins, horizon, want=None,
                        _entry="ci_session_summarize_placebo") -> Dict[str, np.ndarray]:
    """On-device placebo forecasts of every fit (ci_session_summarize_placebo): for every pooled draw
    the filter of `summarize_predictions` up to each origin, then the forecast of the sum of the next
    `horizon` observations without any update, in float64 (`causalimpact_lib._placebo_summary_host`
    is the same definition in numpy).  scale, shift: scalars or [B], as for `summarize`; origins
    [B, O] (or [O] for one series) int: steps, strictly ascending, -1 = unused, at the end of the
    row; horizon: scalar or [B].  Returns float64 arrays [B, O]: predicted_mean, spread_mean,
    pit_mean (0 in the unused slots and where the window counts no observation).  `want`: the names
    to compute (default: all); the others are skipped on the device too."""
    fn = _symbol(self._lib, _entry)
    B = self.pb.num_series
    org, hz = _origin_plan(origins, horizon, B)
    sc, sh = _per_series("scale", scale, B), _per_series("shift", shift, B)
    names = PLACEBO_OUTPUTS
    if want is not None:
      unknown = [k for k in want if k not in PLACEBO_OUTPUTS]
      if unknown:
        raise ValueError(f"unknown placebo outputs {unknown}: choose from {list(PLACEBO_OUTPUTS)}")
      names = [k for k in PLACEBO_OUTPUTS if k in want]
    arrs = {k: np.empty(org.shape, np.float64) for k in names}
    _check(fn(self._h, sc.ctypes.data, sh.ctypes.data, int(org.shape[1]), org.ctypes.data,
              hz.ctypes.data, *[_ptr(arrs.get(k)) for k in PLACEBO_OUTPUTS]))
    return arrs

  def summarize_placebo_blocks(self, scale, shift, origins, horizon, want=None) -> Dict[str, np.ndarray]:
    """`summarize_placebo` for any block list whose state has at most 64 components
    (ci_session_summarize_placebo_blocks): same arguments, same outputs, same `want`.  Ragged
    sessions stay with `summarize_placebo`."""
    return self.summarize_placebo(scale, shift, origins, horizon, want,
                                  _entry="ci_session_summarize_placebo_blocks")

  def summarize_placebo_horizons(self, scale, shift, origins, horizons, want=None,
                                 max_rows=None) -> Dict[str, np.ndarray]:
    """`summarize_placebo` at SEVERAL horizons from one filter pass
    (ci_session_summarize_placebo_horizons): result[name][:, :, k] is, bit for bit, what
    `summarize_placebo(scale, shift, origins, horizons[:, k])` returns -- every horizon looks from the
    same origins.  scale, shift, origins: as there, with origin + the row's largest horizon within the
    series; horizons [B, K] (or [K]: the same for every series) int, K <= 64: >= 1, strictly ascending,
    -1 = unused, at the end of the row (`horizon_table`).  Returns float64 arrays [B, O, K] under the
    names of `PLACEBO_OUTPUTS` (0 in the unused slots and where the window counts no observation);
    `want`: the names to compute (default: all).  Models: a trend with at most one block of 2 to 7
    seasons (for the others call `summarize_placebo_blocks` once per horizon).  max_rows (tests): the
    rows of a chunk in place of the call's own capacity (ci_test_session_summarize_placebo_horizons);
    the result then has "num_chunks" too."""
    fn = _symbol(self._lib, "ci_session_summarize_placebo_horizons" if max_rows is None
                 else "ci_test_session_summarize_placebo_horizons")
    B = self.pb.num_series
    org = np.asarray(origins)
    if org.ndim == 1 and B == 1:
      org = org[None]
    if org.ndim != 2 or org.shape[0] != B:
      raise ValueError(f"`origins` must be [{B}, O], got shape {org.shape}")
    org = np.ascontiguousarray(org, dtype=np.int32)
    hz = horizon_table(horizons, B)
    sc, sh = _per_series("scale", scale, B), _per_series("shift", shift, B)
    names = PLACEBO_OUTPUTS
    if want is not None:
      unknown = [k for k in want if k not in PLACEBO_OUTPUTS]
      if unknown:
        raise ValueError(f"unknown placebo outputs {unknown}: choose from {list(PLACEBO_OUTPUTS)}")
      names = [k for k in PLACEBO_OUTPUTS if k in want]
    arrs = {k: np.empty(org.shape + (hz.shape[1],), np.float64) for k in names}
    chunks = C.c_int32(0)
    _check(fn(self._h, sc.ctypes.data, sh.ctypes.data, int(org.shape[1]), org.ctypes.data, int(hz.shape[1]),
              hz.ctypes.data, *[_ptr(arrs.get(k)) for k in PLACEBO_OUTPUTS],
              *((int(max_rows), C.addressof(chunks)) if max_rows is not None else ())))
    if max_rows is not None:
      arrs["num_chunks"] = chunks.value
    return arrs

  def simulate_placebo(self, scale, shift, origins, horizon, link, seen, ranks, want=None,
                       blocks: bool = False, max_rows=None) -> Dict[str, np.ndarray]:
    """On-device SIMULATED placebo forecasts of every fit (ci_session_simulate_placebo): for every
    pooled draw the filter of `summarize_placebo` up to each origin, then ONE simulated path of the
    window -- the filter's own step fed with a draw from its own forecast -- linked step by step and
    summed (`causalimpact_lib._placebo_simulated_host` is the same definition in numpy).  scale,
    shift, origins, horizon: as for `summarize_placebo`; link: a `LINK_*`, passed explicitly (the
    session's `set_link` is neither read nor changed); seen [B, O]: the observed totals on the data
    scale (None: neither spread_mean nor below can be asked for); ranks: 1 to 8 order statistics.
    Returns float64 arrays: predicted_mean, spread_mean, below [B, O], total_order [B, R, O], totals
    [B, O, N] (0 in the unused slots and where the window counts no observation).  `want`: the names
    to compute (default: all but `totals`, and without `seen` those that need none).  max_rows
    (tests): the rows of a chunk in place of the scratch's (ci_test_session_simulate_placebo); the
    result then has "num_chunks" too."""
    if max_rows is not None:
      name = "ci_test_session_simulate_placebo"
    else:
      name = "ci_session_simulate_placebo_blocks" if blocks else "ci_session_simulate_placebo"
    fn = _symbol(self._lib, name)
    pb = self.pb
    B, N = pb.num_series, pb.num_chains * pb.num_results
    org, hz = _origin_plan(origins, horizon, B)
    O = int(org.shape[1])
    sc, sh = _per_series("scale", scale, B), _per_series("shift", shift, B)
    rk = np.ascontiguousarray(ranks, dtype=np.int32).reshape(-1)
    if seen is not None:
      seen = np.asarray(seen, np.float64)
      if seen.ndim == 1 and B == 1:
        seen = seen[None]
      if seen.shape != org.shape:
        raise ValueError(f"`seen` must be {list(org.shape)}, got {list(seen.shape)}")
      seen = np.ascontiguousarray(seen)
    shapes = dict(predicted_mean=(B, O), spread_mean=(B, O), below=(B, O), total_order=(B, rk.size, O),
                  totals=(B, O, N))
    if want is None:
      want = [k for k in PLACEBO_SIM_OUTPUTS
              if k != "totals" and (seen is not None or k not in ("spread_mean", "below"))]
    unknown = [k for k in want if k not in PLACEBO_SIM_OUTPUTS]
    if unknown:
      raise ValueError(f"unknown simulated placebo outputs {unknown}: choose from {list(PLACEBO_SIM_OUTPUTS)}")
    arrs = {k: np.empty(shapes[k], np.float64) for k in PLACEBO_SIM_OUTPUTS if k in want}
    chunks = C.c_int32(0)
    _check(fn(self._h, *((int(bool(blocks)),) if max_rows is not None else ()),
              sc.ctypes.data, sh.ctypes.data, O, org.ctypes.data, hz.ctypes.data, int(link), _ptr(seen),
              int(rk.size), rk.ctypes.data, *[_ptr(arrs.get(k)) for k in PLACEBO_SIM_OUTPUTS],
              *((int(max_rows), C.addressof(chunks)) if max_rows is not None else ())))
    if max_rows is not None:
      arrs["num_chunks"] = chunks.value
    return arrs

  def simulate_placebo_blocks(self, scale, shift, origins, horizon, link, seen, ranks, want=None,
                              max_rows=None) -> Dict[str, np.ndarray]:
    """`simulate_placebo` for any block list whose state has at most 64 components
    (ci_session_simulate_placebo_blocks): same arguments, same outputs.  Ragged sessions stay with
    `simulate_placebo`."""
    return self.simulate_placebo(scale, shift, origins, horizon, link, seen, ranks, want, blocks=True,
                                 max_rows=max_rows)

  def summarize_windows(self, scale, shift, observed, first, count, ranks,
                        want_draws=True) -> Dict[str, np.ndarray]:
    """On-device per-draw totals over sub-windows of the steps, and their order statistics
    (ci_session_summarize_windows): one streaming pass over the windows' own columns of the resident
    float32 trajectories.  scale, shift: scalars or [B]; observed: [T] or [B, T]; first, count: [W]
    (the same windows for every series) or [B, W], in steps of the session; ranks: 1 to 8 order
    statistics.  Returns per_draw [B, W, 2, N] (the window's sum of the predicted values, and of the
    point effects with the unobserved steps skipped; left out unless want_draws) and per_draw_order
    [B, W, 2, R]; the series axis is kept.  `window_totals_host` is the same loop on the host; a
    window equal to the post-period gives `summarize`'s per_draw and per_draw_order bit for bit."""
    fn = _symbol(self._lib, "ci_session_summarize_windows")
    pb = self.pb
    return _windows_call(fn, self._h, pb.num_series, pb.num_chains * pb.num_results, pb.T, scale, shift,
                         observed, first, count, ranks, want_draws)

  def summarize_paths(self, scale, shift, observed, first, count, ranks, want=PATH_OUTPUTS,
                      max_bytes=None) -> Dict[str, np.ndarray]:
    """On-device moments of the prediction's and the cumulative effect's paths over sub-windows of
    the steps, and every draw's largest standardised excursion from them (ci_session_summarize_paths;
    kernels: csrc/ci_paths.h): what a simultaneous band and a whole-path test are made of.  Arguments
    as for `summarize_windows`; want: the `PATH_OUTPUTS` to return -- center, spread [B, W, 2, T],
    excursion [B, W, 2, N], excursion_order [B, W, 2, R], observed_excursion [B, W, 2], at, exceed
    [B, W, 2] int32; the series axis is kept.  `path_excursions_host` is the same in numpy.
    max_bytes (tests): the limit of the call's device memory in place of the library's
    (ci_test_session_summarize_paths); the result then has "num_chunks" too."""
    name = "ci_session_summarize_paths" if max_bytes is None else "ci_test_session_summarize_paths"
    fn = _symbol(self._lib, name)
    pb, chunks = self.pb, C.c_int32(0)
    out = _paths_call(fn, self._h, pb.num_series, pb.num_chains * pb.num_results, pb.T, scale, shift,
                      observed, first, count, ranks, want,
                      () if max_bytes is None else (int(max_bytes), C.addressof(chunks)))
    if max_bytes is not None:
      out["num_chunks"] = chunks.value
    return out

  def pool_trajectories(self, scale, shift, groups, init=None) -> np.ndarray:
    """Weighted sums over groups of series of the resident predictive trajectories, draw by draw
    (ci_session_pool_trajectories): out[g] = init[g] + sum over the members b of group g, ascending,
    of w[g, b] * (trajectory[b] * scale[b] + shift[b]), float64, one rounding per operation
    (`pool_host` is the same loop in numpy).  scale, shift: scalars or [B]; groups: one entry per
    group, a mapping {position in the session: weight} or a sequence of positions (`groups_csr`);
    init: [G, N, T] float64 -- the result of the part of a batch in front of this session -- or
    None.  Returns [G, N, T] float64, N = chains x draws (chain-major)."""
    pb = self.pb
    return _pool_call(self._lib.ci_session_pool_trajectories, self._h, pb.num_series,
                      pb.num_chains * pb.num_results, pb.T, scale, shift, groups, init)

  def pool_event_trajectories(self, scale, shift, groups, init=None, out_stride=None) -> np.ndarray:
    """`pool_trajectories` over windows of the members' trajectories, every member from a step of its
    own (ci_session_pool_event_trajectories): the draws of a pooled effect in event time.  groups:
    one (members, width) pair per group, members a mapping {position in the session: (weight,
    first)} (`event_groups_csr`).  out[g, n, c] = init[g, n, c] + the sum over the members b of group
    g, ascending, of weight * (trajectory[b, n, first + c] * scale[b] + shift[b]) for c < width,
    float64, one rounding per operation (`pool_event_host` is the same loop in numpy); the columns
    from a group's width to out_stride (default: the widest group) are 0.0.  init: [G, N, out_stride]
    float64 or None.  Returns [G, N, out_stride] float64."""
    fn = _symbol(self._lib, "ci_session_pool_event_trajectories")
    pb = self.pb
    return _pool_call(fn, self._h, pb.num_series, pb.num_chains * pb.num_results, pb.T, scale, shift,
                      groups, init, True, out_stride)

  def _pool_placebo_tables(self, scale, shift, groups, origins, horizon):
    """(scale [B], shift [B], offsets, members, weights, origins [K, O] int32, horizon [G] int32): the
    arguments of `pool_placebo` and `pool_simulated_placebo` as the C entries take them."""
    B = self.pb.num_series
    sc, sh = _per_series("scale", scale, B), _per_series("shift", shift, B)
    offsets, members, weights = _entry_csr(groups, B)
    G = offsets.size - 1
    if isinstance(origins, np.ndarray) or not (len(origins) and hasattr(origins[0], "items")):
      per_series = np.asarray(origins)
      if per_series.ndim != 2 or per_series.shape[0] != B:
        raise ValueError(f"`origins` must be [{B}, O] or one mapping per group, got shape {per_series.shape}")
      org = per_series[members] if members.size else per_series[:0]
    else:
      if len(origins) != G:
        raise ValueError(f"`origins` must have one mapping per group ({G}), got {len(origins)}")
      rows = [np.asarray(origins[g][int(b)]).reshape(-1) for g in range(G) for b in members[offsets[g]:offsets[g + 1]]]
      width = max([r.size for r in rows] + [np.asarray(v).size for m in origins for v in m.values()] + [1])
      org = np.full((len(rows), width), -1, np.int64)
      for k, r in enumerate(rows):
        org[k, :r.size] = r
    org = np.ascontiguousarray(org, dtype=np.int32)
    O = int(org.shape[1])
    if members.size == 0:                  # (no entry at all: the tables still want an address)
      members, weights, org = np.zeros(1, np.int32), np.zeros(1), np.full((1, O), -1, np.int32)
    hz = np.asarray(horizon)
    if hz.shape not in ((), (G,)):
      raise ValueError(f"`horizon` must be a scalar or have one entry per group ({G}), got shape {hz.shape}")
    hz = np.ascontiguousarray(np.broadcast_to(hz, (G,)), dtype=np.int32)
    return sc, sh, offsets, members, weights, org, hz

  def pool_placebo(self, scale, shift, groups, origins, horizon, init=None, seen=None, *,
                   _entry="ci_session_pool_placebo", _tail=()) -> Dict[str, np.ndarray]:
    """Placebo forecasts of POOLED sums (ci_session_pool_placebo): `summarize_placebo`'s forecasts of
    the members of every group, added draw by draw with the group's weights, and the members'
    predictive variances added with the squared weights -- float64, entries ascending, one rounding
    per operation (`pool_placebo_host` is the same loop in numpy).  scale, shift: scalars or [B];
    groups: as for `pool_trajectories` (`groups_csr`: members of zero weight are left out);
    origins: [B, O] int -- every entry takes the row of its series -- or one mapping {position in the
    session: row [O]} per group, every row strictly ascending steps with -1 (unused) at the end;
    horizon: a scalar or [G], ONE horizon per group; init: [G, O, 2, N] float64 -- the `acc` of the
    part of a batch in front of this session -- or None; seen: [G, O] the pooled observed sums on the
    data scale, or None.  Returns acc [G, O, 2, N] (S, then U) and, with `seen`, predicted_mean,
    spread_mean, pit_mean [G, O] (`finish_placebo_host`).  Given every member's draw the pooled sum
    is N(S, U) IF the members are independent of each other: the assumption this check tests."""
    fn = _symbol(self._lib, _entry)
    sc, sh, offsets, members, weights, org, hz = self._pool_placebo_tables(scale, shift, groups, origins, horizon)
    G, O, N = offsets.size - 1, int(org.shape[1]), self.pb.num_chains * self.pb.num_results
    if init is not None:
      init = np.ascontiguousarray(init, dtype=np.float64)
      if init.shape != (G, O, 2, N):
        raise ValueError(f"`init` must be {[G, O, 2, N]}, got {list(init.shape)}")
    out = {"acc": np.empty((G, O, 2, N), np.float64)}
    if seen is not None:
      seen = np.ascontiguousarray(seen, dtype=np.float64)
      if seen.shape != (G, O):
        raise ValueError(f"`seen` must be {[G, O]}, got {list(seen.shape)}")
      out.update({k: np.empty((G, O), np.float64) for k in PLACEBO_OUTPUTS})
    _check(fn(self._h, sc.ctypes.data, sh.ctypes.data, G, offsets.ctypes.data, members.ctypes.data,
              weights.ctypes.data, O, org.ctypes.data, hz.ctypes.data, _ptr(init), out["acc"].ctypes.data,
              _ptr(seen), *[_ptr(out.get(k)) for k in PLACEBO_OUTPUTS], *_tail))
    return out

  def pool_placebo_blocks(self, scale, shift, groups, origins, horizon, init=None, seen=None,
                          chunk_entries=None) -> Dict[str, np.ndarray]:
    """`pool_placebo` for any block list whose state has at most 64 components
    (ci_session_pool_placebo_blocks): same arguments, same outputs; the filter of
    `summarize_placebo_blocks` runs once per chunk of entries for both pooled terms.  Ragged sessions
    stay with `pool_placebo`.  chunk_entries (tests): the entries of a chunk, in [1, B], in place of B
    (ci_test_session_pool_placebo_blocks); the result does not depend on it."""
    if chunk_entries is None:
      return self.pool_placebo(scale, shift, groups, origins, horizon, init, seen,
                               _entry="ci_session_pool_placebo_blocks")
    return self.pool_placebo(scale, shift, groups, origins, horizon, init, seen,
                             _entry="ci_test_session_pool_placebo_blocks", _tail=(int(chunk_entries),))

  def pool_placebo_horizons(self, scale, shift, groups, origins, horizons, init=None, seen=None, *,
                            blocks: bool = False, chunk_entries=None) -> Dict[str, np.ndarray]:
    """`pool_placebo` at SEVERAL HORIZONS per group from one filter pass
    (ci_session_pool_placebo_horizons; blocks=True: .._blocks, the sessions and models of
    `pool_placebo_blocks`): every x[g, i, k] of the result is, bit for bit, what `pool_placebo`
    (`pool_placebo_blocks`) returns at [g, i] with horizon[g] = horizons[g, k], init[:, :, k] and
    seen[:, :, k].  scale, shift, groups, origins: as for `pool_placebo`, the origins checked with the
    group's largest horizon; horizons: [G, K] int or -- the same row for every group -- [K], every row
    strictly ascending, >= 1, -1 = unused, at the end of the row (`horizon_table`, checked here before
    the library is reached); init: [G, O, K, 2, N] or None; seen: [G, O, K] or None.  Returns acc
    [G, O, K, 2, N] (S, then U) and, with `seen`, predicted_mean, spread_mean, pit_mean [G, O, K]; an
    unused horizon slot adds nothing to acc and reads 0 in the means.  chunk_entries (tests): the
    entries of a chunk (ci_test_session_pool_placebo_horizons); the result does not depend on it and
    `num_chunks` is returned besides."""
    name = ("ci_test_session_pool_placebo_horizons" if chunk_entries is not None
            else "ci_session_pool_placebo_horizons" + ("_blocks" if blocks else ""))
    sc, sh, offsets, members, weights, org, _ = self._pool_placebo_tables(scale, shift, groups, origins, 1)
    G, O, N = offsets.size - 1, int(org.shape[1]), self.pb.num_chains * self.pb.num_results
    hz = horizon_table(horizons, G, owner="group")
    K = int(hz.shape[1])
    if init is not None:
      init = np.ascontiguousarray(init, dtype=np.float64)
      if init.shape != (G, O, K, 2, N):
        raise ValueError(f"`init` must be {[G, O, K, 2, N]}, got {list(init.shape)}")
    out = {"acc": np.empty((G, O, K, 2, N), np.float64)}
    if seen is not None:
      seen = np.ascontiguousarray(seen, dtype=np.float64)
      if seen.shape != (G, O, K):
        raise ValueError(f"`seen` must be {[G, O, K]}, got {list(seen.shape)}")
      out.update({k: np.empty((G, O, K), np.float64) for k in PLACEBO_OUTPUTS})
    fn = _symbol(self._lib, name)
    chunks = C.c_int32(0)
    head = (self._h,) + ((int(bool(blocks)),) if chunk_entries is not None else ())
    tail = (int(chunk_entries), C.addressof(chunks)) if chunk_entries is not None else ()
    _check(fn(*head, sc.ctypes.data, sh.ctypes.data, G, offsets.ctypes.data, members.ctypes.data,
              weights.ctypes.data, O, org.ctypes.data, K, hz.ctypes.data, _ptr(init), out["acc"].ctypes.data,
              _ptr(seen), *[_ptr(out.get(k)) for k in PLACEBO_OUTPUTS], *tail))
    if chunk_entries is not None:
      out["num_chunks"] = int(chunks.value)
    return out

  def pool_simulated_placebo(self, scale, shift, groups, origins, horizon, link, init=None, seen=None,
                             counted=None, ranks=None, want=None, *, blocks: bool = False,
                             chunk_entries=None) -> Dict[str, np.ndarray]:
    """SIMULATED placebo forecasts of POOLED sums (ci_session_pool_simulated_placebo): the totals of
    `simulate_placebo` of the members of every group -- the same filter, link and random stream, every
    entry from its own origin row with the group's horizon -- added draw by draw with the group's
    weights, float64, entries ascending, one rounding per operation (`pool_simulated_placebo_host` is
    the same loop in numpy).  scale, shift, groups, origins, horizon: as for `pool_placebo`; link: a
    `LINK_*`, passed explicitly; init: [G, O, N] float64 -- the `acc` of the part of a batch in front
    of this session -- or None; seen [G, O]: the pooled observed totals on the data scale, counted
    [G, O]: the member-steps every window counts -- both or neither; ranks: 1 to 8 order statistics
    (default with `seen`: none asked for).  Returns acc [G, O, N] and, with `seen` and `counted`, the
    statistics of `simulate_placebo` over the rows of acc (`finish_simulated_placebo_host`):
    predicted_mean, spread_mean, below [G, O] and, with `ranks`, total_order [G, R, O]; `want` names
    those to compute.  The members' paths are independent of each other (every series has its own
    Philox key): the assumption this check tests.  chunk_entries (tests): the entries of a chunk, in
    [1, B], in place of B (ci_test_session_pool_simulated_placebo); the result does not depend on it."""
    if chunk_entries is not None:
      name = "ci_test_session_pool_simulated_placebo"
    else:
      name = "ci_session_pool_simulated_placebo_blocks" if blocks else "ci_session_pool_simulated_placebo"
    fn = _symbol(self._lib, name)
    sc, sh, offsets, members, weights, org, hz = self._pool_placebo_tables(scale, shift, groups, origins, horizon)
    G, O, N = offsets.size - 1, int(org.shape[1]), self.pb.num_chains * self.pb.num_results
    if init is not None:
      init = np.ascontiguousarray(init, dtype=np.float64)
      if init.shape != (G, O, N):
        raise ValueError(f"`init` must be {[G, O, N]}, got {list(init.shape)}")
    if (seen is None) != (counted is None):
      raise ValueError("`seen` and `counted` go together: the statistics need both")
    rk = np.ascontiguousarray([0] if ranks is None else ranks, dtype=np.int32).reshape(-1)
    shapes = dict(predicted_mean=(G, O), spread_mean=(G, O), below=(G, O), total_order=(G, rk.size, O))
    if want is None:
      want = [] if seen is None else [k for k in shapes if k != "total_order" or ranks is not None]
    unknown = [k for k in want if k not in shapes]
    if unknown:
      raise ValueError(f"unknown pooled simulated placebo outputs {unknown}: choose from {list(shapes)}")
    if seen is not None:
      seen = np.ascontiguousarray(seen, dtype=np.float64)
      counted = np.ascontiguousarray(counted, dtype=np.int32)
      for what, a in (("seen", seen), ("counted", counted)):
        if a.shape != (G, O):
          raise ValueError(f"`{what}` must be {[G, O]}, got {list(a.shape)}")
    out = {"acc": np.empty((G, O, N), np.float64)}
    out.update({k: np.empty(shapes[k], np.float64) for k in shapes if k in want})
    _check(fn(self._h, *((int(bool(blocks)),) if chunk_entries is not None else ()),
              sc.ctypes.data, sh.ctypes.data, G, offsets.ctypes.data, members.ctypes.data, weights.ctypes.data,
              O, org.ctypes.data, hz.ctypes.data, int(link), _ptr(init), out["acc"].ctypes.data, _ptr(seen),
              _ptr(counted), int(rk.size), rk.ctypes.data, *[_ptr(out.get(k)) for k in shapes],
              *((int(chunk_entries),) if chunk_entries is not None else ())))
    return out

  def pool_simulated_placebo_blocks(self, scale, shift, groups, origins, horizon, link, init=None, seen=None,
                                    counted=None, ranks=None, want=None,
                                    chunk_entries=None) -> Dict[str, np.ndarray]:
    """`pool_simulated_placebo` for any block list whose state has at most 64 components
    (ci_session_pool_simulated_placebo_blocks): same arguments, same outputs, the filter of
    `simulate_placebo_blocks`.  Ragged sessions stay with `pool_simulated_placebo`."""
    return self.pool_simulated_placebo(scale, shift, groups, origins, horizon, link, init, seen, counted, ranks,
                                       want, blocks=True, chunk_entries=chunk_entries)

  def close(self):
    if self._h:
      self._lib.ci_session_destroy(self._h)
      self._h = C.c_void_p()

  def __del__(self):
    try:
      self.close()
    except Exception:  # pylint: disable=broad-except
      pass


DRAW_FIELDS = ("observation_noise_scale", "level_scale", "slope_scale", "seasonal_drift_scales", "weights")


class DrawsSession(Session):
  """A session made from draws (ci_session_create_from_draws[_f64]): the data and the pooled
  parameter draws of B fits, uploaded from the host, for the prediction-error and placebo entries
  alone -- `summarize_predictions`, `summarize_placebo`, `summarize_placebo_horizons`, `simulate_placebo`, `pool_placebo`,
  `pool_placebo_horizons`,
  `pool_simulated_placebo` and their `_blocks` forms, with the signatures and results they have on a
  fit's `Session`.  Every method that needs a fit (`run`, `fetch`, `summarize`, ..) raises NativeError.

  pb: the fit's problem record (geometry, chains, kept draws, seed, chain_offset, series_offset,
  flags, device); chains pooled from several devices are one session with chain_offset 0.  y, mask
  [B, T], X [B, T, P], season_change [K, T], params: as `Session` takes them.  draws: a dict with
  `DRAW_FIELDS` as `Session.fetch` returns them -- [B, C, S], seasonal_drift_scales [B, C, S, K],
  weights [B, C, S, P]; slope_scale, seasonal_drift_scales and weights may be missing where the model
  has no slope, block or design.  dtype float32: the filters of a fit's session on these values, bit
  for bit; float64: y, X and the draws are filtered as float64."""

  summaries = ("predictions", "placebo")

  def __init__(self, pb: Problem, y, mask, X, season_change, params, draws, dtype=np.float32):  # pylint: disable=super-init-not-called
    self._lib = load()
    self.pb = pb
    self._h = C.c_void_p()
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
      raise ValueError(f"`dtype` must be float32 or float64, got {dt}")
    self.dtype = dt
    B, T, P, K = pb.num_series, pb.T, pb.P, pb.num_blocks
    CS = (pb.num_chains, pb.num_results)
    shapes = dict(observation_noise_scale=(B,) + CS, level_scale=(B,) + CS, slope_scale=(B,) + CS,
                  seasonal_drift_scales=(B,) + CS + (K,), weights=(B,) + CS + (P,))
    needed = dict(observation_noise_scale=True, level_scale=True, slope_scale=bool(pb.has_slope),
                  seasonal_drift_scales=K > 0, weights=P > 0)
    arrs = []
    for k in DRAW_FIELDS:
      a = draws.get(k)
      if a is None or not needed[k]:
        if needed[k]:
          raise ValueError(f"`draws` lacks {k!r}, which this model reads")
        arrs.append(None)
        continue
      a = np.asarray(a)
      if a.shape != shapes[k]:
        raise ValueError(f"draws[{k!r}] must be {list(shapes[k])}, got {list(a.shape)}")
      arrs.append(np.ascontiguousarray(a, dtype=dt))
    mask8 = np.ascontiguousarray(np.asarray(mask, dtype=bool).reshape(B, T).astype(np.uint8))
    yd = np.ascontiguousarray(np.asarray(y, dtype=dt).reshape(B, T))
    Xd = np.ascontiguousarray(np.asarray(X, dtype=dt).reshape(B, T, P)) if P > 0 else None
    sc = None
    if K > 0 and season_change is not None:
      sc = np.ascontiguousarray(np.asarray(season_change, dtype=np.uint8).reshape(K, T))
    name = "ci_session_create_from_draws_f64" if dt == np.dtype(np.float64) else "ci_session_create_from_draws"
    _check(_symbol(self._lib, name)(C.byref(pb), _ptr(yd), _ptr(mask8), _ptr(Xd), _ptr(sc), params,
                                    *[_ptr(a) for a in arrs], C.byref(self._h)))


def kalman_loglik(pb: Problem, params, y, mask, X, theta) -> np.ndarray:
  """Log-likelihood l(theta_e) for every row theta_e = (sigma_obs, sigma_level, sigma_slope,
  weights...) of `theta` (row H of SURVEY.md section 8)."""
  L = load()
  T, P = pb.T, pb.P
  m8 = np.ascontiguousarray(np.asarray(mask, bool).astype(np.uint8))
  y32 = np.ascontiguousarray(np.where(m8 != 0, np.float32(0), np.asarray(y, np.float32)))
  X32 = np.ascontiguousarray(np.asarray(X, np.float32).reshape(T, P)) if P > 0 else None
  th = np.ascontiguousarray(np.asarray(theta, np.float64).reshape(-1, 3 + P))
  out = np.zeros(th.shape[0], np.float64)
  _check(L.ci_kalman_loglik(C.byref(pb), params, y32.ctypes.data, m8.ctypes.data, _ptr(X32),
                            th.shape[0], th.ctypes.data, out.ctypes.data))
  return out


def _hmc_options(*, num_chains, chain_offset, num_warmup, num_results, num_leapfrog, target_accept,
                 initial_step_size, seed, prior, horseshoe_scale) -> HmcOptions:
  o = HmcOptions()
  o.num_chains, o.chain_offset = int(num_chains), int(chain_offset)
  o.num_warmup, o.num_results, o.num_leapfrog = int(num_warmup), int(num_results), int(num_leapfrog)
  if prior not in HMC_PRIORS:
    raise ValueError(f"prior must be one of {sorted(HMC_PRIORS)}, got {prior!r}")
  o.prior = HMC_PRIORS[prior]
  o.target_accept, o.initial_step_size = float(target_accept), float(initial_step_size)
  o.horseshoe_scale = float(horseshoe_scale)
  o.seed[0], o.seed[1] = seed_pair(seed)
  return o


class LogLikSession:
  """Device-resident log-likelihood / score evaluator and latent-path drawer for one series."""

  B, batched = 1, False

  def __init__(self, pb: Problem, params, y, mask, X, max_evals: int, season_change=None):
    """season_change [K, T] uint8 for models with seasonal blocks (pb.num_blocks = K): those, and
    series longer than 4096 steps, run on the sequential route (csrc/ci_score_seq.h); parameter
    rows are then (sigma_obs, sigma_level, sigma_slope, sigma_drift[K], weights[P])."""
    self._lib = load()
    self.T, self.P, self.D, self.K = pb.T, pb.P, 2 if pb.has_slope else 1, pb.num_blocks
    self.num_seasons = [int(pb.num_seasons[k]) for k in range(pb.num_blocks)]
    self.max_evals = int(max_evals)
    m8 = np.ascontiguousarray(np.asarray(mask, bool).astype(np.uint8))
    y32 = np.ascontiguousarray(np.where(m8 != 0, np.float32(0), np.asarray(y, np.float32)))
    X32 = (np.ascontiguousarray(np.asarray(X, np.float32).reshape(self.T, self.P))
           if self.P > 0 else None)
    sc = None
    if self.K > 0:
      sc = np.ascontiguousarray(np.asarray(season_change, dtype=np.uint8).reshape(self.K, self.T))
    self._h = C.c_void_p()
    _check(self._lib.ci_ll_session_create2(C.byref(pb), params, y32.ctypes.data, m8.ctypes.data,
                                           _ptr(X32), _ptr(sc), self.max_evals, C.byref(self._h)))

  def evaluate(self, theta, want_grad=True):
    th = np.ascontiguousarray(np.asarray(theta, np.float64).reshape(-1, 3 + self.K + self.P))
    ll = np.zeros(th.shape[0], np.float64)
    grad = np.zeros_like(th) if want_grad else None
    _check(self._lib.ci_ll_session_eval(self._h, th.shape[0], th.ctypes.data, ll.ctypes.data,
                                        _ptr(grad)))
    return ll, grad

  def draw_latents(self, theta, seed, rng_chain=0, iter0=0):
    th = np.ascontiguousarray(np.asarray(theta, np.float64).reshape(-1, 3 + self.P))
    E = th.shape[0]
    out = {k: np.zeros((E, self.T), np.float32) for k in ("level", "slope", "loc", "traj")}
    s = (C.c_uint32 * 2)(*seed_pair(seed))
    _check(self._lib.ci_ll_session_draw_latents(
        self._h, E, th.ctypes.data, s, int(rng_chain), int(iter0), out["level"].ctypes.data,
        out["slope"].ctypes.data, out["loc"].ctypes.data, out["traj"].ctypes.data))
    return out

  def hmc_run(self, *, num_chains, num_warmup, num_results, num_leapfrog=15, target_accept=0.75,
              initial_step_size=0.05, seed=(0, 0), chain_offset=0, init_theta=None, prior="slab",
              horseshoe_scale=0.1):
    """The whole HMC fit on the device (ci_ll_session_hmc_run): chain, latent paths and
    predictive trajectories stay in HBM.  Returns (hmc_kernel_ms, latents_ms)."""
    o = _hmc_options(num_chains=num_chains, chain_offset=chain_offset, num_warmup=num_warmup,
                     num_results=num_results, num_leapfrog=num_leapfrog, target_accept=target_accept,
                     initial_step_size=initial_step_size, seed=seed, prior=prior,
                     horseshoe_scale=horseshoe_scale)
    init = None if init_theta is None else np.ascontiguousarray(init_theta, dtype=np.float64)
    if init is not None:
      dim = (3 * self.P + 2 if prior == "horseshoe" else self.P) + self.D + 1 + self.K
      want = (self.B, int(num_chains), dim) if self.batched else (int(num_chains), dim)
      if init.shape != want:
        raise ValueError(f"init_theta must be {list(want)}, got {list(init.shape)}")
    ms = (C.c_float * 2)()
    _check(self._lib.ci_ll_session_hmc_run(self._h, C.byref(o), _ptr(init), ms))
    self._hmc_shape = (int(num_chains), int(num_results))
    return float(ms[0]), float(ms[1])

  def hmc_fetch(self, want=None):
    """Host copies of the finished fit: draws [C, S, 3+K+P] float64 (sigma_obs, sigma_level,
    sigma_slope, sigma_drift[K], weights), accept_rate, step_size [C] and the float32 sample
    container of `fit_gibbs` (leading series axis of 1)."""
    Cn, S = self._hmc_shape
    pb = make_problem(T=self.T, P=self.P, has_slope=self.D == 2, num_seasons=self.num_seasons,
                      num_warmup=0, num_results=S, num_chains=Cn)
    if want is None:
      want = [f for f in _OUT_FIELDS
              if self.K > 0 or f not in ("seasonal_drift_scales", "seasonal_levels")]
    out, arrs = _alloc_outputs(pb, want)
    draws = np.zeros((Cn, S, 3 + self.K + self.P), np.float64)
    acc = np.zeros(Cn, np.float64)
    eps = np.zeros(Cn, np.float64)
    _check(self._lib.ci_ll_session_hmc_fetch(self._h, draws.ctypes.data, acc.ctypes.data,
                                             eps.ctypes.data, C.byref(out)))
    return draws, acc, eps, arrs

  def hmc(self, **kw):
    """hmc_run + the parameter draws only: draws [C, S, 3+P], accept_rate, step_size [C]."""
    self.hmc_run(**kw)
    Cn, S = self._hmc_shape
    draws = np.zeros((Cn, S, 3 + self.K + self.P), np.float64)
    acc = np.zeros(Cn, np.float64)
    eps = np.zeros(Cn, np.float64)
    _check(self._lib.ci_ll_session_hmc_fetch(self._h, draws.ctypes.data, acc.ctypes.data,
                                             eps.ctypes.data, None))
    return draws, acc, eps

  def pool_trajectories(self, scale, shift, groups, init=None) -> np.ndarray:
    """`Session.pool_trajectories` of the fit's resident predictive trajectories
    (ci_ll_session_pool_trajectories): [G, N, T] float64, N = chains x draws of the last `hmc_run`."""
    Cn, S = self._hmc_shape
    return _pool_call(self._lib.ci_ll_session_pool_trajectories, self._h, self.B, Cn * S, self.T,
                      scale, shift, groups, init)

  def algorithmic_bytes(self) -> float:
    b = C.c_double(0)
    _check(self._lib.ci_ll_session_algorithmic_bytes(self._h, C.byref(b)))
    return float(b.value)

  def kernel_name(self) -> str:
    buf = C.create_string_buffer(128)
    _check(self._lib.ci_ll_session_kernel_name(self._h, buf, 128))
    return buf.value.decode()

  def close(self):
    if self._h:
      self._lib.ci_ll_session_destroy(self._h)
      self._h = C.c_void_p()

  def __del__(self):
    try:
      self.close()
    except Exception:  # pylint: disable=broad-except
      pass


class BatchLogLikSession(LogLikSession):
  """B series in one session (ci_ll_session_create_batch): one launch fits B x num_chains HMC chains.
  Trend models, T <= 4096, P <= 128.  pb.num_series = B, pb.series_offset and
  FLAG_SHARED_SERIES_STREAMS in pb.flags key the series' random streams as in `fit_gibbs`.
  Every result has a leading series axis: hmc_run's init_theta is [B, C, dim], hmc_fetch returns
  draws [B, C, S, 3 + P], accept_rate and step_size [B, C] and the `fit_gibbs` container with this B.
  `evaluate` and `draw_latents` need B = 1."""

  batched = True
  # the kinds of `causalimpact_lib.SummaryRecord` this session takes on the device (it keeps no
  # latent draws and has no filter entries)
  summaries = ("effect", "windows", "paths")

  def __init__(self, pb: Problem, params, y, mask, X, max_evals: int = 1):   # pylint: disable=super-init-not-called
    self._lib = load()
    self.problem = pb      # (seed, series_offset, flags, device: what keys the series' streams)
    self.B, self.T, self.P, self.D, self.K = pb.num_series, pb.T, pb.P, 2 if pb.has_slope else 1, 0
    self.num_seasons = []
    self.max_evals = int(max_evals)
    y32, mask8, X32, _ = _stage_inputs(pb, y, mask, X, None)
    self._h = C.c_void_p()
    _check(self._lib.ci_ll_session_create_batch(C.byref(pb), params, y32.ctypes.data, mask8.ctypes.data,
                                                _ptr(X32), self.max_evals, C.byref(self._h)))

  def hmc_fetch(self, want=None, with_draws=True):
    """Host copies of the finished fit: draws [B, C, S, 3 + P] float64 (None unless with_draws),
    accept_rate and step_size [B, C], and the float32 container of `fit_gibbs` for the fields in
    `want` (default: all the trend model has)."""
    Cn, S = self._hmc_shape
    pb = make_problem(T=self.T, P=self.P, has_slope=self.D == 2, num_warmup=0, num_results=S,
                      num_chains=Cn, num_series=self.B)
    if want is None:
      want = [f for f in _OUT_FIELDS if f not in ("seasonal_drift_scales", "seasonal_levels")]
    out, arrs = _alloc_outputs(pb, want)
    draws = np.zeros((self.B, Cn, S, 3 + self.P), np.float64) if with_draws else None
    acc = np.zeros((self.B, Cn), np.float64)
    eps = np.zeros((self.B, Cn), np.float64)
    _check(self._lib.ci_ll_session_hmc_fetch(self._h, _ptr(draws), acc.ctypes.data,
                                             eps.ctypes.data, C.byref(out)))
    return draws, acc, eps, arrs

  def hmc(self, **kw):
    raise NotImplementedError("use hmc_run + hmc_fetch on a batched session")

  def fetch(self, want) -> Dict[str, np.ndarray]:
    """`Session.fetch` of the finished fit: the fields of `want` that the trend model has."""
    return self.hmc_fetch([k for k in want if k not in ("seasonal_drift_scales", "seasonal_levels")],
                          with_draws=False)[3]

  def summarize(self, scale, shift, observed, flags, ranks) -> Dict[str, np.ndarray]:
    """`Session.summarize` of the fit's resident predictive trajectories (ci_ll_session_hmc_summarize):
    value_order [B,R,T], cum_order [B,R,T], per_draw [B,2,N], per_draw_order [B,2,R], N = C x S
    (the series axis is kept for B = 1)."""
    Cn, S = self._hmc_shape
    B, T, N = self.B, self.T, Cn * S
    sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, np.float64), (B,)))
    sh = np.ascontiguousarray(np.broadcast_to(np.asarray(shift, np.float64), (B,)))
    obs = np.ascontiguousarray(np.broadcast_to(np.asarray(observed, np.float64), (B, T)))
    fl = np.ascontiguousarray(np.broadcast_to(np.asarray(flags, np.uint8), (B, T)))
    rk = np.ascontiguousarray(ranks, dtype=np.int32)
    vo = np.empty((B, rk.size, T), np.float64)
    co = np.empty((B, rk.size, T), np.float64)
    pd_ = np.empty((B, 2, N), np.float64)
    do = np.empty((B, 2, rk.size), np.float64)
    _check(self._lib.ci_ll_session_hmc_summarize(self._h, sc.ctypes.data, sh.ctypes.data,
                                                 obs.ctypes.data, fl.ctypes.data, int(rk.size),
                                                 rk.ctypes.data, vo.ctypes.data, co.ctypes.data,
                                                 pd_.ctypes.data, do.ctypes.data))
    return dict(value_order=vo, cum_order=co, per_draw=pd_, per_draw_order=do)

  def summarize_windows(self, scale, shift, observed, first, count, ranks,
                        want_draws=True) -> Dict[str, np.ndarray]:
    """`Session.summarize_windows` of the fit's resident predictive trajectories
    (ci_ll_session_summarize_windows): per_draw [B, W, 2, N], per_draw_order [B, W, 2, R], N = C x S."""
    fn = _symbol(self._lib, "ci_ll_session_summarize_windows")
    Cn, S = self._hmc_shape
    return _windows_call(fn, self._h, self.B, Cn * S, self.T, scale, shift, observed, first, count,
                         ranks, want_draws)

  def summarize_paths(self, scale, shift, observed, first, count, ranks,
                      want=PATH_OUTPUTS) -> Dict[str, np.ndarray]:
    """`Session.summarize_paths` of the fit's resident predictive trajectories
    (ci_ll_session_summarize_paths), N = C x S."""
    fn = _symbol(self._lib, "ci_ll_session_summarize_paths")
    Cn, S = getattr(self, "_hmc_shape", (0, 0))           # (before a run: the entry refuses the call)
    return _paths_call(fn, self._h, self.B, Cn * S, self.T, scale, shift, observed, first, count, ranks,
                       want)


def test_rng(seed, chain, it, site, sub, n, alpha, device=0):
  L = load()
  s = (C.c_uint32 * 2)(*seed_pair(seed))
  u = np.zeros(n, np.float32)
  z = np.zeros(2 * n, np.float32)
  g = np.zeros(1, np.float64)
  _check(L.ci_test_rng(device, s, chain, it, site, sub, n, u.ctypes.data, z.ctypes.data,
                       float(alpha), g.ctypes.data))
  return u, z[:n], z[n:], float(g[0])


def test_dk_draw(pb: Problem, params, resid, mask, obs_scale, level_scale, slope_scale=0.0, it=0):
  L = load()
  T, D = pb.T, 2 if pb.has_slope else 1
  r32 = np.ascontiguousarray(np.asarray(resid, np.float32))
  m8 = np.ascontiguousarray(np.asarray(mask, bool).astype(np.uint8))
  out = np.zeros((T, D), np.float32)
  _check(L.ci_test_dk_draw(C.byref(pb), params, r32.ctypes.data, m8.ctypes.data, None,
                           float(obs_scale), float(level_scale), float(slope_scale), None, int(it),
                           out.ctypes.data))
  return out
