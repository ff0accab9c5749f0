"""The shapes and inputs the draws-session tests share (tests/test_draws_session.py on the CPU,
tests/test_gpu_draws_session.py and tests/test_gpu_draw_routes.py on the device).

B = 3 series of T = 70 steps with P = 2 design columns; C = 2 chains x S = 40 kept draws, N = 80 pooled
draws: one full wavefront and a remainder of 16 lanes.  The steps 11, 12 and 40 are missing inside the
pre-period and the post-period (from step 49 on) is masked.  Three origins per series with horizon 9;
the last series leaves its last slot unused.  Every comparison to a numpy twin is at rtol 1e-8, atol
1e-8, the project's float64 contract."""
import numpy as np

from causalimpact import _model
from causalimpact import _native
from causalimpact import _synthetic as syn
from causalimpact import causalimpact_lib as lib

B, T, P, C, S = 3, 70, 2, 2, 40
N = C * S
PRE = 49
HORIZON = 9
SEED = (5, 9)
TOL = dict(rtol=1e-8, atol=1e-8)
RANKS = [0, 1, 40, 78, 79]
ORIGINS = np.asarray([[15, 27, 39], [16, 28, 40], [17, 36, -1]], np.int32)
DRAW_FIELDS = ["observation_noise_scale", "level_scale", "slope_scale", "seasonal_drift_scales", "weights"]
PRED = ("forecast_mean", "forecast_order", "variance_mean", "pit_mean", "loglik")
PLAC = ("predicted_mean", "spread_mean", "pit_mean")
SIM = ("predicted_mean", "spread_mean", "below", "total_order")
# two groups of a pooled placebo, the second weighted; one horizon per group
GROUPS = [{0: 1.0, 2: 1.0}, {1: 0.5, 2: -2.0}]
GROUP_HORIZON = [9, 6]

# name: (has_slope, seasons as (num_seasons, num_steps_per_season), the `_blocks` entries)
MODELS = {
    "trend": (False, (), False),
    "slope+7 d=8": (True, ((7, 1),), False),            # the widest state of the one-lane kernels
    "4+3 d=6": (False, ((4, 1), (3, 1)), True),         # groups of 8 lanes
    "slope+12 d=13": (True, ((12, 1),), True),          # groups of 16 lanes
}


def series(b, has_slope, seasons, level=0.0):
  """(y, mask, X, spec) of series b; level: added to the standardised outcome."""
  y, mask, X, _ = syn.standardize_for_sampler(*syn.make_raw_series(T, P - 1, 40 + 7 * b + P), PRE)
  if seasons:
    y = y + 0.8 * np.sin(2 * np.pi * np.arange(T) / 7.0)
  y = y + level
  mask = mask.copy()
  mask[[11, 12, 40]] = True
  spec = _model.series_params(np.where(mask, np.nan, y), mask, X, has_slope=has_slope,
                              num_seasonal_blocks=len(seasons))
  return y, mask, X, spec


def inputs(name, level=0.0):
  """The B series of model `name`: y, mask [B, T], X [B, T, P], the specs, num_seasons and the change
  flags [K, T]."""
  has_slope, seasons, _ = MODELS[name]
  rows = [series(b, has_slope, seasons, level) for b in range(B)]
  num_seasons, sc = _model.expand_seasons(seasons, T)
  return dict(y=np.stack([r[0] for r in rows]), mask=np.stack([r[1] for r in rows]),
              X=np.stack([r[2] for r in rows]), specs=[r[3] for r in rows], num_seasons=num_seasons, sc=sc,
              has_slope=has_slope)


def problem(name, chain_offset=0, series_offset=0, num_warmup=10, which=None):
  has_slope, seasons, _ = MODELS[name]
  num_seasons, _ = _model.expand_seasons(seasons, T)
  return _native.make_problem(T=T, P=P, has_slope=has_slope, num_warmup=num_warmup, num_results=S, num_chains=C,
                              num_series=B if which is None else 1, seed=SEED, chain_offset=chain_offset,
                              series_offset=series_offset, num_seasons=num_seasons)


def synthetic_draws(name, seed=3):
  """Float32 parameter draws {name: [B, C, S, ...]} of plausible size for model `name`, made without
  a fit: positive scales around the priors' scale, weights around 0.5."""
  _, seasons, _ = MODELS[name]
  rng = np.random.default_rng(seed)
  K = len(seasons)
  f = lambda lo, hi, *tail: rng.uniform(lo, hi, (B, C, S) + tail).astype(np.float32)   # pylint: disable=unnecessary-lambda-assignment
  return dict(observation_noise_scale=f(0.3, 0.6), level_scale=f(0.02, 0.1), slope_scale=f(0.002, 0.01),
              seasonal_drift_scales=f(0.01, 0.05, K), weights=f(0.2, 0.8, P))


# ---- the float64 case: inputs that float32 cannot hold ------------------------------------------------
F64_LEVEL = 1000.0                  # the outcome's level: float32 holds it to 6e-5
F64_SCALE, F64_SHIFT = 1.0, -1000.0  # ... and the forecasts are reported around 0, where 1e-8 is absolute


def f64_case(name):
  """(inputs, draws) of the float64 test: the outcome at level 1000, the design and `synthetic_draws`,
  each multiplied by (1 + 1e-3 u), u uniform in float64 -- none of it float32-representable."""
  inp = inputs(name, F64_LEVEL)
  rng = np.random.default_rng(11)
  jitter = lambda a: np.asarray(a, np.float64) * (1.0 + 1e-3 * rng.uniform(size=np.shape(a)))   # pylint: disable=unnecessary-lambda-assignment
  inp = dict(inp, y=jitter(inp["y"]), X=jitter(inp["X"]))
  # (the parameter blocks are those of the jittered outcome: what a float64 fit would have been given)
  inp["specs"] = [_model.series_params(np.where(inp["mask"][b], np.nan, inp["y"][b]), inp["mask"][b], inp["X"][b],
                                       has_slope=inp["has_slope"], num_seasonal_blocks=len(inp["num_seasons"]))
                  for b in range(B)]
  draws = {k: jitter(v) for k, v in synthetic_draws(name).items()}
  return inp, draws


def pooled(draws, b):
  return {k: v[b].reshape((v.shape[1] * v.shape[2],) + v.shape[3:]) for k, v in draws.items()}


def twin_args(inp, draws, b, dtype):
  """The arguments of the numpy twins up to the draws, for series b as a sampler of `dtype` saw it."""
  return (np.where(inp["mask"][b], 0, inp["y"][b]).astype(dtype), inp["mask"][b], inp["X"][b].astype(dtype),
          inp["sc"], inp["num_seasons"], inp["has_slope"], inp["specs"][b],
          {k: v.astype(dtype) for k, v in pooled(draws, b).items()})


def twin_predictions(inp, draws, b, scale, shift, dtype=np.float64):
  return lib._prediction_summary_host(*twin_args(inp, draws, b, dtype), scale, shift, RANKS)   # pylint: disable=protected-access


def twin_placebo(inp, draws, b, scale, shift, dtype=np.float64, horizon=HORIZON, origins=None, per_draw=False):
  return lib._placebo_summary_host(*twin_args(inp, draws, b, dtype), scale, shift,             # pylint: disable=protected-access
                                   ORIGINS[b] if origins is None else origins, horizon, per_draw=per_draw)


def twin_simulated(inp, draws, b, scale, shift, link, stream, seen=None, horizon=HORIZON, dtype=np.float64):
  return lib._placebo_simulated_host(*twin_args(inp, draws, b, dtype), scale, shift, ORIGINS[b], horizon, link,   # pylint: disable=protected-access
                                     stream, seen=seen, ranks=RANKS)


def beyond(a, b, factor=100.0):
  """True where a and b differ by more than `factor` times the tolerance somewhere."""
  a, b = np.asarray(a), np.asarray(b)
  return bool(np.any(np.abs(a - b) > factor * (TOL["atol"] + TOL["rtol"] * np.abs(b))))
