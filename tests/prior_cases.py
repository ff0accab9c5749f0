"""A prior record in which no two fields agree, and the cases that run every float32 Gibbs build on it.

`oracle.default_spec` -- the record every float32 GPU test used -- sets level_ub == slope_ub ==
drift_ub == init_*_scale == sd, level_conc == slope_conc, level_scale == slope_scale,
weights_prior_scale == 1 and bounds no draw ever reaches: a kernel that reads one field for another,
or that never clips, passes.  This module builds the record that tells the fields apart:

  distinct_spec(spec)   every field at least 25 % away from every field it could be confused with
  bind_bounds(...)      the four upper bounds at the median of a pilot run of the ORACLE without
                        bounds, so that about half of the draws of every scale are clipped
  CASES                 shape, flags and the substring Session.kernel_name() must contain, one case
                        per build (the ROUTE_CASES pattern of test_gpu_float64_routes.py)
  deviations(a, w, T)   every compared output of a fit `a` against the oracle's `w`, in units of its
                        tolerance: the GPU test asserts <= 1, the CPU test that a swapped field moves
                        the oracle itself by >= 3

tests/test_prior_cases.py checks the table on the oracle alone; tests/test_gpu_prior_record.py runs
it on the device.  `python tests/prior_cases.py` writes profiles/prior_record_cases.txt."""
import collections
import copy
import functools
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "tfp-causalimpact_amd")):
  if _p not in sys.path:
    sys.path.insert(0, _p)

from causalimpact import _native            # noqa: E402  pylint: disable=wrong-import-position
from causalimpact import _synthetic as syn  # noqa: E402  pylint: disable=wrong-import-position
from oracle import ci_oracle as orc         # noqa: E402  pylint: disable=wrong-import-position

SEED = (5, 9)
NO_BOUND = 1e30
SEPARATION = 0.25
MARGIN = 3.0                 # a swapped field must move a compared output by 3 tolerances
EARLY = 4                    # draws 1-4 take the per-draw tolerances, later ones 2e-2

WEEK = ((7, 1),)
REF_SEASONS = ((4, (2, 1, 1, 1)), (7, 1), (6, ((2, 2, 1, 1, 1, 1), (2, 2, 1, 1, 1, 1))))
SEQ = _native.FLAG_SEQUENTIAL_SEASONAL
FOUR = _native.FLAG_FOUR_WAVES
WS = _native.FLAG_SEASONAL_WORKSPACE
CLUSTER = _native.FLAG_CLUSTER_SEASONAL
MW = _native.FLAG_MULTIWAVE_SEASONAL

FAMILIES = {1: "trend (ci_kernels.h, ci_kernels8.h)", 2: "regression blocks (ci_kernels.h, ci_bigp.h)",
            3: "ci_wide.h", 4: "sequential ci_seasonal.h", 5: "time-parallel ci_seasonal_tp.h",
            6: "multi-wave ci_seasonal_mw.h"}

Case = collections.namedtuple("Case", "name family T p has_slope seasons flags kernel S data_seed extra")


def _case(name, family, T, p, has_slope, seasons=(), flags=0, kernel="", S=12, data_seed=0, **extra):
  return Case(name, family, T, p, has_slope, seasons, flags, kernel, S, data_seed, extra)


# P = 0 has one build, four wavefronts (no regression wave to add): FLAG_FOUR_WAVES changes nothing there.
CASES = [
    _case("trend-p0", 1, 100, 0, 0, kernel="gibbs_kernel<1,1,0,false>"),
    _case("trend-8w", 1, 300, 4, 1, kernel="gibbs_kernel8<2,2>"),
    _case("trend-8w-L8", 1, 1500, 12, 0, kernel="gibbs_kernel8<1,8,L2>"),      # the design read from L2
    _case("trend-4w", 1, 300, 4, 1, flags=FOUR, kernel="gibbs_kernel<2,2,1,false>"),
    _case("trend-4w-p0", 1, 100, 0, 0, flags=FOUR, kernel="gibbs_kernel<1,1,0,false>"),
    _case("block-wave", 2, 260, 19, 0, kernel="gibbs_kernel<1,2,2,false>"),
    _case("block-workgroup", 2, 300, 31, 1, kernel="gibbs_kernel<2,2,2,false>"),
    _case("bigp-wide", 2, 400, 60, 0, kernel="gibbs_wide_kernel<1,2,bigp>"),
    _case("bigp-tp", 2, 400, 60, 0, flags=CLUSTER, kernel="gibbs_seasonal_tp_kernel"),
    _case("bigp-seq", 2, 400, 60, 0, flags=SEQ, kernel="gibbs_seasonal_kernel<false,true>"),
    _case("bigp-weekly", 2, 350, 66, 0, WEEK, kernel="gibbs_wide_kernel<1,7,bigp>"),
    # (five columns or fewer: the weights' prior decides no inclusion at 2.5 times the default -- these carry
    #  weights_prior_scale and, through it, obs_scale0 with a stronger prior)
    _case("wide-weekly", 3, 120, 4, 1, WEEK, kernel="gibbs_wide_kernel<2,7>", weights_prior_scale=40.0),
    _case("wide-weekly-p0", 3, 120, 0, 0, WEEK, kernel="gibbs_wide_kernel<1,7>"),
    _case("wide-long", 3, 5000, 3, 0, kernel="gibbs_wide_kernel<1,2>", S=6,
          level_scale0=0.02),     # (from 0.045 sd the level scale only falls over six draws: one clipped draw)
    _case("wide-p21", 3, 1030, 20, 0, WEEK, kernel="gibbs_wide_kernel<1,7>",        # spike_slab_draw_block on ci_wide.h
          level_scale0=0.035),
    _case("seq-weekly", 4, 120, 4, 1, WEEK, flags=SEQ, kernel="gibbs_seasonal_kernel<false,false>"),
    _case("seq-d13", 4, 200, 2, 0, ((12, 1),), flags=SEQ, kernel="gibbs_seasonal_kernel<false,false>"),
    _case("seq-d64", 4, 250, 0, 1, ((62, 1),), kernel="gibbs_seasonal_kernel<"),
    _case("seq-workspace", 4, 300, 3, 0, REF_SEASONS, flags=WS, kernel="gibbs_seasonal_kernel<true,false>"),
    _case("seq-p21", 4, 300, 20, 0, REF_SEASONS, flags=SEQ, kernel="gibbs_seasonal_kernel<",     # spike_slab_draw
          level_scale=0.036, level_scale0=0.03),   # (at 0.05 sd the level bound meets the bound of the obs variance)
    _case("tp-ref", 5, 112, 3, 0, REF_SEASONS, kernel="gibbs_seasonal_tp_kernel"),
    _case("tp-d10", 5, 130, 2, 1, ((5, 1), (3, 5)), kernel="gibbs_seasonal_tp_kernel", weights_prior_scale=400.0),
    _case("tp-p21", 5, 300, 20, 0, REF_SEASONS, kernel="gibbs_seasonal_tp_kernel",                 # spike_slab_draw
          level_scale=0.036, level_scale0=0.03),
    _case("mw-d53", 6, 300, 3, 0, ((52, 1),), flags=MW, kernel="(multi-wave)", weights_prior_scale=400.0),
]
CASE_BY_NAME = {c.name: c for c in CASES}

# Three series with three different records in ONE launch: (name, the case whose model and flags it
# takes, the three lengths, ragged session, kernel substring).  Series b is variant b of that case.
Batch = collections.namedtuple("Batch", "name case lengths ragged kernel")
BATCH_CASES = [
    Batch("batch-4w", "trend-4w", (300, 300, 300), False, "gibbs_kernel<2,2,1,false>"),
    Batch("batch-wide", "wide-weekly", (120, 120, 120), False, "gibbs_wide_kernel<2,7>"),
    Batch("ragged-trend", "trend-4w", (300, 287, 261), True, "gibbs_kernel<2,2,1,false,ragged>"),
    Batch("ragged-wide", "wide-weekly", (120, 113, 99), True, "gibbs_wide_kernel<2,7,ragged>"),
]
BATCH_BY_NAME = {b.name: b for b in BATCH_CASES}


def batch_members():
  """Every (case, variant, T) that some batch runs."""
  return sorted({(bc.case, b, T) for bc in BATCH_CASES for b, T in enumerate(bc.lengths)})

# ---- the record -------------------------------------------------------------------------------------
# fields a kernel could read for one another: each group is checked pairwise for the 25 % separation
GROUPS = {
    "conc": ("level_conc", "slope_conc", "obs_conc", "drift_conc"),
    "scale": ("level_scale", "slope_scale", "obs_scale", "drift_scale"),
    "ub": ("level_ub", "slope_ub", "obs_ub", "drift_ub"),
    "init": ("init_level_scale", "init_slope_scale", "init_seasonal_scale"),
    "scale0": ("obs_scale0", "level_scale0", "slope_scale0"),      # + every drift_scale0[k]
}


def distinct_spec(spec, **over):
  """A copy of a `default_spec` record with every field moved off its siblings (the bounds stay to be
  set by `bind_bounds`).  `over`: fields a case sets for itself."""
  d = copy.deepcopy(spec)
  sd, P = spec["outcome_sd"], spec["P"]
  d.update(
      level_conc=40.0, level_scale=40.0 * (0.05 * sd) ** 2,
      slope_conc=3.0, slope_scale=3.0 * (0.004 * sd) ** 2,
      obs_conc=14.0 if P > 0 else 0.7, obs_scale=(3.0 if P > 0 else 0.4) * sd * sd,
      drift_conc=8.0, drift_scale=8.0 * (0.02 * sd) ** 2,
      # (the default min(1, 3/P) is 0.6 at five columns and below 0.16 from twenty on)
      nonzero_prob=(0.35 if P <= 8 else 0.6) if P > 1 else spec["nonzero_prob"],
      init_level_loc=spec["init_level_loc"] + 2.5 * sd,
      init_level_scale=0.7 * sd, init_slope_scale=0.02 * sd, init_seasonal_scale=0.15 * sd,
      obs_scale0=0.36 * sd, level_scale0=0.045 * sd,
      slope_scale0=0.0025 * sd if spec["has_slope"] else 0.0,
      drift_scale0=[0.004 * sd * 2.0 ** k for k in range(len(spec["drift_scale0"]))],
      weights_prior_scale=2.5,
      level_ub=NO_BOUND, slope_ub=NO_BOUND, obs_ub=NO_BOUND, drift_ub=NO_BOUND)
  d.update(over)
  return d


def bind_bounds(y, mask, X, spec, S, seed):
  """The record with its four bounds at the median of what the oracle draws without them: level_ub,
  slope_ub, drift_ub (pooled over blocks) and, without a regression, obs_ub bound a SCALE; with one
  obs_ub bounds the VARIANCE.  Nothing but the reference decides them."""
  pilot = dict(spec, level_ub=NO_BOUND, slope_ub=NO_BOUND, obs_ub=NO_BOUND, drift_ub=NO_BOUND)
  w = orc.fit_gibbs(y, mask, X, pilot, num_results=S, num_warmup=0, seed=seed,
                    want=("obs_scale", "level_scale", "slope_scale", "drift_scales"))
  out = dict(pilot)
  out["level_ub"] = float(np.median(w["level_scale"]))
  if spec["has_slope"]:
    out["slope_ub"] = float(np.median(w["slope_scale"]))
  else:
    out["slope_ub"] = 0.1 * out["level_ub"]          # never read; off its siblings all the same
  if len(spec["num_seasons"]):
    out["drift_ub"] = float(np.median(w["drift_scales"]))
  else:
    out["drift_ub"] = 0.4 * out["level_ub"]          # read by no draw of a model without blocks
  obs = w["obs_scale"] if spec["P"] == 0 else w["obs_scale"] ** 2
  out["obs_ub"] = float(np.median(obs))
  return out


def make_series(T, p, has_slope, seasons, data_seed=0):
  """(y, mask, X or None, default spec): the synthetic series of the per-draw tests with a weekly wave,
  gaps in the pre-period and the first three steps unobserved (the prior of the first state carries
  over them)."""
  y, mask, X, _ = syn.make_sampler_inputs(T, p, data_seed)
  y = y + 0.5 * np.sin(2 * np.pi * np.arange(T) / 7.0)
  mask = mask.copy()
  mask[[0, 1, 2, 3, 40, T // 2]] = True
  return y, mask, X, orc.default_spec(y, mask, X, has_slope=bool(has_slope), seasons=seasons)


@functools.lru_cache(maxsize=None)
def case_inputs(name, variant=0, T=None):
  """(y, mask, X, spec) of a case: the distinct record with pilot-median bounds.  `variant` > 0: another
  series with another record, `T`: of another length (three records in one launch: BATCH_CASES)."""
  c = CASE_BY_NAME[name]
  y, mask, X, base = make_series(T or c.T, c.p, c.has_slope, c.seasons, c.data_seed + 17 * variant)
  spec = distinct_spec(base, **c.extra)
  if variant:
    spec = vary(spec, variant)
  spec = bind_bounds(y, mask, X, spec, c.S, stream(c, variant))
  for a in (y, mask) + (() if X is None else (X,)):
    a.setflags(write=False)
  return y, mask, X, spec


def vary(spec, b):
  """Record number b of a batch: every field of series 0's record times its own factor, so that no two
  series of a launch share a value (the bounds follow from each record's own pilot)."""
  d = copy.deepcopy(spec)
  f = (1.0, 1.7, 0.55)[b]
  for k in ("level_conc", "slope_conc", "obs_conc", "drift_conc"):
    d[k] = spec[k] * (1.0, 1.5, 2.2)[b]
  for k in ("level_scale", "slope_scale", "obs_scale", "drift_scale", "init_level_scale", "init_slope_scale",
            "init_seasonal_scale", "obs_scale0", "level_scale0", "slope_scale0", "weights_prior_scale"):
    d[k] = spec[k] * f
  d["drift_scale0"] = [v * f for v in spec["drift_scale0"]]
  d["init_level_loc"] = spec["init_level_loc"] + (0.0, 1.5, -5.5)[b] * spec["outcome_sd"]   # 2.5, 4, -3 sd off
  if spec["P"] > 1:
    d["nonzero_prob"] = spec["nonzero_prob"] * (1.0, 0.5, 0.2)[b]
  return d


def filter_record(params, P, has_slope, b):
  """Record b of a session whose filters are checked (tests/test_gpu_predictions.py, test_gpu_placebo.py):
  `_model.series_params` made distinct, varied by series, with bounds near what such a fit draws (they are
  read by the fit, not by the filters)."""
  d = vary(distinct_spec(dict(params, P=P, has_slope=int(has_slope))), b)
  sd = params["outcome_sd"]
  d.update(level_ub=0.06 * sd, slope_ub=0.005 * sd, drift_ub=0.03 * sd, obs_ub=(0.5 if P else 0.8) * sd)
  return d


def stream(c, variant=0):
  """The Philox key of a case's fit: series b > 0 of a batch has its own, series 0 the plain seed."""
  del c
  return SEED if variant == 0 else tuple(_native.series_stream_key(SEED, variant))


def oracle_fit(name, spec=None, variant=0, T=None):
  c = CASE_BY_NAME[name]
  y, mask, X, own = case_inputs(name, variant, T)
  return orc.fit_gibbs(y, mask, X, own if spec is None else spec, num_results=c.S, num_warmup=0,
                       seed=stream(c, variant))


@functools.lru_cache(maxsize=None)
def oracle_reference(name, variant=0, T=None):
  """The oracle's fit of a case, computed once and shared read-only."""
  w = oracle_fit(name, variant=variant, T=T)
  for v in w.values():
    v.setflags(write=False)
  return w


# ---- the comparison ---------------------------------------------------------------------------------
DEVICE_NAMES = dict(obs_scale="observation_noise_scale", level_scale="level_scale", slope_scale="slope_scale",
                    drift_scales="seasonal_drift_scales", weights="weights", level="level", slope="slope",
                    seasonal="seasonal_levels", trajectories="posterior_trajectories", pred_mean="posterior_means")


def from_device(got, b=0, c=0):
  """Series b, chain c of a device fit under the oracle's names."""
  return {k: np.asarray(got[v][b, c], np.float64) for k, v in DEVICE_NAMES.items() if v in got}


def tolerances(w, T, has_slope, P, K):
  """{output: allowed |difference| per element, shaped like the oracle's array}: draws 1-4 at the
  tolerances of the per-draw tests of tests/test_gpu_gibbs.py (5e-3 relative on the scales, 2e-2
  relative on the drift scales, 5e-3 on weights and paths, 1e-2 on trajectories, plus 2e-3 of the level's
  range from 4096 steps on), later draws at 2e-2 throughout (the 40-iteration test of the regression
  block).  posterior_means is the mean over the draws, so it takes the mean of their tolerances."""
  S = w["level"].shape[0]
  lev = 5e-3 if T < 4096 else 5e-3 + 2e-3 * float(np.ptp(w["level"]))
  late = np.arange(S) >= EARLY

  def per_draw(early, arr, relative):
    tol = np.where(late, 2e-2, early).reshape((S,) + (1,) * (arr.ndim - 1))
    return tol * np.abs(arr) if relative else np.broadcast_to(tol, arr.shape)

  tol = dict(obs_scale=per_draw(5e-3, w["obs_scale"], True), level_scale=per_draw(5e-3, w["level_scale"], True),
             level=per_draw(lev, w["level"], False), trajectories=per_draw(2 * lev, w["trajectories"], False))
  tol["pred_mean"] = np.full(w["pred_mean"].shape, (min(S, EARLY) * lev + max(S - EARLY, 0) * 2e-2) / S)
  if has_slope:
    tol["slope_scale"] = per_draw(5e-3, w["slope_scale"], True)
    tol["slope"] = per_draw(5e-3, w["slope"], False)
  if P:
    tol["weights"] = per_draw(5e-3, w["weights"], False)
  if K:
    tol["drift_scales"] = per_draw(2e-2, w["drift_scales"], True)
    tol["seasonal"] = per_draw(5e-3, w["seasonal"], False)
  return tol


def deviations(a, w, T, has_slope, P, K):
  """{output: max |a - w| / tolerance}; 'inclusion' is inf where the patterns of included columns differ."""
  out = {}
  for k, tol in tolerances(w, T, has_slope, P, K).items():
    out[k] = float(np.max(np.abs(np.asarray(a[k], np.float64) - w[k]) / tol)) if w[k].size else 0.0
  if P:
    out["inclusion"] = 0.0 if np.array_equal(np.asarray(a["weights"]) != 0, w["weights"] != 0) else np.inf
  return out


def case_deviations(name, a, variant=0, T=None):
  c = CASE_BY_NAME[name]
  spec = case_inputs(name, variant, T)[3]
  return deviations(a, oracle_reference(name, variant, T), T or c.T, c.has_slope, spec["P"], len(c.seasons))


# ---- (a) separation ---------------------------------------------------------------------------------
def apart(a, b):
  return abs(a - b) >= SEPARATION * max(abs(a), abs(b))


def separation_failures(spec):
  """Pairs of confusable fields of a record that are less than 25 % apart."""
  bad = []
  for group, names in GROUPS.items():
    vals = [(n, spec[n]) for n in names]
    if group == "scale0":
      vals += [(f"drift_scale0[{k}]", v) for k, v in enumerate(spec["drift_scale0"])]
      if not spec["has_slope"]:
        vals = [v for v in vals if v[0] != "slope_scale0"]      # 0: the model has no slope scale
    for i, (n1, v1) in enumerate(vals):
      for n2, v2 in vals[i + 1:]:
        if not apart(v1, v2):
          bad.append((n1, v1, n2, v2))
  P = spec["P"]
  if P > 1 and (not apart(spec["nonzero_prob"], min(1.0, 3.0 / P)) or not spec["nonzero_prob"] < 1.0):
    bad.append(("nonzero_prob", spec["nonzero_prob"], "default", min(1.0, 3.0 / P)))
  if not apart(spec.get("weights_prior_scale", 1.0), 1.0):
    bad.append(("weights_prior_scale", spec.get("weights_prior_scale", 1.0), "default", 1.0))
  return bad


# ---- (b) clip counts --------------------------------------------------------------------------------
def clip_counts(name, variant=0, T=None):
  """{scale: (clipped, unclipped)} of the oracle's draws; 'drift' pooled, 'drift[k]' per block."""
  c = CASE_BY_NAME[name]
  spec, w = case_inputs(name, variant, T)[3], oracle_reference(name, variant, T)
  P = spec["P"]

  def count(draws, ub):
    assert np.all(draws <= ub * (1 + 1e-12))
    hit = np.isclose(draws, ub, rtol=1e-12, atol=0.0)
    return int(hit.sum()), int((~hit).sum())

  out = {"obs": count(w["obs_scale"] if P == 0 else w["obs_scale"] ** 2, spec["obs_ub"]),
         "level": count(w["level_scale"], spec["level_ub"])}
  if c.has_slope:
    out["slope"] = count(w["slope_scale"], spec["slope_ub"])
  if c.seasons:
    out["drift"] = count(w["drift_scales"], spec["drift_ub"])
    for k in range(len(c.seasons)):
      out[f"drift[{k}]"] = count(w["drift_scales"][:, k], spec["drift_ub"])
  return out


# ---- (c) sensitivity --------------------------------------------------------------------------------
def swaps(name):
  """{field: the record with that field replaced by its sibling's value (or the default's)}, for every
  field the case's model has."""
  c = CASE_BY_NAME[name]
  y, mask, _, spec = case_inputs(name)
  P, K = spec["P"], len(c.seasons)
  out = {}

  def put(field, value):
    out[field] = dict(spec, **{field: value})

  for part in ("conc", "scale", "ub"):
    put(f"level_{part}", spec[f"slope_{part}"])
    put(f"obs_{part}", spec[f"level_{part}"])
    if c.has_slope:
      put(f"slope_{part}", spec[f"level_{part}"])
    if K:
      put(f"drift_{part}", spec[f"level_{part}"])
  put("init_level_scale", spec["init_slope_scale"])
  put("init_level_loc", float(y[~mask][0]))
  put("obs_scale0", spec["level_scale0"])
  put("level_scale0", spec["slope_scale0"] if c.has_slope else 0.0025 * spec["outcome_sd"])
  if c.has_slope:
    put("init_slope_scale", spec["init_level_scale"])
    put("slope_scale0", spec["level_scale0"])
  if K:
    put("init_seasonal_scale", spec["init_level_scale"])
    for k in range(K):
      d0 = list(spec["drift_scale0"])
      d0[k] = spec["drift_scale0"][k + 1] if k + 1 < K else spec["level_scale0"]
      out[f"drift_scale0[{k}]"] = dict(spec, drift_scale0=d0)
  if P > 1:
    put("nonzero_prob", min(1.0, 3.0 / P))
  if P:
    put("weights_prior_scale", 1.0)
  return out


@functools.lru_cache(maxsize=None)
def sensitivity(name):
  """{field: (ratio, output)}: how far the swap of that field moves the oracle, in tolerances of the
  output it moves most."""
  out = {}
  for field, swapped in swaps(name).items():
    dev = case_deviations(name, oracle_fit(name, spec=swapped))
    best = max(dev, key=dev.get)
    out[field] = (dev[best], best)
  return out


def inert_fields_change_nothing(name):
  """A trend-only series on ci_wide.h carries an inert block: the oracle, which has none, ignores the
  record's drift_* and init_seasonal_scale.  True when the oracle's fit does not depend on them."""
  spec, w = case_inputs(name)[3], oracle_reference(name)
  other = dict(spec, drift_conc=spec["level_conc"], drift_scale=spec["level_scale"], drift_ub=spec["level_ub"],
               init_seasonal_scale=spec["init_level_scale"])
  v = oracle_fit(name, spec=other)
  return all(np.array_equal(v[k], w[k]) for k in w)


def carriers():
  """{(family, field): (ratio, case, output)}: the case of each family in which the field is strongest."""
  best = {}
  for c in CASES:
    for field, (ratio, output) in sensitivity(c.name).items():
      key = (c.family, field.split("[")[0] if field.startswith("drift_scale0") else field)
      if key not in best or ratio > best[key][0]:
        best[key] = (ratio, c.name, output)
  return best


def main():
  lines = ["Prior-record cases: the oracle's clip counts and the sensitivity of every field (tests/prior_cases.py).",
           "clip counts: clipped/unclipped draws of each scale; sensitivity: |oracle(swapped) - oracle| / tolerance.",
           ""]
  for c in CASES:
    spec = case_inputs(c.name)[3]
    counts = clip_counts(c.name)
    lines.append(f"{c.name}: family {c.family}, T={c.T} p={c.p} slope={c.has_slope} seasons={c.seasons} "
                 f"flags={c.flags} S={c.S} kernel~'{c.kernel}'")
    lines.append("  bounds: " + " ".join(f"{k}={spec[k]:.5g}" for k in GROUPS["ub"]))
    lines.append("  clips:  " + " ".join(f"{k}={a}/{b}" for k, (a, b) in counts.items()))
    lines.append("  sensitivity: " + " ".join(f"{f}={r:.3g}({o})" for f, (r, o) in sensitivity(c.name).items()))
  lines += ["", "Three records in one launch (series b of a batch: record b on its own data and length):"]
  for bc in BATCH_CASES:
    for b, T in enumerate(bc.lengths):
      counts = clip_counts(bc.case, b, T)
      lines.append(f"  {bc.name} series {b} (model of {bc.case}, T={T}): clips "
                   + " ".join(f"{k}={a}/{c}" for k, (a, c) in counts.items()))
  lines += ["", "Carrier of every field in every family that reads it (ratio >= 3 required; inf: the swap changes",
            "the pattern of included columns, which must be identical):"]
  for (family, field), (ratio, name, output) in sorted(carriers().items()):
    lines.append(f"  family {family} {field:22s} {ratio:10.3g}  {name} ({output})")
  path = os.path.join(_ROOT, "profiles", "prior_record_cases.txt")
  with open(path, "w") as f:
    f.write("\n".join(lines) + "\n")
  print("\n".join(lines))


if __name__ == "__main__":
  main()
