"""What filtering on the device costs the fits whose parameter draws lie on the host (float64 fits, HMC
fits, chains pooled over devices), next to the numpy twins they used to run -- at the shape of BASELINE
cfg5 (T = 500, 5 covariates, 1 chain x 1000 draws; the default placebo plan: 32 origins, horizon 116).

The filter step alone (`--legs filter`), for one series and for a block of 64, for the local-level
model and for `Seasons(7)` + `Seasons(4, num_steps_per_season=7)`: a float32 Gibbs session is fitted
and its parameter draws fetched; then
  device  `_native.DrawsSession` created from those draws, `summarize_predictions`,
          `summarize_placebo`, `simulate_placebo` (the `_blocks` entries for the seasonal model) and
          `close`, uploads included -- as float32, and with the same values as float64;
  numpy   the twins `_prediction_summary_host`, `_placebo_summary_host`, `_placebo_simulated_host` on
          the same draws, over `--twin-share` series of the block (they loop over the series).
End to end (`--legs e2e`, with `--baseline-root DIR`, a built checkout of the parent commit):
`fit_causalimpact(dtype=float64)` on one series and `fit_causalimpact_batch(sampler="hmc")` on 64
series, each as two calls -- `prediction_errors=True` with `placebo=True`, then
`placebo=Placebo(simulate=True)` -- parent and branch alternating.

Every run is a fresh child process; a leg is the median of its `--rounds` runs, the legs of a round
interleaved.  A device run reports `cold_ms` (the first pass of the process: code objects loaded, the
scratch allocated) and `warm_ms` (the same pass again).  One JSON line per leg in `--out`.

  python tools/exp_draw_filters.py [--legs filter,e2e] [--baseline-root DIR] [--rounds 5]
      [--out profiles/draw_filters.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (`--root DIR`, the child runs: the tree whose package is measured, the parent's checkout or this one)
TREE = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else ROOT
for p in (TREE, os.path.join(TREE, "tfp-causalimpact_amd")):
  if p not in sys.path:
    sys.path.insert(0, p)

import numpy as np  # pylint: disable=wrong-import-position
import pandas as pd  # pylint: disable=wrong-import-position

import causalimpact as ci  # pylint: disable=wrong-import-position
from causalimpact import _model, _native, batch  # pylint: disable=wrong-import-position
from causalimpact import _synthetic as syn  # pylint: disable=wrong-import-position
from causalimpact import causalimpact_lib as lib  # pylint: disable=wrong-import-position

DRAWS = ("observation_noise_scale", "level_scale", "slope_scale", "seasonal_drift_scales", "weights")
MODELS = {"level": dict(), "weekly+monthly": dict(seasons=[ci.Seasons(7), ci.Seasons(4, num_steps_per_season=7)])}
ALPHA, SEED = 0.05, (0, 1)


def values_of(B, T, covariates):
  return np.stack([np.column_stack(syn.make_raw_series(T, covariates, b)) for b in range(B)])


def periods(T):
  return (0, int(0.7 * T) - 1), (int(0.7 * T), T - 1)


def filter_child(a):
  """One run of one leg of the filter step: a JSON line with its milliseconds."""
  B, T = a.series, a.steps
  mo = MODELS[a.model]
  prep = batch.prepare_batch(values_of(B, T, a.covariates), pd.RangeIndex(T), *periods(T))
  P = prep.design.shape[2]
  num_seasons, sc = _model.expand_seasons(mo.get("seasons", ()), T)
  d = lib.prediction_state_dim(False, num_seasons)
  params = [_model.series_params(prep.y[b], prep.mask[b], prep.design[b], has_slope=False,
                                 num_seasonal_blocks=len(num_seasons),
                                 outcome_sd=float(np.nanstd(prep.y[b, :prep.num_pre], ddof=1))) for b in range(B)]
  n_post = int(np.count_nonzero(prep.flags & 2))
  origins, horizon = batch.placebo_plans(lib.Placebo(), [prep.num_pre] * B, [n_post] * B, d)
  pb = _native.make_problem(T=T, P=P, has_slope=False, num_warmup=-(-a.draws // 9), num_results=a.draws,
                            num_series=B, seed=SEED, num_seasons=num_seasons)
  sess = _native.Session(pb, prep.y, prep.mask, prep.design, sc if len(num_seasons) else None, _native.make_params(params))
  try:
    sess.run()
    draws = sess.fetch(list(DRAWS))
  finally:
    sess.close()
  scale, shift = prep.outcome_sd, prep.outcome_mean
  ranks = lib._summary_ranks(a.draws, (ALPHA / 2, 1 - ALPHA / 2))             # pylint: disable=protected-access
  sim_ranks = lib._placebo_sim_ranks(a.draws, (ALPHA / 2, 1 - ALPHA / 2))     # pylint: disable=protected-access
  seen = np.zeros(origins.shape)
  shape = dict(model=a.model, series=B, steps=T, covariates=a.covariates, draws=a.draws, state=d,
               origins=int(origins.shape[1]), horizon=int(horizon[0]))
  if a.route == "numpy":
    share = min(a.twin_share, B)
    dtype = np.float32
    t = [time.perf_counter()]
    for fn, tail in ((lib._prediction_summary_host, lambda b: (ranks,)),                      # pylint: disable=protected-access
                     (lib._placebo_summary_host, lambda b: (origins[b], int(horizon[b]))),    # pylint: disable=protected-access
                     (lib._placebo_simulated_host, lambda b: (origins[b], int(horizon[b]), _native.LINK_IDENTITY,   # pylint: disable=protected-access
                                                              lib.placebo_stream(SEED, b if B > 1 else None, range(1))))):
      for b in range(share):
        fn(np.where(prep.mask[b], 0.0, prep.y[b]).astype(dtype), prep.mask[b], prep.design[b].astype(dtype), sc,
           num_seasons, False, params[b], {k: draws[k][b, 0] for k in DRAWS}, scale[b], shift[b], *tail(b))
      t.append(time.perf_counter())
    ms = [(t[i + 1] - t[i]) * 1e3 for i in range(3)]
    print(json.dumps(dict(shape, route="numpy", share=share, predictions_ms=ms[0], placebo_ms=ms[1], simulated_ms=ms[2],
                          total_ms=sum(ms), per_series_ms=sum(ms) / share)), flush=True)
    return
  dtype = np.float64 if a.route == "device_f64" else np.float32
  blocks = not lib.device_predictions_supported(num_seasons)
  tail = "_blocks" if blocks else ""

  def once():
    t0 = time.perf_counter()
    drawn = _native.DrawsSession(pb, prep.y, prep.mask, prep.design, sc if len(num_seasons) else None,
                                 _native.make_params(params), {k: draws[k].astype(dtype) for k in DRAWS}, dtype=dtype)
    try:
      t1 = time.perf_counter()
      getattr(drawn, "summarize_predictions" + tail)(scale, shift, ranks)
      t2 = time.perf_counter()
      getattr(drawn, "summarize_placebo" + tail)(scale, shift, origins, horizon)
      t3 = time.perf_counter()
      drawn.simulate_placebo(scale, shift, origins, horizon, _native.LINK_IDENTITY, seen, sim_ranks, blocks=blocks)
      t4 = time.perf_counter()
    finally:
      drawn.close()
    t5 = time.perf_counter()
    return [(y - x) * 1e3 for x, y in ((t0, t1), (t1, t2), (t2, t3), (t3, t4), (t4, t5), (t0, t5))]
  cold, warm = once(), once()
  print(json.dumps(dict(shape, route=a.route, cold_ms=cold[5], warm_ms=warm[5], warm_create_ms=warm[0],
                        warm_predictions_ms=warm[1], warm_placebo_ms=warm[2], warm_simulated_ms=warm[3],
                        warm_close_ms=warm[4])), flush=True)


def e2e_child(a):
  """One run of one end-to-end case on the package of `--root`: a JSON line with its milliseconds."""
  T = a.steps
  calls = (dict(prediction_errors=True, placebo=True), dict(prediction_errors=False, placebo=ci.Placebo(simulate=True)))
  ms = []
  if a.case == "float64 fit":
    frame = pd.DataFrame(values_of(1, T, a.covariates)[0], index=pd.RangeIndex(T))
    for call in calls:
      t0 = time.perf_counter()
      got = ci.fit_causalimpact(frame, *periods(T), seed=1, alpha=ALPHA, data_options=ci.DataOptions(dtype=np.float64),
                                inference_options=ci.InferenceOptions(num_results=a.draws, prediction_errors=call["prediction_errors"]),
                                placebo=call["placebo"])
      ms.append((time.perf_counter() - t0) * 1e3)
    check = float(np.nansum(np.abs(got.placebo.select_dtypes("number").to_numpy())))
  else:
    values = values_of(a.series, T, a.covariates)
    for call in calls:
      t0 = time.perf_counter()
      got = ci.fit_causalimpact_batch(values, *periods(T), seed=1, alpha=ALPHA, index=pd.RangeIndex(T),
                                      inference_options=ci.InferenceOptions(num_results=a.draws, sampler="hmc",
                                                                            prediction_errors=call["prediction_errors"]),
                                      placebo=call["placebo"])
      ms.append((time.perf_counter() - t0) * 1e3)
    check = float(np.nansum(np.abs(got.placebo_quality.select_dtypes("number").to_numpy())))
  print(json.dumps(dict(case=a.case, series=a.series if a.case != "float64 fit" else 1, steps=T, covariates=a.covariates,
                        draws=a.draws, analytic_call_ms=ms[0], simulated_call_ms=ms[1], total_ms=sum(ms),
                        placebo_checksum=check)), flush=True)


def child(args, root=ROOT):
  cmd = [sys.executable, os.path.abspath(__file__), "--root", root] + [str(x) for x in args]
  out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout.strip().splitlines()
  return json.loads([l for l in out if l.startswith("{")][-1])


def median_of(runs, keys):
  return {k: statistics.median(r[k] for r in runs) for k in keys}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--legs", default="filter,e2e")
  ap.add_argument("--baseline-root", default=None, help="a built checkout of the parent commit (the e2e legs)")
  ap.add_argument("--rounds", type=int, default=5)
  ap.add_argument("--e2e-batch-rounds", type=int, default=None, help="rounds of the 64-series HMC batch (default: --rounds)")
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "draw_filters.jsonl"))
  ap.add_argument("--root", default=ROOT, help="(child runs) the tree whose package is imported")
  ap.add_argument("--child", choices=("filter", "e2e"), default=None)
  ap.add_argument("--model", choices=sorted(MODELS), default="level")
  ap.add_argument("--route", choices=("device_f32", "device_f64", "numpy"), default="device_f32")
  ap.add_argument("--case", choices=("float64 fit", "hmc batch"), default="float64 fit")
  ap.add_argument("--series", type=int, default=1)
  ap.add_argument("--twin-share", type=int, default=8)
  ap.add_argument("--steps", type=int, default=500)
  ap.add_argument("--covariates", type=int, default=5)
  ap.add_argument("--draws", type=int, default=1000)
  a = ap.parse_args()
  if a.child == "filter":
    return filter_child(a)
  if a.child == "e2e":
    return e2e_child(a)
  lines = []
  common = ["--steps", a.steps, "--covariates", a.covariates, "--draws", a.draws, "--twin-share", a.twin_share]
  if "filter" in a.legs.split(","):
    for model in MODELS:
      for series in (1, 64):
        runs = {route: [] for route in ("device_f32", "device_f64", "numpy")}
        for _ in range(a.rounds):                             # interleaved: drift hits all alike
          for route in runs:
            runs[route].append(child(["--child", "filter", "--model", model, "--series", series, "--route", route] + common))
        base = {k: runs["numpy"][0][k] for k in ("model", "series", "steps", "covariates", "draws", "state", "origins", "horizon")}
        twin = median_of(runs["numpy"], ("predictions_ms", "placebo_ms", "simulated_ms", "total_ms", "per_series_ms"))
        share = runs["numpy"][0]["share"]
        lines.append(json.dumps(dict(base, leg="filter step, numpy twins", rounds=a.rounds, share=share, **twin,
                                     whole_block_ms_derived=twin["per_series_ms"] * series)))
        for route in ("device_f32", "device_f64"):
          dev = median_of(runs[route], ("cold_ms", "warm_ms", "warm_create_ms", "warm_predictions_ms", "warm_placebo_ms",
                                        "warm_simulated_ms", "warm_close_ms"))
          lines.append(json.dumps(dict(base, leg=f"filter step, DrawsSession {route[7:]}", rounds=a.rounds, **dev,
                                       all_cold_ms=[round(r["cold_ms"], 2) for r in runs[route]],
                                       twin_over_cold=twin["per_series_ms"] * series / dev["cold_ms"],
                                       twin_over_warm=twin["per_series_ms"] * series / dev["warm_ms"])))
        for l in lines[-3:]:
          print(l, flush=True)
  if "e2e" in a.legs.split(","):
    if not a.baseline_root:
      raise SystemExit("the e2e legs need --baseline-root DIR, a built checkout of the parent commit")
    for case, series, rounds in (("float64 fit", 1, a.rounds), ("hmc batch", 64, a.e2e_batch_rounds or a.rounds)):
      runs = {"parent": [], "branch": []}
      for _ in range(rounds):                                 # parent and branch alternating
        for tree, root in (("parent", a.baseline_root), ("branch", ROOT)):
          runs[tree].append(child(["--child", "e2e", "--case", case, "--series", series] + common, root))
      for tree in runs:
        med = median_of(runs[tree], ("analytic_call_ms", "simulated_call_ms", "total_ms"))
        lines.append(json.dumps(dict(leg=f"end to end, {case}", tree=tree, series=series, steps=a.steps,
                                     covariates=a.covariates, draws=a.draws, rounds=rounds, **med,
                                     all_total_ms=[round(r["total_ms"], 1) for r in runs[tree]],
                                     placebo_checksum=runs[tree][0]["placebo_checksum"])))
        print(lines[-1], flush=True)
  with open(a.out, "a" if os.path.exists(a.out) and len(a.legs.split(",")) == 1 else "w", encoding="utf-8") as f:
    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
