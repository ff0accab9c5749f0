"""What `prediction_errors=True` and `placebo=` cost a batch whose model the one-lane filters do not
take, now that the block-model filters (csrc/ci_predict_blocks.h, ci_placebo_blocks.h) run them on
the device: `fit_causalimpact_batch` of 64 series, T = 500, 5 covariates, 1 chain x 1000 draws, for
  weekly+monthly   ModelOptions(seasons=[Seasons(7), Seasons(4, num_steps_per_season=7)])     d = 10
  seasons52        ModelOptions(local_linear_trend=True, seasons=[Seasons(52)])               d = 53
with each option off and on, interleaved over `--runs` rounds after one warm-up of each; the device
calls alone (`Session.summarize_predictions_blocks`, `summarize_placebo_blocks` on a finished session
of the whole batch); and, on a share of the batch, the device calls against the alternative they
replace -- the share's parameter draws downloaded and filtered with numpy
(`causalimpact_lib._prediction_summary_host`, `_placebo_summary_host`), both at the same shape.
`--twin-origins` caps the origins of the share's placebo legs (device and numpy alike): the numpy
recursion at d = 53 takes minutes per series.

Prints one JSON line per leg: wall-clock ms of every run, their median and their spread (max - min).

  python tools/exp_block_predictions.py [--series 64] [--steps 500] [--covariates 5] [--draws 1000]
      [--runs 5] [--share 8] [--twin-origins 0] [--models weekly+monthly,seasons52]
      [--out profiles/block_predictions.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tfp-causalimpact_amd")):
  if p not in sys.path:
    sys.path.insert(0, p)

import numpy as np  # pylint: disable=wrong-import-position
import pandas as pd  # pylint: disable=wrong-import-position

import causalimpact as ci  # pylint: disable=wrong-import-position
from causalimpact import _model, _native, batch  # pylint: disable=wrong-import-position
from causalimpact import _synthetic as syn  # pylint: disable=wrong-import-position
from causalimpact import causalimpact_lib as lib  # pylint: disable=wrong-import-position

DRAWS = ("observation_noise_scale", "level_scale", "slope_scale", "seasonal_drift_scales", "weights")
MODELS = {
    "weekly+monthly": dict(local_linear_trend=False, seasons=[ci.Seasons(7), ci.Seasons(4, num_steps_per_season=7)]),
    "seasons52": dict(local_linear_trend=True, seasons=[ci.Seasons(52)]),
}
LINES = []


def report(leg, times, **extra):
  LINES.append(json.dumps(dict(leg=leg, median_ms=statistics.median(times), spread_ms=max(times) - min(times),
                               all_ms=[round(t, 2) for t in times], **extra)))
  print(LINES[-1], flush=True)


def timed(fn, runs):
  times = []
  for _ in range(runs):
    t0 = time.perf_counter()
    fn()
    times.append((time.perf_counter() - t0) * 1e3)
  return times


def session_legs(model, values, index, pre, post, draws, count, runs, twin_origins, host):
  """A finished session of the first `count` series.  {leg: times}: the two device calls `runs` times
  each and, with `host`, the download of the parameter draws and the numpy filters from them, once."""
  mo = MODELS[model]
  prep = batch.prepare_batch(values[:count], index, pre, post)
  T, P = prep.y.shape[1], prep.design.shape[2]
  num_seasons, sc = _model.expand_seasons(mo["seasons"], T)
  hs = mo["local_linear_trend"]
  d = lib.prediction_state_dim(hs, num_seasons)
  params = [_model.series_params(prep.y[b], prep.mask[b], prep.design[b], has_slope=hs,
                                 num_seasonal_blocks=len(num_seasons),
                                 outcome_sd=float(np.nanstd(prep.y[b, :prep.num_pre], ddof=1)))
            for b in range(count)]
  origins, horizon = batch.placebo_plans(lib.Placebo(), [prep.num_pre] * count,
                                         [int(np.count_nonzero(prep.flags & 2))] * count, d)
  if twin_origins:
    origins = np.ascontiguousarray(origins[:, :twin_origins])
  ranks = [25, 500, 974] if draws == 1000 else [0, draws // 2, draws - 1]
  pb = _native.make_problem(T=T, P=P, has_slope=hs, num_warmup=-(-draws // 9), num_results=draws,
                            num_series=count, seed=(0, 1), num_seasons=num_seasons)
  sess = _native.Session(pb, prep.y, prep.mask, prep.design, sc, _native.make_params(params))
  out = {}
  try:
    sess.run()
    pred = lambda: sess.summarize_predictions_blocks(prep.outcome_sd, prep.outcome_mean, ranks)
    plac = lambda: sess.summarize_placebo_blocks(prep.outcome_sd, prep.outcome_mean, origins, horizon)
    pred(), plac()                                          # warm-up: the scratch
    out["device_predictions"] = timed(pred, runs)
    out["device_placebo"] = timed(plac, runs)
    plan = dict(state=d, origins=int(origins.shape[1]), horizon=int(horizon[0]), kernel=sess.kernel_name())
    if host:
      t0 = time.perf_counter()
      got = sess.fetch(list(DRAWS))
      out["numpy_fetch"] = [(time.perf_counter() - t0) * 1e3]
      y32, X32 = np.where(prep.mask, 0.0, prep.y).astype(np.float32), prep.design.astype(np.float32)
      own = lambda b: (y32[b], prep.mask[b], X32[b], sc, num_seasons, hs, params[b],
                       {k: got[k][b, 0] for k in DRAWS}, prep.outcome_sd[b], prep.outcome_mean[b])
      out["numpy_predictions"] = timed(
          lambda: [lib._prediction_summary_host(*own(b), ranks) for b in range(count)], 1)   # pylint: disable=protected-access
      print(json.dumps(dict(progress=f"{model}: numpy predictions done")), flush=True)
      out["numpy_placebo"] = timed(
          lambda: [lib._placebo_summary_host(*own(b), origins[b], horizon[b]) for b in range(count)], 1)   # pylint: disable=protected-access
    return out, plan
  finally:
    sess.close()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--series", type=int, default=64)
  ap.add_argument("--steps", type=int, default=500)
  ap.add_argument("--covariates", type=int, default=5)
  ap.add_argument("--draws", type=int, default=1000)
  ap.add_argument("--runs", type=int, default=5)
  ap.add_argument("--share", type=int, default=8)
  ap.add_argument("--twin-origins", type=int, default=0, help="cap on the origins of the share's placebo legs (0: all)")
  ap.add_argument("--models", default=",".join(MODELS))
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_predictions.jsonl"))
  a = ap.parse_args()
  B, T = a.series, a.steps
  values = np.stack([np.column_stack(syn.make_raw_series(T, a.covariates, b)) for b in range(B)])
  index = pd.RangeIndex(T)
  pre, post = (0, int(0.7 * T) - 1), (int(0.7 * T), T - 1)
  for model in a.models.split(","):
    mo = ci.ModelOptions(**MODELS[model])

    def fit(errors, placebo):
      return ci.fit_causalimpact_batch(
          values, pre, post, seed=1, index=index, placebo=True if placebo else None, model_options=mo,
          inference_options=ci.InferenceOptions(num_results=a.draws, prediction_errors=errors))

    fit(False, False), fit(True, False), fit(False, True)     # warm-up: library load, scratch, pools
    off, errors, placebo = [], [], []
    for _ in range(a.runs):                                   # interleaved: drift hits all alike
      off += timed(lambda: fit(False, False), 1)
      errors += timed(lambda: fit(True, False), 1)
      placebo += timed(lambda: fit(False, True), 1)
    shape = dict(model=model, series=B, steps=T, covariates=a.covariates, draws=a.draws)
    report("batch_off", off, **shape)
    report("batch_prediction_errors", errors, **shape)
    report("batch_placebo", placebo, **shape)
    legs, plan = session_legs(model, values, index, pre, post, a.draws, B, a.runs, 0, False)
    for leg, times in legs.items():
      report(leg, times, **shape, **plan)
    share = min(a.share, B)
    legs, plan = session_legs(model, values, index, pre, post, a.draws, share, a.runs, a.twin_origins, True)
    for leg, times in legs.items():
      report("share_" + leg, times, **dict(shape, series=share), **plan)
    with open(a.out, "w", encoding="utf-8") as f:
      f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
  main()
