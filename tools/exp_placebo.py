"""What `placebo=` costs a batch: `fit_causalimpact_batch` at the shape of BASELINE cfg5 (512 series,
T = 500, 5 covariates, 1 chain x 1000 draws) with the option off and on (the default `Placebo()`:
32 origins, horizon min(n_post, n_pre // 3)), in interleaved runs after one warm-up of each; the
device call alone (`Session.summarize_placebo` on a finished session of the whole batch); and the
alternative the option replaces -- the parameter draws of a share of the batch (64 series)
downloaded and forecast with numpy (`causalimpact_lib._placebo_summary_host`), scaled to the batch
by the series count.

Prints one JSON line per leg: wall-clock ms of every run, their median and their spread
(max - min).  "on_quality" also builds the batch's `placebo_quality` table.

  python tools/exp_placebo.py [--series 512] [--steps 500] [--covariates 5] [--draws 1000]
                              [--runs 5] [--share 64] [--out profiles/placebo.jsonl]
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
LINES = []


def report(leg, times, **extra):
  LINES.append(json.dumps(dict(leg=leg, median_ms=statistics.median(times), spread_ms=max(times) - min(times),
                               all_ms=[round(t, 2) for t in times], **extra)))
  print(LINES[-1], flush=True)


def session_legs(values, index, pre, post, draws, count, runs, host):
  """A finished session of the first `count` series: the device call `runs` times (host=False), or
  the download of its parameter draws and the numpy forecasts from them, once (host=True)."""
  prep = batch.prepare_batch(values[:count], index, pre, post)
  T, P = prep.y.shape[1], prep.design.shape[2]
  params = [_model.series_params(prep.y[b], prep.mask[b], prep.design[b],
                                 outcome_sd=float(np.nanstd(prep.y[b, :prep.num_pre], ddof=1)))
            for b in range(count)]
  origins, horizon = batch.placebo_plans(lib.Placebo(), [prep.num_pre] * count,
                                         [int(np.count_nonzero(prep.flags & 2))] * count, 1)
  pb = _native.make_problem(T=T, P=P, has_slope=False, num_warmup=-(-draws // 9), num_results=draws,
                            num_series=count, seed=(0, 1))
  sess = _native.Session(pb, prep.y, prep.mask, prep.design, None, _native.make_params(params))
  try:
    sess.run()
    if not host:
      sess.summarize_placebo(prep.outcome_sd, prep.outcome_mean, origins, horizon)      # warm-up: the scratch
      times = []
      for _ in range(runs):
        t0 = time.perf_counter()
        sess.summarize_placebo(prep.outcome_sd, prep.outcome_mean, origins, horizon)
        times.append((time.perf_counter() - t0) * 1e3)
      return times, int(origins.shape[1]), int(horizon[0])
    t0 = time.perf_counter()
    out = sess.fetch(list(DRAWS))
    t1 = time.perf_counter()
    y32, X32 = np.where(prep.mask, 0.0, prep.y).astype(np.float32), prep.design.astype(np.float32)
    for b in range(count):
      lib._placebo_summary_host(                        # pylint: disable=protected-access
          y32[b], prep.mask[b], X32[b], np.zeros((0, T), np.uint8), [], False, params[b],
          {k: out[k][b, 0] for k in DRAWS}, prep.outcome_sd[b], prep.outcome_mean[b], origins[b], horizon[b])
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3
  finally:
    sess.close()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--series", type=int, default=512)
  ap.add_argument("--steps", type=int, default=500)
  ap.add_argument("--covariates", type=int, default=5)
  ap.add_argument("--draws", type=int, default=1000)
  ap.add_argument("--runs", type=int, default=5)
  ap.add_argument("--share", type=int, default=64)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "placebo.jsonl"))
  a = ap.parse_args()
  B, T = a.series, a.steps
  values = np.stack([np.column_stack(syn.make_raw_series(T, a.covariates, b)) for b in range(B)])
  index = pd.RangeIndex(T)
  pre, post = (0, int(0.7 * T) - 1), (int(0.7 * T), T - 1)

  def fit(on):
    return ci.fit_causalimpact_batch(values, pre, post, seed=1, index=index, placebo=True if on else None,
                                     inference_options=ci.InferenceOptions(num_results=a.draws))

  fit(False), fit(True)                                     # warm-up: library load, scratch, pools
  off, on, quality = [], [], []
  for _ in range(a.runs):                                   # interleaved: drift hits both alike
    t0 = time.perf_counter()
    fit(False)
    t1 = time.perf_counter()
    res = fit(True)
    t2 = time.perf_counter()
    _ = res.placebo_quality
    t3 = time.perf_counter()
    off.append((t1 - t0) * 1e3)
    on.append((t2 - t1) * 1e3)
    quality.append((t3 - t2) * 1e3)
  shape = dict(series=B, steps=T, covariates=a.covariates, draws=a.draws)
  report("placebo_off", off, **shape)
  report("placebo_on", on, **shape)
  report("on_quality", quality, note="the placebo_quality table of the batch, one row per series", **shape)
  times, num_origins, horizon = session_legs(values, index, pre, post, a.draws, B, a.runs, False)
  report("device_call", times, note="Session.summarize_placebo, all three outputs", origins=num_origins,
         horizon=horizon, **shape)
  share = min(a.share, B)
  fetch, forecast = session_legs(values, index, pre, post, a.draws, share, 1, True)
  report("numpy_share_fetch", [fetch], series=share)
  report("numpy_share_forecast", [forecast], series=share, scaled_to_batch_ms=forecast * B / share)
  with open(a.out, "w", encoding="utf-8") as f:
    f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
  main()
