"""What joint bands of the pooled aggregates cost: `fit_causalimpact_batch` at the shape of BASELINE
cfg5 (512 series, T = 500, 5 covariates, 1 chain x 1000 draws) with four aggregates (all series, two
halves, one weighted eighth).  Per round, interleaved so that drift hits every leg alike:

  the batch call with `aggregates`, `joint_bands` off and on;
  the new device call alone (`_native.summarize_draw_paths`, ci_summarize_draw_paths_f64) on the pooled
    draws [4, 1000, 500] float64 the batch call handed it, upload included, with the bytes of the
    draws it uploads per second;
  `_native.path_excursions_host`, the numpy loop it replaces for a pooled group, on the same draws.

Prints one JSON line per leg: wall-clock ms of every round, their median and their spread (max - min).
One process; run it under a time limit of its own:

  timeout -k 10 600 python tools/exp_aggregate_joint_bands.py

  [--series 512] [--steps 500] [--covariates 5] [--draws 1000] [--runs 5]
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
from causalimpact import _native  # pylint: disable=wrong-import-position
from causalimpact import _synthetic as syn  # pylint: disable=wrong-import-position


def report(leg, times, **extra):
  print(json.dumps(dict(leg=leg, median_ms=statistics.median(times), spread_ms=max(times) - min(times),
                        all_ms=[round(t, 2) for t in times], **extra)), flush=True)


def timed(fn):
  t0 = time.perf_counter()
  fn()
  return (time.perf_counter() - t0) * 1e3


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--series", type=int, default=512)
  ap.add_argument("--steps", type=int, default=500)
  ap.add_argument("--covariates", type=int, default=5)
  ap.add_argument("--draws", type=int, default=1000)
  ap.add_argument("--runs", type=int, default=5)
  a = ap.parse_args()
  B, T = a.series, a.steps
  values = np.stack([np.column_stack(syn.make_raw_series(T, a.covariates, b)) for b in range(B)])
  index = pd.RangeIndex(T)
  start = int(0.7 * T)
  pre, post = (0, start - 1), (start, T - 1)
  aggregates = {"all": "all", "first_half": list(range(B // 2)), "second_half": list(range(B // 2, B)),
                "eighth": {b: 0.5 + b % 3 for b in range(0, B, 8)}}
  shape = dict(series=B, steps=T, covariates=a.covariates, draws=a.draws, window_steps=T - start,
               groups=len(aggregates))

  def fit(on):
    return ci.fit_causalimpact_batch(values, pre, post, seed=1, index=index,
                                     inference_options=ci.InferenceOptions(num_results=a.draws),
                                     aggregates=aggregates, joint_bands=on)

  # warm-up of both (library load, scratch, pools); the call with the option on shows what the device
  # call is handed
  seen, real = [], _native.summarize_draw_paths

  def spy(*args, **kw):
    seen.append((args, kw))
    return real(*args, **kw)

  fit(False)
  _native.summarize_draw_paths = spy
  try:
    fit(True)
  finally:
    _native.summarize_draw_paths = real
  (args, kw), = seen
  draws, observed, first, count, ranks = args[0], args[3], args[4], args[5], args[6]
  assert draws.shape == (len(aggregates), a.draws, T) and draws.dtype == np.float64
  device = lambda: real(*args, **kw)                        # pylint: disable=unnecessary-lambda-assignment
  host = lambda: _native.path_excursions_host(draws, 1.0, 0.0, observed, first, count, ranks=ranks)   # pylint: disable=unnecessary-lambda-assignment
  device()
  off, on, dev, numpy_ = [], [], [], []
  for _ in range(a.runs):
    off.append(timed(lambda: fit(False)))
    on.append(timed(lambda: fit(True)))
    dev.append(timed(device))
    numpy_.append(timed(host))
  report("aggregates_joint_bands_off", off, **shape)
  report("aggregates_joint_bands_on", on, **shape)
  chunks = real(draws, 1.0, 0.0, observed, first, count, ranks, want=("exceed",), max_bytes=1 << 30)["num_chunks"]
  report("device_call", dev, note="summarize_draw_paths: upload of the pooled draws, four kernels, what the record keeps",
         uploaded_bytes=draws.nbytes, gb_per_s=draws.nbytes / (statistics.median(dev) * 1e-3) / 1e9, chunks=chunks,
         **shape)
  report("numpy_path_excursions_host", numpy_, note="the same pooled draws through the host loop", **shape)


if __name__ == "__main__":
  main()
