"""What `joint_bands=True` costs a batch: `fit_causalimpact_batch` at the shape of BASELINE cfg5 (512
series, T = 500, 5 covariates, 1 chain x 1000 draws), the option off and on in interleaved runs after
one warm-up of each; the device call alone (`Session.summarize_paths` on a finished session of the
whole batch, the post-period as its one window) with the bytes of the window's columns it reads per
second and the number of chunks it took; and the alternative it replaces -- the trajectories of a
share of the batch (64 series) downloaded and taken through `_native.path_excursions_host`, scaled to
the batch by the series count.

Prints one JSON line per leg: wall-clock ms of every run, their median and their spread
(max - min).  One leg per process, every process that uses the GPU under a time limit of its own,
a later leg only after the one before it has ended well:

  timeout -k 10 300 python tools/exp_joint_bands.py --leg batch && \\
  timeout -k 10 120 python tools/exp_joint_bands.py --leg device && \\
  timeout -k 10 300 python tools/exp_joint_bands.py --leg host

  [--series 512] [--steps 500] [--covariates 5] [--draws 1000] [--runs 5] [--share 64]
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


def report(leg, times, **extra):
  print(json.dumps(dict(leg=leg, median_ms=statistics.median(times), spread_ms=max(times) - min(times),
                        all_ms=[round(t, 2) for t in times], **extra)), flush=True)


def timed(fn, runs):
  times = []
  for _ in range(runs):
    t0 = time.perf_counter()
    fn()
    times.append((time.perf_counter() - t0) * 1e3)
  return times


def open_session(values, index, pre, post, draws, count):
  """A finished session of the first `count` series, and their prepared batch."""
  prep = batch.prepare_batch(values[:count], index, pre, post)
  T, P = prep.y.shape[1], prep.design.shape[2]
  params = [_model.series_params(prep.y[b], prep.mask[b], prep.design[b],
                                 outcome_sd=float(np.nanstd(prep.y[b, :prep.num_pre], ddof=1)))
            for b in range(count)]
  pb = _native.make_problem(T=T, P=P, has_slope=False, num_warmup=-(-draws // 9), num_results=draws,
                            num_series=count, seed=(0, 1))
  sess = _native.Session(pb, prep.y, prep.mask, prep.design, None, _native.make_params(params))
  sess.run()
  return sess, prep


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--leg", choices=("batch", "device", "host"), required=True)
  ap.add_argument("--series", type=int, default=512)
  ap.add_argument("--steps", type=int, default=500)
  ap.add_argument("--covariates", type=int, default=5)
  ap.add_argument("--draws", type=int, default=1000)
  ap.add_argument("--runs", type=int, default=5)
  ap.add_argument("--share", type=int, default=64)
  a = ap.parse_args()
  B, T = a.series, a.steps
  values = np.stack([np.column_stack(syn.make_raw_series(T, a.covariates, b)) for b in range(B)])
  index = pd.RangeIndex(T)
  start = int(0.7 * T)
  pre, post = (0, start - 1), (start, T - 1)
  first, count = np.array([start]), np.array([T - start])   # the post-period
  shape = dict(series=B, steps=T, covariates=a.covariates, draws=a.draws, window_steps=T - start)
  ranks = lib._path_ranks(a.draws, 0.05)                    # pylint: disable=protected-access

  if a.leg == "batch":
    def fit(on):
      return ci.fit_causalimpact_batch(values, pre, post, seed=1, index=index,
                                       inference_options=ci.InferenceOptions(num_results=a.draws),
                                       joint_bands=on)
    fit(False), fit(True)                                   # warm-up: library load, scratch, pools
    off, on = [], []
    for _ in range(a.runs):                                 # interleaved: drift hits both alike
      off += timed(lambda: fit(False), 1)
      on += timed(lambda: fit(True), 1)
    report("joint_bands_off", off, **shape)
    report("joint_bands_on", on, **shape)
    return

  n = B if a.leg != "host" else min(a.share, B)
  sess, prep = open_session(values, index, pre, post, a.draws, n)
  try:
    if a.leg == "device":
      want = lib._PATH_RECORD                               # pylint: disable=protected-access
      call = lambda: sess.summarize_paths(prep.outcome_sd, prep.outcome_mean, prep.observed, first, count, ranks,
                                          want=want)
      call()                                                # warm-up: the pools
      times = timed(call, a.runs)
      read = n * a.draws * int(count.sum()) * 4             # the float32 columns inside the window
      chunks = sess.summarize_paths(prep.outcome_sd, prep.outcome_mean, prep.observed, first, count, ranks,
                                    want=("exceed",), max_bytes=1 << 30)["num_chunks"]
      report("device_call", times, note="Session.summarize_paths: what the record keeps, downloaded",
             window_bytes=read, gb_per_s=read / (statistics.median(times) * 1e-3) / 1e9, chunks=chunks, **shape)
      everything = lambda: sess.summarize_paths(prep.outcome_sd, prep.outcome_mean, prep.observed, first, count,
                                                ranks)
      report("device_call_with_excursions", timed(everything, a.runs),
             note="the same with every draw's excursions downloaded too", **shape)
    else:
      t0 = time.perf_counter()
      traj = sess.fetch(["posterior_trajectories"])["posterior_trajectories"]
      t1 = time.perf_counter()
      traj = traj.reshape(n, -1, traj.shape[-1])
      for b in range(n):                                    # (series by series: the paths it returns are large)
        _native.path_excursions_host(traj[b:b + 1], prep.outcome_sd[b], prep.outcome_mean[b], prep.observed[b],
                                     first, count, ranks=ranks)
      t2 = time.perf_counter()
      report("numpy_share_fetch", [(t1 - t0) * 1e3], series=n)
      report("numpy_share_excursions", [(t2 - t1) * 1e3], series=n, scaled_to_batch_ms=(t2 - t1) * 1e3 * B / n)
  finally:
    sess.close()


if __name__ == "__main__":
  main()
