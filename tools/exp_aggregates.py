"""What `fit_causalimpact_batch(aggregates=...)` costs a batch at the shape of BASELINE cfg5 (512
series, T = 500, 5 covariates, 1 chain x 1000 draws): the call with the argument off, with one group
of all series, and with a partition into 8 groups, in interleaved runs after one warm-up of each;
the pool step alone on a session that holds the batch (csrc/ci_pool.h), its bytes per second against
the bytes it must read; and the only alternative a user has without it -- the trajectories of a
share of the batch (64 series) downloaded and added up in numpy, scaled to the batch by the series
count.

The pool call has no timer of its own.  Its kernel is isolated by difference: one group of all B
series against one group of one series move the same [N, T] float64 result to the host and differ
by the (B - 1) * N * T * 4 bytes of trajectories the kernel reads.  No event-timed figure is
available: the difference of two wall-clock medians also carries the larger weight table's upload
(B entries of 32 bytes) and the noise of the result copies, so it is a lower bound on the kernel's
rate, reported as null when the difference is not positive.

Prints one JSON line per leg: wall-clock ms of every run, their median and their spread (max - min).

  python tools/exp_aggregates.py [--series 512] [--steps 500] [--covariates 5] [--draws 1000]
                                 [--runs 5] [--share 64]
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


def report(leg, times, **extra):
  print(json.dumps(dict(leg=leg, median_ms=statistics.median(times), spread_ms=max(times) - min(times),
                        all_ms=[round(t, 2) for t in times], **extra)), flush=True)


def session_of(values, index, pre, post, draws, count):
  """A finished session of the first `count` series, as the batch path runs them."""
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


def pool_alone(values, index, pre, post, draws, runs):
  """The pool step on a resident batch: all series in one group, in 8 groups, and one series."""
  B = values.shape[0]
  sess, prep = session_of(values, index, pre, post, draws, B)
  legs = {"pool_one_group": [list(range(B))],
          "pool_8_groups": [list(range(g, B, 8)) for g in range(8)] if B >= 8 else [list(range(B))],
          "pool_one_series": [[0]]}
  times = {k: [] for k in legs}
  try:
    sess.summarize(prep.outcome_sd, prep.outcome_mean, prep.observed, prep.flags, [0])   # the scratch
    for groups in legs.values():
      sess.pool_trajectories(prep.outcome_sd, prep.outcome_mean, groups)                 # warm-up
    for _ in range(runs):
      for leg, groups in legs.items():
        t0 = time.perf_counter()
        sess.pool_trajectories(prep.outcome_sd, prep.outcome_mean, groups)
        times[leg].append((time.perf_counter() - t0) * 1e3)
  finally:
    sess.close()
  NT = draws * prep.y.shape[1]
  read = B * NT * 4
  for leg, t in times.items():
    groups = len(legs[leg])
    report(leg, t, series=B, groups=groups, result_bytes=groups * NT * 8,
           trajectory_bytes=(read if leg != "pool_one_series" else NT * 4))
  kernel_ms = statistics.median(times["pool_one_group"]) - statistics.median(times["pool_one_series"])
  print(json.dumps(dict(leg="pool_kernel_by_difference", ms=kernel_ms, bytes=(B - 1) * NT * 4,
                        gb_per_s=((B - 1) * NT * 4 / (kernel_ms * 1e-3) / 1e9 if kernel_ms > 0 else None),
                        note="one group of all series minus one group of one series: same result "
                             "traffic, (B - 1) series of float32 trajectories more to read")), flush=True)


def host_share(values, index, pre, post, draws, share):
  """Download the trajectories of `share` series and add them up in numpy."""
  sess, prep = session_of(values, index, pre, post, draws, share)
  try:
    t0 = time.perf_counter()
    traj = sess.fetch(["posterior_trajectories"])["posterior_trajectories"]
    t1 = time.perf_counter()
    _native.pool_host(traj.reshape(share, draws, -1), prep.outcome_sd, prep.outcome_mean,
                      [list(range(share))])
    t2 = time.perf_counter()
  finally:
    sess.close()
  return (t1 - t0) * 1e3, (t2 - t1) * 1e3


def main():
  ap = argparse.ArgumentParser()
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
  pre, post = (0, int(0.7 * T) - 1), (int(0.7 * T), T - 1)
  legs = {"aggregates_off": None, "aggregates_all": {"all": "all"},
          "aggregates_8_groups": {f"g{g}": list(range(g, B, 8)) for g in range(min(8, B))}}

  def fit(aggregates):
    return ci.fit_causalimpact_batch(values, pre, post, seed=1, index=index, aggregates=aggregates,
                                     inference_options=ci.InferenceOptions(num_results=a.draws))

  for aggregates in legs.values():                          # warm-up: library load, scratch, pools
    fit(aggregates)
  times = {k: [] for k in legs}
  for _ in range(a.runs):                                   # interleaved: drift hits all alike
    for leg, aggregates in legs.items():
      t0 = time.perf_counter()
      fit(aggregates)
      times[leg].append((time.perf_counter() - t0) * 1e3)
  shape = dict(series=B, steps=T, covariates=a.covariates, draws=a.draws)
  for leg, t in times.items():
    report(leg, t, **shape)
  pool_alone(values, index, pre, post, a.draws, a.runs)
  share = min(a.share, B)
  fetch, add = zip(*[host_share(values, index, pre, post, a.draws, share) for _ in range(3)])
  report("numpy_share_fetch", list(fetch), series=share)
  report("numpy_share_add", list(add), series=share,
         scaled_to_batch_ms=statistics.median(add) * B / share)


if __name__ == "__main__":
  main()
