"""What `fit_causalimpact_panel(event_aggregates=...)` costs a panel at the shape of
tools/exp_panel.py (512 series, 5 covariates, lengths uniform in 257..512 -- one steps-per-thread
class --, own periods, 1 chain x 1000 draws): the call with the argument off and with one group of
all series, in interleaved runs after one warm-up of each; the pool step alone on a ragged session
that holds the panel (csrc/ci_pool.h), one group of all series against one group of one
series; and the alternative the feature replaces -- the trajectories of a share of the panel (64
series) downloaded and their shifted windows added up in numpy, scaled to the panel by the series
count.

The pool call has no timer of its own.  Its kernel is isolated by difference, as in
tools/exp_aggregates.py: one group of all B series against one group of one series of the same width
move the same [N, width] float64 result to the host and differ by the (B - 1) * N * width * 4 bytes
of trajectories the kernel reads.  The difference of two wall-clock medians also carries the larger
table's upload and the noise of the result copies: it is a lower bound on the kernel's rate, reported
as null when the difference is not positive.

Prints one JSON line per leg: wall-clock ms of every run, their median and their spread (max - min).

  python tools/exp_event_aggregates.py [--series 512] [--draws 1000] [--runs 5] [--share 64]
                                       [--min-length 257] [--max-length 512] [--covariates 5]
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
from causalimpact import _native, batch  # pylint: disable=wrong-import-position
from causalimpact import _synthetic as syn  # pylint: disable=wrong-import-position


def report(leg, times, **extra):
  print(json.dumps(dict(leg=leg, median_ms=statistics.median(times), spread_ms=max(times) - min(times),
                        all_ms=[round(t, 2) for t in times], **extra)), flush=True)


def data(a):
  """The panel of tools/exp_panel.py."""
  rng = np.random.default_rng(2024)
  lengths = rng.integers(a.min_length, a.max_length + 1, size=a.series)
  frames, periods = [], []
  for b, T in enumerate(int(t) for t in lengths):
    y, X = syn.make_raw_series(T, a.covariates, b)
    frames.append(pd.DataFrame(np.column_stack([y, X]), index=pd.RangeIndex(T),
                               columns=["y"] + [f"x{j}" for j in range(a.covariates)]))
    n_pre = int(0.7 * T)
    periods.append(((0, n_pre - 1), (n_pre, T - 1)))
  return frames, periods


def session_of(frames, periods, draws, count):
  """A finished ragged session of the first `count` series, as the panel path runs them, with the
  event-time group of all of them and of the first alone (the same width)."""
  prep = batch.prepare_panel(frames[:count], periods[:count])
  io = ci.InferenceOptions(num_results=draws)
  y = batch._sampler_outcome(prep, ci.DataOptions())                      # pylint: disable=protected-access
  with np.errstate(invalid="ignore"):
    pre_sd = [np.nanstd(y[b, :nb], ddof=1) for b, nb in enumerate(prep.num_pre)]
  fit = batch._new_fit(prep, y, prep.lengths, pre_sd, 0.05, (0, 1), ci.ModelOptions(), io, False)   # pylint: disable=protected-access
  T = int(prep.lengths.max())
  pb = _native.make_problem(T=T, P=prep.design.shape[2], has_slope=False, num_warmup=io.num_warmup_steps,
                            num_results=draws, num_series=count, seed=(0, 1))
  sess = _native.Session.ragged(pb, prep.lengths, fit.y, fit.mask, fit.design, _native.make_params(fit.params),
                                series_ids=np.arange(count))
  sess.run()
  _, csr = batch.aggregate_groups({"all": "all"}, list(range(count)))
  axis = batch.event_axes(prep, csr)[0]
  every = ({b: (1.0, int(f)) for b, f in enumerate(axis.first)}, axis.width)
  first = ({0: (1.0, int(axis.first[0]))}, axis.width)
  return sess, prep, every, first


def pool_alone(frames, periods, draws, runs):
  B = len(frames)
  sess, prep, every, first = session_of(frames, periods, draws, B)
  legs = {"pool_one_group": [every], "pool_one_series": [first]}
  times = {k: [] for k in legs}
  try:
    sess.summarize(prep.outcome_sd, prep.outcome_mean, prep.observed, prep.flags, [0])   # the scratch
    for groups in legs.values():
      sess.pool_event_trajectories(prep.outcome_sd, prep.outcome_mean, groups)           # warm-up
    for _ in range(runs):
      for leg, groups in legs.items():
        t0 = time.perf_counter()
        sess.pool_event_trajectories(prep.outcome_sd, prep.outcome_mean, groups)
        times[leg].append((time.perf_counter() - t0) * 1e3)
  finally:
    sess.close()
  NW = draws * every[1]
  for leg, t in times.items():
    report(leg, t, series=B, width=every[1], result_bytes=NW * 8,
           trajectory_bytes=(B if leg == "pool_one_group" else 1) * NW * 4)
  kernel_ms = statistics.median(times["pool_one_group"]) - statistics.median(times["pool_one_series"])
  print(json.dumps(dict(leg="pool_kernel_by_difference", ms=kernel_ms, bytes=(B - 1) * NW * 4,
                        gb_per_s=((B - 1) * NW * 4 / (kernel_ms * 1e-3) / 1e9 if kernel_ms > 0 else None),
                        note="one group of all series minus one group of one series: same result "
                             "traffic, (B - 1) windows of float32 trajectories more to read")), flush=True)


def host_share(frames, periods, draws, share):
  """Download the trajectories of `share` series and add their windows up in numpy."""
  sess, prep, every, _ = session_of(frames, periods, draws, share)
  try:
    t0 = time.perf_counter()
    traj = sess.fetch(["posterior_trajectories"])["posterior_trajectories"]
    t1 = time.perf_counter()
    _native.pool_event_host(traj.reshape(share, draws, -1), prep.outcome_sd, prep.outcome_mean, [every])
    t2 = time.perf_counter()
  finally:
    sess.close()
  return (t1 - t0) * 1e3, (t2 - t1) * 1e3


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--series", type=int, default=512)
  ap.add_argument("--draws", type=int, default=1000)
  ap.add_argument("--runs", type=int, default=5)
  ap.add_argument("--share", type=int, default=64)
  ap.add_argument("--min-length", type=int, default=257)
  ap.add_argument("--max-length", type=int, default=512)
  ap.add_argument("--covariates", type=int, default=5)
  a = ap.parse_args()
  frames, periods = data(a)
  legs = {"event_aggregates_off": None, "event_aggregates_all": {"all": "all"}}

  def fit(aggregates):
    return ci.fit_causalimpact_panel(frames, periods, seed=1, event_aggregates=aggregates,
                                     inference_options=ci.InferenceOptions(num_results=a.draws))

  for aggregates in legs.values():                          # warm-up: library load, scratch, pools
    fit(aggregates)
  times = {k: [] for k in legs}
  for _ in range(a.runs):                                   # interleaved: drift hits all alike
    for leg, aggregates in legs.items():
      t0 = time.perf_counter()
      fit(aggregates)
      times[leg].append((time.perf_counter() - t0) * 1e3)
  shape = dict(series=a.series, min_length=a.min_length, max_length=a.max_length,
               covariates=a.covariates, draws=a.draws)
  for leg, t in times.items():
    report(leg, t, **shape)
  pool_alone(frames, periods, a.draws, a.runs)
  share = min(a.share, a.series)
  fetch, add = zip(*[host_share(frames, periods, a.draws, share) for _ in range(3)])
  report("numpy_share_fetch", list(fetch), series=share)
  report("numpy_share_add", list(add), series=share,
         scaled_to_panel_ms=statistics.median(add) * a.series / share)


if __name__ == "__main__":
  main()
