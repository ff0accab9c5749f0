"""What `outcome_link=` costs a batch: `fit_causalimpact_batch` at the shape of BASELINE cfg5 (512
series, T = 500, 5 covariates, 1 chain x 1000 draws, positive outcomes) with the option None and
"log" in interleaved rounds after one warm-up of each; the device calls alone on a finished session
of the whole batch -- `Session.summarize` under the identity and under the log link, and
`Session.value_mean` -- with the largest gap of the device's exp to numpy's in ulp; and the
alternative the link replaces: the trajectories of a share of the batch (64 series) downloaded,
exponentiated and summarised in numpy, scaled to the batch by the series count.

`--leg stock`: `Session.summarize` with no link set at the same shape, for the comparison of a commit
with its parent (the only leg that runs on a tree without the option).

Prints one JSON line per leg: wall-clock ms of every run, their median and their spread
(max - min).  One leg per process, every process that uses the GPU under a time limit of its own,
a later leg only after the one before it has ended well:

  timeout -k 10 300 python tools/exp_outcome_link.py --leg batch && \\
  timeout -k 10 120 python tools/exp_outcome_link.py --leg device && \\
  timeout -k 10 300 python tools/exp_outcome_link.py --leg host

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


def timed(fn):
  t0 = time.perf_counter()
  fn()
  return (time.perf_counter() - t0) * 1e3


def positive_values(B, T, p):
  """[B, T, 1 + p]: the synthetic series of bench.py's cfg5 with the outcome as exp of its z-score * 0.3
  + 4 (positive, a multiplicative effect in the post-period)."""
  values = np.stack([np.column_stack(syn.make_raw_series(T, p, b)) for b in range(B)])
  y = values[:, :, 0]
  z = (y - y.mean(axis=1, keepdims=True)) / y.std(axis=1, keepdims=True)
  values[:, :, 0] = np.exp(0.3 * z + 4.0)
  return values


def open_session(values, index, pre, post, draws, count, logged):
  """A finished session of the first `count` series (the outcome logged first: the model of
  `outcome_link="log"`), and their prepared batch."""
  values = values[:count].copy()
  if logged:
    values[:, :, 0] = np.log(values[:, :, 0])
  prep = batch.prepare_batch(values, index, pre, post)
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
  ap.add_argument("--leg", choices=("batch", "device", "host", "stock"), required=True)
  ap.add_argument("--series", type=int, default=512)
  ap.add_argument("--steps", type=int, default=500)
  ap.add_argument("--covariates", type=int, default=5)
  ap.add_argument("--draws", type=int, default=1000)
  ap.add_argument("--runs", type=int, default=5)
  ap.add_argument("--share", type=int, default=64)
  a = ap.parse_args()
  B, T = a.series, a.steps
  values = positive_values(B, T, a.covariates)
  index = pd.RangeIndex(T)
  n_pre = int(0.7 * T)
  pre, post = (0, n_pre - 1), (n_pre, T - 1)
  shape = dict(series=B, steps=T, covariates=a.covariates, draws=a.draws)
  ranks = lib._summary_ranks(a.draws, (0.025, 0.975))   # pylint: disable=protected-access

  if a.leg == "batch":
    opts = ci.InferenceOptions(num_results=a.draws)
    fit = lambda link: ci.fit_causalimpact_batch(values, pre, post, index=index, seed=1,   # pylint: disable=unnecessary-lambda-assignment
                                                 inference_options=opts, outcome_link=link)
    for link in (None, "log"):
      fit(link)
    times = {None: [], "log": []}
    for _ in range(a.runs):                       # interleaved rounds
      for link in (None, "log"):
        times[link].append(timed(lambda link=link: fit(link)))
    report("batch outcome_link=None", times[None], **shape)
    report("batch outcome_link='log'", times["log"], **shape)
    return

  if a.leg in ("device", "stock"):
    sess, prep = open_session(values, index, pre, post, a.draws, B, logged=a.leg == "device")
    observed = np.exp(prep.observed) if a.leg == "device" else prep.observed
    args = (prep.outcome_sd, prep.outcome_mean, observed, prep.flags, ranks)
    try:
      if a.leg == "stock":
        sess.summarize(*args)
        report("Session.summarize, no link set", [timed(lambda: sess.summarize(*args)) for _ in range(a.runs)],
               **shape)
        return
      times = {"identity": [], "log": [], "value_mean": []}
      for link in (_native.LINK_IDENTITY, _native.LINK_LOG):       # warm-up: the scratch, the pinned blocks
        sess.set_link(link)
        sess.summarize(*args)
      sess.value_mean(prep.outcome_sd, prep.outcome_mean)
      for _ in range(a.runs):                     # interleaved rounds
        sess.set_link(_native.LINK_IDENTITY)
        times["identity"].append(timed(lambda: sess.summarize(*args)))
        sess.set_link(_native.LINK_LOG)
        times["log"].append(timed(lambda: sess.summarize(*args)))
        times["value_mean"].append(timed(lambda: sess.value_mean(prep.outcome_sd, prep.outcome_mean)))
      report("Session.summarize, identity", times["identity"], **shape)
      report("Session.summarize, log link", times["log"], **shape)
      report("Session.value_mean, log link", times["value_mean"], **shape)
      # the device's exp against numpy's on a share of the values (singleton pools)
      gaps = {}
      for name, link in (("log", _native.LINK_LOG), ("log1p", _native.LINK_LOG1P)):
        sess.set_link(link)
        worst, n = 0.0, min(B, 8)
        traj = sess.fetch(["posterior_trajectories"])["posterior_trajectories"][:n].reshape(n, a.draws, -1)
        for b in range(n):
          group = [{b: 1.0}]
          got = sess.pool_trajectories(prep.outcome_sd, prep.outcome_mean, group)[0]
          z = traj[b].astype(np.float64) * prep.outcome_sd[b] + prep.outcome_mean[b]
          want = _native.link_values_host(z, link)
          worst = max(worst, float((np.abs(got - want) / np.spacing(np.abs(want))).max()))
        gaps[name] = worst
      print(json.dumps(dict(leg="device exp / expm1 against numpy, largest gap in ulp",
                            values_per_link=int(min(B, 8) * a.draws * prep.y.shape[1]), **gaps, **shape)), flush=True)
    finally:
      sess.close()
    return

  # host: the share's trajectories downloaded, exponentiated and summarised in numpy
  sess, prep = open_session(values, index, pre, post, a.draws, a.share, logged=True)
  try:
    def host():
      traj = sess.fetch(["posterior_trajectories"])["posterior_trajectories"].reshape(a.share, a.draws, -1)
      v = np.exp(traj.astype(np.float64) * prep.outcome_sd[:, None, None] + prep.outcome_mean[:, None, None])
      mean = v.mean(axis=1)
      bands = np.quantile(v, (0.025, 0.975), axis=1)
      win = (prep.flags & 2) != 0
      totals = v[:, :, win].sum(axis=2)
      point = np.exp(prep.observed)[:, None, :] - v
      cum = np.nancumsum(np.where((prep.flags & 1)[None, None, :] != 0, point, 0.0), axis=2)
      return mean, bands, np.quantile(totals, (0.025, 0.975), axis=1), np.quantile(cum, (0.025, 0.975), axis=1)
    host()
    times = [timed(host) for _ in range(a.runs)]
    report(f"download + numpy, {a.share} series", times, **dict(shape, series=a.share),
           scaled_to_batch_ms=statistics.median(times) * B / a.share)
  finally:
    sess.close()


if __name__ == "__main__":
  main()
