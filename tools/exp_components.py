"""What `InferenceOptions(components=True)` costs a batch: `fit_causalimpact_batch` at the shape of
BASELINE cfg5 (512 series, T = 500, 5 covariates, 1 chain x 1000 draws) with the option off and on,
in interleaved runs after one warm-up of each, and the alternative the option replaces -- the draws
of a share of the batch (64 series) downloaded and reduced with numpy
(`causalimpact_lib._component_summary_host`), scaled to the batch by the series count.

Prints one JSON line per leg: wall-clock ms of every run, their median and their spread
(max - min).  "on_frames" also builds every series' two frames (they are assembled on indexing).

  python tools/exp_components.py [--series 512] [--steps 500] [--covariates 5] [--draws 1000]
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
from causalimpact import causalimpact_lib as lib  # pylint: disable=wrong-import-position


def report(leg, times, **extra):
  print(json.dumps(dict(leg=leg, median_ms=statistics.median(times), spread_ms=max(times) - min(times),
                        all_ms=[round(t, 2) for t in times], **extra)), flush=True)


def host_share(values, index, pre, post, draws, share):
  """Download the draws of `share` series and reduce them in numpy: what a user of the batch path
  would have to do without the option (and with a session of their own: the batch keeps no draws)."""
  prep = batch.prepare_batch(values[:share], index, pre, post)
  T, P = prep.y.shape[1], prep.design.shape[2]
  params = [_model.series_params(prep.y[b], prep.mask[b], prep.design[b],
                                 outcome_sd=float(np.nanstd(prep.y[b, :prep.num_pre], ddof=1)))
            for b in range(share)]
  pb = _native.make_problem(T=T, P=P, has_slope=False, num_warmup=-(-draws // 9), num_results=draws,
                            num_series=share, seed=(0, 1))
  sess = _native.Session(pb, prep.y, prep.mask, prep.design, None, _native.make_params(params))
  try:
    sess.run()
    ranks = lib._summary_ranks(draws, (0.025, 0.975))   # pylint: disable=protected-access
    t0 = time.perf_counter()
    out = sess.fetch(["level", "weights", "seasonal_levels"])
    t1 = time.perf_counter()
    X = prep.design.astype(np.float32)
    for b in range(share):
      lib._component_summary_host(out["level"][b, 0], out["seasonal_levels"][b, 0],   # pylint: disable=protected-access
                                  out["weights"][b, 0], X[b], prep.outcome_sd[b], prep.outcome_mean[b],
                                  ranks)
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

  def fit(components):
    return ci.fit_causalimpact_batch(
        values, pre, post, seed=1, index=index,
        inference_options=ci.InferenceOptions(num_results=a.draws, components=components))

  fit(False), fit(True)                                     # warm-up: library load, scratch, pools
  off, on, frames = [], [], []
  for _ in range(a.runs):                                   # interleaved: drift hits both alike
    t0 = time.perf_counter()
    fit(False)
    t1 = time.perf_counter()
    res = fit(True)
    t2 = time.perf_counter()
    for b in range(B):
      _ = res[b].components, res[b].coefficients
    t3 = time.perf_counter()
    off.append((t1 - t0) * 1e3)
    on.append((t2 - t1) * 1e3)
    frames.append((t3 - t2) * 1e3)
  shape = dict(series=B, steps=T, covariates=a.covariates, draws=a.draws)
  report("components_off", off, **shape)
  report("components_on", on, **shape)
  report("on_frames", frames, note="all per-series analyses built on indexing (series frames included)", **shape)
  share = min(a.share, B)
  fetch, reduce_ = zip(*[host_share(values, index, pre, post, a.draws, share) for _ in range(3)])
  report("numpy_share_fetch", list(fetch), series=share)
  report("numpy_share_reduce", list(reduce_), series=share,
         scaled_to_batch_ms=statistics.median(reduce_) * B / share)


if __name__ == "__main__":
  main()
