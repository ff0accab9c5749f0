"""One-launch HMC batch vs the series-by-series route on cfg5's shape: 512 series, T = 500, 5
covariates, 1 chain, 15 leapfrog steps, W = 500, S = 1000.

The one-launch time is measured on the whole batch (`fit_causalimpact_batch(sampler="hmc")`, host
preparation and summary included).  The series-by-series time is NOT measured on all 512 series:
`fit_causalimpact(sampler="hmc")` is timed on a sample of series and the mean is scaled by 512; the
output says so.

  python tools/exp_hmc_batch.py [--sample 4] [--out profiles/r08_exp_hmc_batch.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tfp-causalimpact_amd")]

import pandas as pd  # noqa: E402

import causalimpact as ci  # noqa: E402
from causalimpact import _synthetic as syn  # noqa: E402

B, T, P, PRE, W, S, NL = 512, 500, 5, 350, 500, 1000, 15


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--sample", type=int, default=4, help="series timed on the series-by-series route")
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  values = np.stack([np.column_stack(syn.make_raw_series(T, P, 100 + b, effect=3.0)) for b in range(B)])
  opts = ci.InferenceOptions(num_results=S, num_warmup_steps=W, num_chains=1, sampler="hmc")
  pre, post = (0, PRE - 1), (PRE, T - 1)
  # warm-up: library load, device initialisation, kernel loading
  ci.fit_causalimpact_batch(values[:2], pre, post, seed=1, inference_options=ci.InferenceOptions(
      num_results=10, num_warmup_steps=10, sampler="hmc"))
  t0 = time.perf_counter()
  got = ci.fit_causalimpact_batch(values, pre, post, seed=1, inference_options=opts)
  one_launch_s = time.perf_counter() - t0
  assert np.isfinite(got.summary.drop(columns=["p_value", "alpha"]).to_numpy(float)).all()
  cols = ["y"] + [f"x{j}" for j in range(P)]
  times = []
  for b in range(args.sample):
    df = pd.DataFrame(values[b], columns=cols)
    t0 = time.perf_counter()
    ci.fit_causalimpact(df, pre, post, seed=1, inference_options=opts)
    times.append(time.perf_counter() - t0)
  per_series_s = float(np.mean(times))
  res = dict(
      shape=dict(num_series=B, T=T, covariates=P, chains=1, leapfrog=NL, num_warmup=W, num_results=S),
      one_launch_s=round(one_launch_s, 4),
      series_by_series_s_estimated=round(per_series_s * B, 2),
      series_by_series_note=(f"estimated: fit_causalimpact(sampler='hmc') timed on {args.sample} of the "
                             f"{B} series (mean {per_series_s:.4f} s, each {[round(t, 4) for t in times]}) "
                             f"and scaled by {B}; not measured on every series"),
      speedup_estimated=round(per_series_s * B / one_launch_s, 1))
  line = json.dumps(res)
  print(line)
  if args.out:
    with open(args.out, "w") as f:
      f.write(line + "\n")


if __name__ == "__main__":
  main()
