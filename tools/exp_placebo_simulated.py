"""What `Placebo(simulate=True)` costs a batch under `outcome_link="log"`: `fit_causalimpact_batch` at
the shape of BASELINE cfg5 with positive outcomes (512 series, T = 500, 5 covariates, 1 chain x 1000
draws; 32 origins, horizon min(n_post, n_pre // 3)) with the option off and on, in interleaved rounds
after one warm-up of each; the device call alone (`Session.simulate_placebo`, one filter pass) against
`Session.summarize_placebo` (three passes) on the same finished session, interleaved; the numpy twin
(`causalimpact_lib._placebo_simulated_host`) on a share of the batch (64 series), scaled to the batch
by the series count; and the block route (`Seasons(7)` + `Seasons(4, num_steps_per_season=7)`, 64
series), simulated against analytic, likewise.

Prints one JSON line per leg: wall-clock ms of every run, their median and their spread (max - min).

  python tools/exp_placebo_simulated.py [--series 512] [--steps 500] [--covariates 5] [--draws 1000]
      [--runs 5] [--share 64] [--block-series 64] [--out profiles/placebo_simulated.jsonl]
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
SEED = (0, 1)


def report(leg, times, **extra):
  LINES.append(json.dumps(dict(leg=leg, median_ms=statistics.median(times), spread_ms=max(times) - min(times),
                               all_ms=[round(t, 2) for t in times], **extra)))
  print(LINES[-1], flush=True)


def positive(values):
  """The outcome column as a positive, multiplicative one: exp of its standardised values."""
  out = values.copy()
  y = values[:, :, 0]
  out[:, :, 0] = np.exp(3.0 + 0.25 * (y - y.mean(axis=1, keepdims=True)) / y.std(axis=1, keepdims=True))
  return out


def session_legs(values, index, pre, post, draws, count, runs, host, seasons=()):
  """A finished session of the first `count` series fitted to the log outcome: the simulated and the
  analytic device call `runs` times each, interleaved (host=False), or the download of its parameter
  draws and the numpy twin on them, once (host=True)."""
  logged = values[:count].copy()
  logged[:, :, 0] = np.log(logged[:, :, 0])
  prep = batch.prepare_batch(logged, index, pre, post)
  raw = batch.prepare_batch(values[:count], index, pre, post)
  T, P = prep.y.shape[1], prep.design.shape[2]
  num_seasons, season_change = _model.expand_seasons(seasons, T)
  params = [_model.series_params(prep.y[b], prep.mask[b], prep.design[b], num_seasonal_blocks=len(num_seasons),
                                 outcome_sd=float(np.nanstd(prep.y[b, :prep.num_pre], ddof=1)))
            for b in range(count)]
  dim = lib.prediction_state_dim(False, num_seasons)
  origins, horizon = batch.placebo_plans(lib.Placebo(), [prep.num_pre] * count,
                                         [int(np.count_nonzero(prep.flags & 2))] * count, dim)
  seen = np.nan_to_num(np.stack([lib._placebo_seen_linked(               # pylint: disable=protected-access
      raw.observed[b], prep.mask[b], origins[b], horizon[b], _native.LINK_LOG)[1] for b in range(count)]))
  ranks = lib._placebo_sim_ranks(draws, (0.025, 0.975))                   # pylint: disable=protected-access
  pb = _native.make_problem(T=T, P=P, has_slope=False, num_warmup=-(-draws // 9), num_results=draws,
                            num_series=count, seed=SEED, num_seasons=num_seasons)
  sess = _native.Session(pb, prep.y, prep.mask, prep.design, season_change if len(num_seasons) else None,
                         _native.make_params(params))
  blocks = not lib.device_predictions_supported(num_seasons)
  analytic = sess.summarize_placebo_blocks if blocks else sess.summarize_placebo
  args = (prep.outcome_sd, prep.outcome_mean, origins, horizon)
  try:
    sess.run()
    if not host:
      sess.simulate_placebo(*args, _native.LINK_LOG, seen, ranks, blocks=blocks)      # warm-up: the scratch
      analytic(*args)
      sim, ana = [], []
      for _ in range(runs):                                               # interleaved: drift hits both alike
        t0 = time.perf_counter()
        sess.simulate_placebo(*args, _native.LINK_LOG, seen, ranks, blocks=blocks)
        t1 = time.perf_counter()
        analytic(*args)
        t2 = time.perf_counter()
        sim.append((t1 - t0) * 1e3)
        ana.append((t2 - t1) * 1e3)
      return sim, ana, int(origins.shape[1]), int(horizon[0])
    t0 = time.perf_counter()
    out = sess.fetch(list(DRAWS))
    t1 = time.perf_counter()
    y32, X32 = np.where(prep.mask, 0.0, prep.y).astype(np.float32), prep.design.astype(np.float32)
    for b in range(count):
      lib._placebo_simulated_host(                        # pylint: disable=protected-access
          y32[b], prep.mask[b], X32[b], season_change, num_seasons, False, params[b],
          {k: out[k][b, 0] for k in DRAWS}, prep.outcome_sd[b], prep.outcome_mean[b], origins[b], horizon[b],
          _native.LINK_LOG, lib.placebo_stream(SEED, b, (0,)), seen=seen[b], ranks=ranks)
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
  ap.add_argument("--block-series", type=int, default=64)
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "placebo_simulated.jsonl"))
  a = ap.parse_args()
  B, T = a.series, a.steps
  values = positive(np.stack([np.column_stack(syn.make_raw_series(T, a.covariates, b)) for b in range(B)]))
  index = pd.RangeIndex(T)
  pre, post = (0, int(0.7 * T) - 1), (int(0.7 * T), T - 1)

  def fit(on):
    return ci.fit_causalimpact_batch(values, pre, post, seed=SEED, index=index, outcome_link="log",
                                     placebo=ci.Placebo(simulate=True) if on else None,
                                     inference_options=ci.InferenceOptions(num_results=a.draws))

  fit(False), fit(True)                                     # warm-up: library load, scratch, pools
  off, on = [], []
  for _ in range(a.runs):                                   # interleaved: drift hits both alike
    t0 = time.perf_counter()
    fit(False)
    t1 = time.perf_counter()
    fit(True)
    t2 = time.perf_counter()
    off.append((t1 - t0) * 1e3)
    on.append((t2 - t1) * 1e3)
  shape = dict(series=B, steps=T, covariates=a.covariates, draws=a.draws)
  report("link_placebo_off", off, **shape)
  report("link_placebo_simulated", on, **shape)
  sim, ana, num_origins, horizon = session_legs(values, index, pre, post, a.draws, B, a.runs, False)
  report("device_call_simulated", sim, origins=num_origins, horizon=horizon, **shape,
         note="Session.simulate_placebo: predicted_mean, spread_mean, below, total_order; one filter pass")
  report("device_call_analytic", ana, origins=num_origins, horizon=horizon, **shape,
         note="Session.summarize_placebo on the same session: three outputs, three filter passes")
  share = min(a.share, B)
  fetch, forecast = session_legs(values, index, pre, post, a.draws, share, 1, True)
  report("numpy_share_fetch", [fetch], series=share)
  report("numpy_share_simulate", [forecast], series=share, scaled_to_batch_ms=forecast * B / share)
  nb = min(a.block_series, B)
  sim, ana, num_origins, horizon = session_legs(values, index, pre, post, a.draws, nb, a.runs, False,
                                                seasons=((7, 1), (4, 7)))
  shape = dict(shape, series=nb, seasons="Seasons(7) + Seasons(4, num_steps_per_season=7)")
  report("block_device_call_simulated", sim, origins=num_origins, horizon=horizon, **shape)
  report("block_device_call_analytic", ana, origins=num_origins, horizon=horizon, **shape)
  with open(a.out, "w", encoding="utf-8") as f:
    f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
  main()
