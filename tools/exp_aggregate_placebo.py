"""What the placebo forecasts of POOLED effects cost a batch: `fit_causalimpact_batch` at the shape of
BASELINE cfg5 (512 series, T = 500, 5 covariates, 1 chain x 1000 draws) with `placebo=True` and four
aggregates (all series, two halves, a weighted quarter), the pooled placebo off -- the launch and the
frames of the call without it, its chain and its frames stubbed out here -- and on, as medians of
interleaved rounds after one warm-up of each; the device call alone (`Session.pool_placebo` with
`seen` on a finished session of the whole batch) next to its yardstick, `Session.summarize_placebo`
at the same shape on the same session; and the host twin on a share of the batch (64 series): the
parameter draws downloaded, every entry filtered in numpy (`causalimpact_lib._placebo_entry_host`)
and pooled by `_native.pool_placebo_host` / `_native.finish_placebo_host`, scaled to the batch by the
entry count.

Prints one JSON line per leg: wall-clock ms of every run, their median and their spread (max - min).

  python tools/exp_aggregate_placebo.py [--series 512] [--steps 500] [--covariates 5] [--draws 1000]
                                        [--runs 5] [--share 64] [--out profiles/aggregate_placebo.jsonl]
"""
import argparse
import contextlib
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


def aggregates_of(count):
  """Four groups over `count` series: all, the two halves, every fourth series with weight 0.5."""
  half = count // 2
  return {"all": "all", "first_half": list(range(half)), "second_half": list(range(half, count)),
          "quarter": {b: 0.5 for b in range(0, count, 4)}}


class _NoChain:
  """The pooled placebo switched off: no step, no sums."""
  means = None

  def __init__(self, *a, **k):
    pass

  def session_pool(self, *a, **k):
    return None

  def step(self, *a, **k):
    pass

  def guarded(self, run):
    return run


@contextlib.contextmanager
def pooled_placebo_off():
  saved = (batch._PlaceboChain, batch._take_aggregate_placebo, batch._fit_placebo_observed)   # pylint: disable=protected-access
  batch._PlaceboChain = _NoChain                                                  # pylint: disable=protected-access
  batch._take_aggregate_placebo = lambda *a, **k: None                            # pylint: disable=protected-access
  batch._fit_placebo_observed = lambda *a, **k: {"seen_sum": None}                # pylint: disable=protected-access
  try:
    yield
  finally:
    batch._PlaceboChain, batch._take_aggregate_placebo, batch._fit_placebo_observed = saved   # pylint: disable=protected-access


def session_legs(values, index, pre, post, draws, count, runs, host):
  """A finished session of the first `count` series: the two device calls `runs` times each,
  interleaved (host=False), or the download of its parameter draws and the host twin, once."""
  prep = batch.prepare_batch(values[:count], index, pre, post)
  T, P = prep.y.shape[1], prep.design.shape[2]
  params = [_model.series_params(prep.y[b], prep.mask[b], prep.design[b],
                                 outcome_sd=float(np.nanstd(prep.y[b, :prep.num_pre], ddof=1)))
            for b in range(count)]
  n_post = int(np.count_nonzero(prep.flags & 2))
  origins, horizon = batch.placebo_plans(lib.Placebo(), [prep.num_pre] * count, [n_post] * count, 1)
  names, csr = batch.aggregate_groups(aggregates_of(count), range(count))
  pp = batch.batch_placebo_pool_plan(csr, origins[0], horizon[0], n_post, prep.index[prep.model_rows])
  groups = [dict(zip(csr[1][csr[0][g]:csr[0][g + 1]].tolist(), csr[2][csr[0][g]:csr[0][g + 1]].tolist()))
            for g in range(len(names))]
  y32 = np.where(prep.mask, 0.0, prep.y).astype(np.float32)
  inputs = [lib.SeriesInputs(y32[b], prep.mask[b], prep.design[b], np.zeros((0, T), np.uint8), (), False, params[b])
            for b in range(count)]
  seen = batch._placebo_pool_observed(pp, lambda g, k: lib._placebo_entry_seen(   # pylint: disable=protected-access
      inputs[csr[1][k]], prep.outcome_sd[csr[1][k]], prep.outcome_mean[csr[1][k]], prep.observed[csr[1][k]],
      pp.origins[k], int(pp.horizon[g])))["seen_sum"]
  pb = _native.make_problem(T=T, P=P, has_slope=False, num_warmup=-(-draws // 9), num_results=draws,
                            num_series=count, seed=(0, 1))
  sess = _native.Session(pb, prep.y, prep.mask, prep.design, None, _native.make_params(params))
  try:
    sess.run()
    if not host:
      pooled = lambda: sess.pool_placebo(prep.outcome_sd, prep.outcome_mean, groups, origins, int(horizon[0]), seen=seen)   # pylint: disable=unnecessary-lambda-assignment
      single = lambda: sess.summarize_placebo(prep.outcome_sd, prep.outcome_mean, origins, horizon)   # pylint: disable=unnecessary-lambda-assignment
      pooled(), single()                                      # warm-up: the scratch
      times = ([], [])
      for _ in range(runs):
        for leg, call in enumerate((pooled, single)):
          t0 = time.perf_counter()
          call()
          times[leg].append((time.perf_counter() - t0) * 1e3)
      return times, int(origins.shape[1]), int(horizon[0]), int(csr[0][-1])
    t0 = time.perf_counter()
    out = sess.fetch(list(DRAWS))
    t1 = time.perf_counter()
    terms = [lib._placebo_entry_host(                       # pylint: disable=protected-access
        inputs[b], {k: out[k][b, 0] for k in DRAWS}, prep.outcome_sd[b], prep.outcome_mean[b], prep.observed[b],
        pp.origins[k], int(horizon[0])) for k, b in enumerate(csr[1].tolist())]
    t2 = time.perf_counter()
    acc = _native.pool_placebo_host(np.stack([t["s"] for t in terms]), np.stack([t["v"] for t in terms]), csr)
    _native.finish_placebo_host(acc, seen)
    t3 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, int(csr[0][-1])
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
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aggregate_placebo.jsonl"))
  a = ap.parse_args()
  B, T = a.series, a.steps
  values = np.stack([np.column_stack(syn.make_raw_series(T, a.covariates, b)) for b in range(B)])
  index = pd.RangeIndex(T)
  pre, post = (0, int(0.7 * T) - 1), (int(0.7 * T), T - 1)

  def fit():
    return ci.fit_causalimpact_batch(values, pre, post, seed=1, index=index, placebo=True,
                                     aggregates=aggregates_of(B),
                                     inference_options=ci.InferenceOptions(num_results=a.draws))

  with pooled_placebo_off():
    fit()                                                   # warm-up: library load, scratch, pools
  fit()
  off, on = [], []
  for _ in range(a.runs):                                   # interleaved: drift hits both alike
    t0 = time.perf_counter()
    with pooled_placebo_off():
      res = fit()
    t1 = time.perf_counter()
    assert res.aggregate_placebo_quality is None
    res = fit()
    t2 = time.perf_counter()
    assert res.aggregate_placebo_quality.shape[0] == 4
    off.append((t1 - t0) * 1e3)
    on.append((t2 - t1 - 0.0) * 1e3)
  shape = dict(series=B, steps=T, covariates=a.covariates, draws=a.draws, aggregates=4)
  report("pooled_placebo_off", off, note="placebo=True and aggregates, the pooled placebo stubbed out", **shape)
  report("pooled_placebo_on", on, **shape)
  (pooled, single), num_origins, horizon, entries = session_legs(values, index, pre, post, a.draws, B, a.runs, False)
  report("device_call", pooled, note="Session.pool_placebo with seen: two filter passes per chunk of entries, "
         "the accumulators, the three means", origins=num_origins, horizon=horizon, entries=entries, **shape)
  report("device_call_yardstick", single, note="Session.summarize_placebo, all three outputs, same session",
         origins=num_origins, horizon=horizon, ratio_pooled_to_yardstick=statistics.median(pooled) / statistics.median(single),
         **shape)
  share = min(a.share, B)
  fetch, filt, pool, share_entries = session_legs(values, index, pre, post, a.draws, share, 1, True)
  report("numpy_share_fetch", [fetch], series=share)
  report("numpy_share_filter", [filt], series=share, entries=share_entries,
         scaled_to_batch_ms=filt * entries / share_entries)
  report("numpy_share_pool_and_finish", [pool], series=share, entries=share_entries,
         scaled_to_batch_ms=pool * entries / share_entries)
  with open(a.out, "w", encoding="utf-8") as f:
    f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
  main()
