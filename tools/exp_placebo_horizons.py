"""What the placebo table at several horizons costs, at the shape of BASELINE cfg5 (512 series, T = 500,
5 covariates, 1 chain x 1000 draws; the default plan: 32 origins, H = 116), at K = 8 and K = 16
horizons (`Placebo(horizons=K)`: spread over 1..H):

  device_call      `Session.summarize_placebo_horizons` on a finished session of the whole batch: one
                   filter pass per chunk and 3 K row-statistics passes;
  k_calls          K calls of `Session.summarize_placebo` on the same session with the same origins and
                   horizon h_k -- 3 K filter passes: the only way to the same numbers before this entry,
                   and the baseline (the two tables are compared bit for bit before anything is timed);
  batch_off / on   `fit_causalimpact_batch` with `placebo=Placebo()` and `Placebo(horizons=K)`;
  numpy_share      `_placebo_summary_host(horizons=...)` on the downloaded draws of a share of the batch
                   (64 series), scaled to the batch by the series count.

The legs of a round run interleaved, after one warm-up of each; every leg reports the wall-clock ms of
every round, their median and their spread (max - min).

With `--baseline-root DIR` (a built checkout of the parent commit) the STOCK path -- `Session.summarize_placebo`
at the same shape, which this work must leave as it was -- parent and branch alternating, one child
process per run, five runs each, with the checksum of the outputs; written to `--stock-out`.

  python tools/exp_placebo_horizons.py [--series 512] [--steps 500] [--covariates 5] [--draws 1000]
      [--rounds 5] [--share 64] [--out profiles/placebo_horizons.jsonl]
      [--baseline-root DIR] [--stock-out profiles/placebo_horizons_stock_parent_vs_branch.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (`--root DIR`, the child runs: the tree whose package is measured, the parent's checkout or this one)
_TREE = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else ROOT
for p in (_TREE, os.path.join(_TREE, "tfp-causalimpact_amd")):
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


def data(a):
  values = np.stack([np.column_stack(syn.make_raw_series(a.steps, a.covariates, b)) for b in range(a.series)])
  return values, pd.RangeIndex(a.steps), (0, int(0.7 * a.steps) - 1), (int(0.7 * a.steps), a.steps - 1)


def open_session(values, index, pre, post, draws, count):
  """(finished session of the first `count` series, prep, params, origins [B, O], horizon [B])."""
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
  sess.run()
  return sess, prep, params, origins, horizon


def timed(fn):
  t0 = time.perf_counter()
  out = fn()
  return (time.perf_counter() - t0) * 1e3, out


def main_legs(a):
  values, index, pre, post = data(a)
  shape = dict(series=a.series, steps=a.steps, covariates=a.covariates, draws=a.draws)
  sess, prep, _, origins, horizon = open_session(values, index, pre, post, a.draws, a.series)
  try:
    H = int(horizon[0])
    for K in a.horizons:
      hs = lib.placebo_horizon_list(lib.Placebo(horizons=K), H)
      one = lambda: sess.summarize_placebo_horizons(prep.outcome_sd, prep.outcome_mean, origins, hs)   # pylint: disable=cell-var-from-loop
      each = lambda: [sess.summarize_placebo(prep.outcome_sd, prep.outcome_mean, origins, int(h)) for h in hs]   # pylint: disable=cell-var-from-loop
      table, columns = one(), each()                        # warm-up of both, and the comparison
      same = all(np.array_equal(table[name][:, :, k], columns[k][name])
                 for k in range(len(hs)) for name in _native.PLACEBO_OUTPUTS)
      chunks = sess.summarize_placebo_horizons(prep.outcome_sd, prep.outcome_mean, origins, hs,
                                               max_rows=2 ** 40)["num_chunks"]
      new, old = [], []
      for _ in range(a.rounds):                             # interleaved: drift hits both alike
        new.append(timed(one)[0])
        old.append(timed(each)[0])
      note = dict(horizons=[int(h) for h in hs], origins=int(origins.shape[1]), bits_equal=bool(same), **shape)
      report(f"device_call_K{len(hs)}", new, note="Session.summarize_placebo_horizons, all three outputs",
             filter_passes=int(chunks), **note)
      report(f"k_calls_K{len(hs)}", old, note="K calls of Session.summarize_placebo, all three outputs",
             filter_passes=3 * len(hs), **note)
      LINES.append(json.dumps(dict(leg=f"ratio_K{len(hs)}", k_calls_over_device_call=statistics.median(old) / statistics.median(new))))
      print(LINES[-1], flush=True)
  finally:
    sess.close()

  def fit(placebo):
    return ci.fit_causalimpact_batch(values, pre, post, seed=1, index=index, placebo=placebo,
                                     inference_options=ci.InferenceOptions(num_results=a.draws))

  options = [("batch_placebo_at_H", lib.Placebo())] + [(f"batch_horizons_K{K}", lib.Placebo(horizons=K)) for K in a.horizons]
  for _, placebo in options:
    fit(placebo)                                            # warm-up: library load, scratch, pools
  times = {name: [] for name, _ in options}
  tables = {name: [] for name, _ in options if name != "batch_placebo_at_H"}
  for _ in range(a.rounds):
    for name, placebo in options:
      ms, res = timed(lambda: fit(placebo))                 # pylint: disable=cell-var-from-loop
      times[name].append(ms)
      if name in tables:
        tables[name].append(timed(lambda: res.placebo_profile)[0])   # pylint: disable=cell-var-from-loop
  for name, _ in options:
    report(name, times[name], **shape)
    if name in tables:
      report(name + "_profile_table", tables[name], note="the batch's placebo_profile, (series, horizon)", **shape)

  share = min(a.share, a.series)
  sess, prep, params, origins, horizon = open_session(values, index, pre, post, a.draws, share)
  try:
    fetch, out = timed(lambda: sess.fetch(list(DRAWS)))
  finally:
    sess.close()
  report("numpy_share_fetch", [fetch], series=share)
  y32, X32 = np.where(prep.mask, 0.0, prep.y).astype(np.float32), prep.design.astype(np.float32)
  T = prep.y.shape[1]
  for K in a.horizons:
    hs = lib.placebo_horizon_list(lib.Placebo(horizons=K), int(horizon[0]))
    def twin():
      for b in range(share):
        lib._placebo_summary_host(                          # pylint: disable=protected-access
            y32[b], prep.mask[b], X32[b], np.zeros((0, T), np.uint8), [], False, params[b],
            {k: out[k][b, 0] for k in DRAWS}, prep.outcome_sd[b], prep.outcome_mean[b], origins[b], horizons=hs)   # pylint: disable=cell-var-from-loop
    ms = timed(twin)[0]
    report(f"numpy_share_K{len(hs)}", [ms], series=share, scaled_to_batch_ms=ms * a.series / share)
  with open(a.out, "w", encoding="utf-8") as f:
    f.write("\n".join(LINES) + "\n")


def stock_child(a):
  """One run of the stock path: `Session.summarize_placebo` at H on a finished session of the batch."""
  values, index, pre, post = data(a)
  sess, prep, _, origins, horizon = open_session(values, index, pre, post, a.draws, a.series)
  try:
    call = lambda: sess.summarize_placebo(prep.outcome_sd, prep.outcome_mean, origins, horizon)
    got = call()                                            # warm-up: the scratch
    times = [timed(call)[0] for _ in range(a.rounds)]
  finally:
    sess.close()
  print(json.dumps(dict(median_ms=statistics.median(times), all_ms=[round(t, 3) for t in times],
                        checksum=float(sum(np.abs(got[k]).sum() for k in _native.PLACEBO_OUTPUTS)))))


def stock_main(a):
  """Parent and branch alternating, the parent first in each round; one child process per run."""
  lines, runs = [], []
  forward = ["--series", a.series, "--steps", a.steps, "--covariates", a.covariates, "--draws", a.draws,
             "--rounds", a.rounds]
  for run in range(1, 6):
    for tree, root in (("parent", a.baseline_root), ("branch", ROOT)):
      out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", root] +
                           [str(v) for v in forward], check=True, capture_output=True, text=True, timeout=600).stdout
      one = json.loads(out.strip().splitlines()[-1])
      runs.append((tree, one))
      lines.append(json.dumps(dict(tree=tree, run=run, leg=f"Session.summarize_placebo, cfg5 shape, {a.series} series", **one)))
      print(lines[-1], flush=True)
  parent = [g["median_ms"] for t, g in runs if t == "parent"]
  branch = [g["median_ms"] for t, g in runs if t == "branch"]
  lines.append(json.dumps(dict(
      leg="Session.summarize_placebo", parent_median_ms=statistics.median(parent), parent_min_ms=min(parent),
      parent_max_ms=max(parent), branch_median_ms=statistics.median(branch), branch_min_ms=min(branch),
      branch_max_ms=max(branch), checksums_equal=len({g["checksum"] for _, g in runs}) == 1,
      branch_median_inside_parent_range=min(parent) <= statistics.median(branch) <= max(parent))))
  print(lines[-1], flush=True)
  with open(a.stock_out, "w", encoding="utf-8") as f:
    f.write("\n".join(lines) + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--series", type=int, default=512)
  ap.add_argument("--steps", type=int, default=500)
  ap.add_argument("--covariates", type=int, default=5)
  ap.add_argument("--draws", type=int, default=1000)
  ap.add_argument("--rounds", type=int, default=5)
  ap.add_argument("--share", type=int, default=64)
  ap.add_argument("--horizons", type=int, nargs="+", default=[8, 16])
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "placebo_horizons.jsonl"))
  ap.add_argument("--baseline-root", default=None, help="a built checkout of the parent commit: the stock path only")
  ap.add_argument("--stock-out", default=os.path.join(ROOT, "profiles", "placebo_horizons_stock_parent_vs_branch.jsonl"))
  ap.add_argument("--root", default=ROOT, help="(child runs) the tree whose package is imported")
  ap.add_argument("--child", action="store_true", help="(internal) one stock run of the tree `--root`")
  a = ap.parse_args()
  if a.child:
    return stock_child(a)
  if a.baseline_root:
    return stock_main(a)
  return main_legs(a)


if __name__ == "__main__":
  main()
