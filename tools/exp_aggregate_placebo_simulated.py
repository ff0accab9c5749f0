"""What the SIMULATED placebo forecasts of POOLED effects cost a batch fitted under `outcome_link="log"`:
`fit_causalimpact_batch` at the shape of BASELINE cfg5 (512 series, T = 500, 5 covariates, 1 chain x
1000 draws) with positive outcomes and four aggregates (all series, two halves, a weighted quarter:
1152 entries), as medians of interleaved rounds after one warm-up of each --
  the call with `Placebo(simulate=True)` and no aggregates,
  the call with the aggregates and no placebo,
  the call with both and `pool=True`;
the device call alone (`Session.pool_simulated_placebo` with `seen`, `counted` and the frame's ranks on
a finished session of the whole batch) next to its yardstick, `Session.simulate_placebo` at the same
shape on the same session; and the host twin on a share of the batch (64 series): the parameter draws
downloaded, every entry simulated in numpy (`causalimpact_lib._placebo_simulated_host`) and pooled by
`_native.pool_simulated_placebo_host` / `_native.finish_simulated_placebo_host`.

With `--seasons MODEL` the same for a model the one-lane filter does not take
(`Session.pool_simulated_placebo_blocks` next to `Session.simulate_placebo_blocks`): 64 series by
default, the host twin on `--share` series with `--twin-origins` origins each.

With `--baseline-root DIR` (a built checkout of the parent commit) the stock paths -- the device calls
of `Session.summarize_predictions`, `summarize_placebo`, `simulate_placebo`, `pool_placebo` and
`pool_simulated_placebo` on the 512 series, and of their _blocks builds on 64 series of the
weekly+monthly model -- parent and branch alternating, one child process per session and run, five
runs each, with the checksum of their outputs; written to `--stock-out`.

Prints one JSON line per leg: wall-clock ms of every run, their median and their spread (max - min).

  python tools/exp_aggregate_placebo_simulated.py [--series 512] [--steps 500] [--covariates 5] [--draws 1000]
      [--runs 5] [--share 64] [--out profiles/aggregate_placebo_simulated.jsonl]
  python tools/exp_aggregate_placebo_simulated.py --seasons weekly+monthly|seasons52 [--series 64] [--share 4]
      [--twin-origins 4] [--out profiles/aggregate_placebo_simulated_blocks.jsonl]
  python tools/exp_aggregate_placebo_simulated.py --baseline-root DIR
      [--stock-out profiles/aggregate_placebo_simulated_stock_parent_vs_branch.jsonl]
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
TREE = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else ROOT
for p in (TREE, os.path.join(TREE, "tfp-causalimpact_amd")):
  if p not in sys.path:
    sys.path.insert(0, p)

import numpy as np  # pylint: disable=wrong-import-position
import pandas as pd  # pylint: disable=wrong-import-position

import causalimpact as ci  # pylint: disable=wrong-import-position
from causalimpact import _model, _native, batch  # pylint: disable=wrong-import-position
from causalimpact import _synthetic as syn  # pylint: disable=wrong-import-position
from causalimpact import causalimpact_lib as lib  # pylint: disable=wrong-import-position

DRAWS = ("observation_noise_scale", "level_scale", "slope_scale", "seasonal_drift_scales", "weights")
MODELS = {
    None: dict(),
    "weekly+monthly": dict(local_linear_trend=False, seasons=[ci.Seasons(7), ci.Seasons(4, num_steps_per_season=7)]),
    "seasons52": dict(local_linear_trend=True, seasons=[ci.Seasons(52)]),
}
ALPHA = 0.05
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


def positive_values(B, T, covariates):
  """[B, T, 1 + covariates]: outcomes around 20 that move multiplicatively, the covariates as they are."""
  out = []
  for b in range(B):
    y, X = syn.make_raw_series(T, covariates, b)
    out.append(np.column_stack([np.exp(3.0 + 0.25 * (y - y.mean()) / y.std()), X]))
  return np.stack(out)


def open_session(model, values, index, pre, post, draws, count, max_origins=None):
  """An open, not yet run session of the first `count` series on the LOG of the outcome, and what the
  simulated placebo, pooled over the four aggregates or not, needs."""
  mo = MODELS[model]
  logged = values[:count].copy()
  logged[:, :, 0] = np.log(logged[:, :, 0])
  prep = batch.prepare_batch(logged, index, pre, post)
  raw = batch.prepare_batch(values[:count], index, pre, post)
  T, P = prep.y.shape[1], prep.design.shape[2]
  num_seasons, sc = _model.expand_seasons(mo.get("seasons", ()), T)
  hs = bool(mo.get("local_linear_trend", False))
  d = lib.prediction_state_dim(hs, num_seasons)
  params = [_model.series_params(prep.y[b], prep.mask[b], prep.design[b], has_slope=hs,
                                 num_seasonal_blocks=len(num_seasons),
                                 outcome_sd=float(np.nanstd(prep.y[b, :prep.num_pre], ddof=1)))
            for b in range(count)]
  n_post = int(np.count_nonzero(prep.flags & 2))
  placebo = lib.Placebo() if max_origins is None else lib.Placebo(max_origins=max_origins)
  origins, horizon = batch.placebo_plans(placebo, [prep.num_pre] * count, [n_post] * count, d)
  names, csr = batch.aggregate_groups(aggregates_of(count), range(count))
  pp = batch.batch_placebo_pool_plan(csr, origins[0], horizon[0], n_post, prep.index[prep.model_rows])
  groups = [dict(zip(csr[1][csr[0][g]:csr[0][g + 1]].tolist(), csr[2][csr[0][g]:csr[0][g + 1]].tolist()))
            for g in range(len(names))]
  y32 = np.where(prep.mask, 0.0, prep.y).astype(np.float32)
  inputs = [lib.SeriesInputs(y32[b], prep.mask[b], prep.design[b], sc, num_seasons, hs, params[b]) for b in range(count)]
  per_series = [lib._placebo_seen_linked(raw.observed[b], prep.mask[b], origins[b], int(horizon[b]), _native.LINK_LOG)   # pylint: disable=protected-access
                for b in range(count)]
  # (the pooled observed totals as `batch._placebo_pool_observed` forms them under a link, from what the
  #  parent commit has too: the stock paths run this function on its package)
  observed = dict(seen_sum=np.zeros(pp.columns.shape), n_counted=np.zeros(pp.columns.shape))
  for g in range(len(names)):
    for k in range(csr[0][g], csr[0][g + 1]):
      cnt, seen = per_series[csr[1][k]]
      observed["seen_sum"][g] = observed["seen_sum"][g] + csr[2][k] * np.nan_to_num(seen)
      observed["n_counted"][g] = observed["n_counted"][g] + cnt
  pb = _native.make_problem(T=T, P=P, has_slope=hs, num_warmup=-(-draws // 9), num_results=draws,
                            num_series=count, seed=(0, 1), num_seasons=num_seasons)
  sess = _native.Session(pb, prep.y, prep.mask, prep.design, sc if len(num_seasons) else None, _native.make_params(params))
  return sess, dict(prep=prep, origins=origins, horizon=horizon, groups=groups, csr=csr, pp=pp, inputs=inputs,
                    seen=observed["seen_sum"], counted=observed["n_counted"].astype(np.int32), state=d,
                    series_seen=np.nan_to_num(np.stack([s for _, s in per_series])),
                    ranks=lib._placebo_sim_ranks(draws, (ALPHA / 2, 1 - ALPHA / 2)))   # pylint: disable=protected-access


def checksum(got):
  return float(sum(np.abs(np.asarray(v, np.float64)).sum() for v in got.values()))


def stock_child(a, values, index, pre, post):
  """One run of the stock paths of one session -- `--child one_lane`: the five Kalman-filter entries;
  `--child blocks`: their _blocks builds on the weekly+monthly model -- each `--runs` times after a
  warm-up, and the checksum of its outputs: one JSON line per entry."""
  blocks = a.child == "blocks"
  sess, w = open_session("weekly+monthly" if blocks else None, values, index, pre, post, a.draws, a.series)
  sfx = "_blocks" if blocks else ""
  try:
    sess.run()
    prep = w["prep"]
    sc, sh, H = prep.outcome_sd, prep.outcome_mean, int(w["horizon"][0])
    calls = {
        "summarize_predictions" + sfx: lambda: getattr(sess, "summarize_predictions" + sfx)(sc, sh, w["ranks"]),
        "summarize_placebo" + sfx: lambda: getattr(sess, "summarize_placebo" + sfx)(sc, sh, w["origins"], w["horizon"]),
        "simulate_placebo" + sfx: lambda: sess.simulate_placebo(sc, sh, w["origins"], w["horizon"], _native.LINK_LOG,
                                                                w["series_seen"], w["ranks"], blocks=blocks),
        "pool_placebo" + sfx: lambda: getattr(sess, "pool_placebo" + sfx)(sc, sh, w["groups"], w["origins"], H,
                                                                          seen=w["seen"]),
        "pool_simulated_placebo" + sfx: lambda: sess.pool_simulated_placebo(
            sc, sh, w["groups"], w["origins"], H, _native.LINK_LOG, None, w["seen"], w["counted"], w["ranks"],
            blocks=blocks),
    }
    for name, call in calls.items():
      got = call()                                            # warm-up: the scratch
      times = []
      for _ in range(a.runs):
        t0 = time.perf_counter()
        got = call()
        times.append((time.perf_counter() - t0) * 1e3)
      print(json.dumps(dict(entry=name, median_ms=statistics.median(times), all_ms=[round(t, 3) for t in times],
                            checksum=checksum(got))), flush=True)
  finally:
    sess.close()


STOCK = (("one_lane", 512), ("blocks", 64))


def stock_main(a):
  """Parent and branch alternating, the parent first in each round; one child process per run."""
  lines, got = [], {}
  for child, series in STOCK:
    for run in range(1, 6):
      for tree, root in (("parent", a.baseline_root), ("branch", ROOT)):
        cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--child", child, "--series", str(series),
               "--steps", str(a.steps), "--covariates", str(a.covariates), "--draws", str(a.draws), "--runs", str(a.runs)]
        out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout.strip().splitlines()
        for one in (json.loads(l) for l in out if l.startswith("{")):
          entry = one.pop("entry")
          got.setdefault((entry, series), []).append((tree, one))
          lines.append(json.dumps(dict(tree=tree, run=run, leg=f"Session.{entry}, {series} series, stock path", **one)))
          print(lines[-1], flush=True)
  for (entry, series), runs in got.items():
    parent = [g["median_ms"] for t, g in runs if t == "parent"]
    branch = [g["median_ms"] for t, g in runs if t == "branch"]
    lines.append(json.dumps(dict(
        leg=f"Session.{entry}", series=series, parent_median_ms=statistics.median(parent), parent_min_ms=min(parent),
        parent_max_ms=max(parent), branch_median_ms=statistics.median(branch), branch_min_ms=min(branch),
        branch_max_ms=max(branch), checksums_equal=len({g["checksum"] for _, g in runs}) == 1,
        ranges_overlap=min(branch) <= max(parent) and min(parent) <= max(branch),
        branch_median_inside_parent_range=min(parent) <= statistics.median(branch) <= max(parent))))
    print(lines[-1], flush=True)
  with open(a.stock_out, "w", encoding="utf-8") as f:
    f.write("\n".join(lines) + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--seasons", choices=sorted(k for k in MODELS if k), default=None, help="a block list: the block-model route")
  ap.add_argument("--twin-origins", type=int, default=None, help="origins per entry of the numpy share (default: all)")
  ap.add_argument("--baseline-root", default=None, help="a built checkout of the parent commit: the stock paths only")
  ap.add_argument("--stock-out", default=os.path.join(ROOT, "profiles", "aggregate_placebo_simulated_stock_parent_vs_branch.jsonl"))
  ap.add_argument("--root", default=ROOT, help="(child runs) the tree whose package is imported")
  ap.add_argument("--child", choices=[c for c, _ in STOCK], default=None, help="(child runs) one run, one JSON line")
  ap.add_argument("--series", type=int, default=None, help="512; 64 with --seasons")
  ap.add_argument("--steps", type=int, default=500)
  ap.add_argument("--covariates", type=int, default=5)
  ap.add_argument("--draws", type=int, default=1000)
  ap.add_argument("--runs", type=int, default=5)
  ap.add_argument("--share", type=int, default=None, help="64; 4 with --seasons")
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  blocks = a.seasons is not None
  a.series = a.series or (64 if blocks else 512)
  a.share = a.share or (4 if blocks else 64)
  a.out = a.out or os.path.join(ROOT, "profiles", "aggregate_placebo_simulated_blocks.jsonl" if blocks
                                else "aggregate_placebo_simulated.jsonl")
  if a.baseline_root and not a.child:
    return stock_main(a)
  B, T = a.series, a.steps
  values = positive_values(B, T, a.covariates)
  index = pd.RangeIndex(T)
  pre, post = (0, int(0.7 * T) - 1), (int(0.7 * T), T - 1)
  if a.child:
    return stock_child(a, values, index, pre, post)
  mo = ci.ModelOptions(**MODELS[a.seasons])
  kw = dict(seed=1, index=index, outcome_link="log", alpha=ALPHA, model_options=mo,
            inference_options=ci.InferenceOptions(num_results=a.draws))
  legs = (("simulated_placebo_only", dict(placebo=ci.Placebo(simulate=True))),
          ("aggregates_only", dict(aggregates=aggregates_of(B))),
          ("pooled_simulated_placebo", dict(placebo=ci.Placebo(simulate=True, pool=True), aggregates=aggregates_of(B))))
  for _, extra in legs:                                     # warm-up: library load, scratch, pools
    ci.fit_causalimpact_batch(values, pre, post, **kw, **extra)
  times = {leg: [] for leg, _ in legs}
  for _ in range(a.runs):                                   # interleaved: drift hits all alike
    for leg, extra in legs:
      t0 = time.perf_counter()
      res = ci.fit_causalimpact_batch(values, pre, post, **kw, **extra)
      times[leg].append((time.perf_counter() - t0) * 1e3)
      assert (res.aggregate_placebo_quality is not None) == (leg == "pooled_simulated_placebo")
  shape = dict(model=a.seasons or "level", series=B, steps=T, covariates=a.covariates, draws=a.draws, aggregates=4,
               outcome_link="log")
  report("simulated_placebo_only", times["simulated_placebo_only"], note="Placebo(simulate=True), no aggregates", **shape)
  report("aggregates_only", times["aggregates_only"], note="four aggregates, no placebo", **shape)
  report("pooled_simulated_placebo", times["pooled_simulated_placebo"],
         note="Placebo(simulate=True, pool=True) and the four aggregates", **shape)
  sess, w = open_session(a.seasons, values, index, pre, post, a.draws, B)
  try:
    sess.run()
    prep, origins, horizon = w["prep"], w["origins"], w["horizon"]
    sc, sh = prep.outcome_sd, prep.outcome_mean
    plan = dict(state=w["state"], origins=int(origins.shape[1]), horizon=int(horizon[0]), entries=int(w["csr"][0][-1]),
                kernel=sess.kernel_name())
    pooled = lambda: sess.pool_simulated_placebo(sc, sh, w["groups"], origins, int(horizon[0]), _native.LINK_LOG, None,   # pylint: disable=unnecessary-lambda-assignment
                                                 w["seen"], w["counted"], w["ranks"], blocks=blocks)
    single = lambda: sess.simulate_placebo(sc, sh, origins, horizon, _native.LINK_LOG, w["series_seen"], w["ranks"],   # pylint: disable=unnecessary-lambda-assignment
                                           blocks=blocks)
    pooled(), single()                                      # warm-up: the scratch
    dev = ([], [])
    for _ in range(a.runs):
      for leg, call in enumerate((pooled, single)):
        t0 = time.perf_counter()
        call()
        dev[leg].append((time.perf_counter() - t0) * 1e3)
    report("device_call", dev[0], note="Session.pool_simulated_placebo with seen, counted and the frame's ranks: one "
           "simulation pass per chunk of entries, the accumulators, the statistics", **shape, **plan)
    report("device_call_yardstick", dev[1], note="Session.simulate_placebo, the same statistics, same session",
           ratio_pooled_to_yardstick=statistics.median(dev[0]) / statistics.median(dev[1]),
           entries_per_series=plan["entries"] / B, **shape, **plan)
    # the host twin on a stated share: the four aggregates over the first `share` series
    share = min(a.share, B)
    few = origins.shape[1] if a.twin_origins is None else a.twin_origins
    names, csr = batch.aggregate_groups(aggregates_of(share), range(share))
    t0 = time.perf_counter()
    out = sess.fetch(list(DRAWS))
    t1 = time.perf_counter()
    totals = [lib._placebo_simulated_host(                    # pylint: disable=protected-access
        *w["inputs"][b].filter_inputs(), {k: out[k][b, 0] for k in DRAWS}, sc[b], sh[b], origins[b, :few],
        int(horizon[0]), _native.LINK_LOG, lib.placebo_stream((0, 1), b, range(1)))["totals"] for b in csr[1].tolist()]
    t2 = time.perf_counter()
    acc = _native.pool_simulated_placebo_host(np.stack(totals), csr)
    _native.finish_simulated_placebo_host(acc, np.zeros(acc.shape[:2]), np.ones(acc.shape[:2], np.int32), w["ranks"])
    t3 = time.perf_counter()
    report("numpy_share_fetch", [(t1 - t0) * 1e3], series=B)
    report("numpy_share_simulate", [(t2 - t1) * 1e3], note="lib._placebo_simulated_host of every entry", series=share,
           entries=len(totals), origins=int(few), horizon=int(horizon[0]), per_entry_ms=(t2 - t1) * 1e3 / len(totals),
           groups=len(names), **{k: v for k, v in shape.items() if k not in ("series", "aggregates")})
    report("numpy_share_pool_and_finish", [(t3 - t2) * 1e3], series=share, entries=len(totals))
  finally:
    sess.close()
  with open(a.out, "w", encoding="utf-8") as f:
    f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
  main()
