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

With `--seasons MODEL` (a block list as in tools/exp_block_predictions.py) the same for a model the
one-lane filter does not take, whose pooled placebo `ci_session_pool_placebo_blocks` filters on the
device: 64 series by default, the batch call with the pooled placebo off and on, `Session.pool_placebo_blocks`
next to `Session.summarize_placebo_blocks` on the same session, and `_placebo_entry_host` on a stated
share -- the entries of the group of all series over the first `--share` series, `--twin-origins`
origins each.  With `--baseline-root DIR` (a built checkout of the parent commit) two more sets of
lines, parent and branch alternating, one child process per run: the package call with `placebo` and
`aggregates` at the stated, reduced shape (`--baseline-series`, `--baseline-origins`,
`--baseline-runs`: the parent pools such a model in numpy, so the full shape takes it hours), and with
`--stock` the stock path `Session.summarize_placebo_blocks` at the full shape with the checksum of its
outputs.
Lines are appended to `--out` (default profiles/aggregate_placebo_blocks.jsonl).

Prints one JSON line per leg: wall-clock ms of every run, their median and their spread (max - min).

  python tools/exp_aggregate_placebo.py [--series 512] [--steps 500] [--covariates 5] [--draws 1000]
                                        [--runs 5] [--share 64] [--out profiles/aggregate_placebo.jsonl]
  python tools/exp_aggregate_placebo.py --seasons weekly+monthly|seasons52 [--series 64] [--share 4]
      [--twin-origins 4] [--baseline-root DIR] [--baseline-series 16] [--baseline-origins 4] [--baseline-runs 5] [--stock]
"""
import argparse
import contextlib
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
    "weekly+monthly": dict(local_linear_trend=False, seasons=[ci.Seasons(7), ci.Seasons(4, num_steps_per_season=7)]),
    "seasons52": dict(local_linear_trend=True, seasons=[ci.Seasons(52)]),
}
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


def block_session(model, values, index, pre, post, draws, count, max_origins=None):
  """An open, not yet run session of the first `count` series under MODELS[model], and what the
  pooled placebo of the four aggregates over them needs."""
  mo = MODELS[model]
  prep = batch.prepare_batch(values[:count], index, pre, post)
  T, P = prep.y.shape[1], prep.design.shape[2]
  num_seasons, sc = _model.expand_seasons(mo["seasons"], T)
  hs = mo["local_linear_trend"]
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
  seen = batch._placebo_pool_observed(pp, lambda g, k: lib._placebo_entry_seen(   # pylint: disable=protected-access
      inputs[csr[1][k]], prep.outcome_sd[csr[1][k]], prep.outcome_mean[csr[1][k]], prep.observed[csr[1][k]],
      pp.origins[k], int(pp.horizon[g])))["seen_sum"]
  pb = _native.make_problem(T=T, P=P, has_slope=hs, num_warmup=-(-draws // 9), num_results=draws,
                            num_series=count, seed=(0, 1), num_seasons=num_seasons)
  sess = _native.Session(pb, prep.y, prep.mask, prep.design, sc, _native.make_params(params))
  return sess, dict(prep=prep, origins=origins, horizon=horizon, groups=groups, csr=csr, pp=pp, inputs=inputs,
                    seen=seen, state=d)


def stock_child(a, values, index, pre, post):
  """One run of the stock path: `Session.summarize_placebo_blocks`, `--runs` times, and its checksum."""
  sess, w = block_session(a.seasons, values, index, pre, post, a.draws, a.series)
  try:
    sess.run()
    prep = w["prep"]
    call = lambda: sess.summarize_placebo_blocks(prep.outcome_sd, prep.outcome_mean, w["origins"], w["horizon"])   # pylint: disable=unnecessary-lambda-assignment
    got = call()                                              # warm-up: the scratch
    times = []
    for _ in range(a.runs):
      t0 = time.perf_counter()
      got = call()
      times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(median_ms=statistics.median(times), all_ms=[round(t, 3) for t in times],
                          checksum=float(sum(np.abs(v).sum() for v in got.values())))), flush=True)
  finally:
    sess.close()


def package_child(a, values, index, pre, post):
  """One timed package call with `placebo` and `aggregates` after a warm-up without the pooled placebo."""
  B = a.series

  def fit():
    return ci.fit_causalimpact_batch(values[:B], pre, post, seed=1, index=index,
                                     placebo=ci.Placebo(max_origins=a.baseline_origins), aggregates=aggregates_of(B),
                                     model_options=ci.ModelOptions(**MODELS[a.seasons]),
                                     inference_options=ci.InferenceOptions(num_results=a.draws))

  with pooled_placebo_off():
    fit()                                                     # warm-up: library load, scratch, pools
  t0 = time.perf_counter()
  res = fit()
  ms = (time.perf_counter() - t0) * 1e3
  quality = res.aggregate_placebo_quality
  print(json.dumps(dict(ms=ms, checksum=float(np.nansum(np.abs(quality.to_numpy(np.float64)))))), flush=True)


def alternate(a, child, runs, extra):
  """[(tree, run, the child's JSON line)] of `runs` rounds, the parent's tree first in each."""
  out = []
  for run in range(1, runs + 1):
    for tree, root in (("parent", a.baseline_root), ("branch", ROOT)):
      cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--child", child, "--seasons", a.seasons,
             "--steps", str(a.steps), "--covariates", str(a.covariates), "--draws", str(a.draws),
             "--runs", str(a.runs)] + extra
      got = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1]
      out.append((tree, run, json.loads(got)))
      print(json.dumps(dict(progress=f"{child} {tree} run {run}", **out[-1][2])), flush=True)
  return out


def blocks_main(a, values, index, pre, post):
  B, model = a.series, a.seasons
  mo = ci.ModelOptions(**MODELS[model])
  shape = dict(model=model, series=B, steps=a.steps, covariates=a.covariates, draws=a.draws, aggregates=4)

  def fit():
    return ci.fit_causalimpact_batch(values, pre, post, seed=1, index=index, placebo=True, aggregates=aggregates_of(B),
                                     model_options=mo, inference_options=ci.InferenceOptions(num_results=a.draws))

  with pooled_placebo_off():
    fit()                                                   # warm-up: library load, scratch, pools
  fit()
  off, on = [], []
  for _ in range(a.runs):                                   # interleaved: drift hits both alike
    t0 = time.perf_counter()
    with pooled_placebo_off():
      fit()
    t1 = time.perf_counter()
    res = fit()
    t2 = time.perf_counter()
    assert res.aggregate_placebo_quality.shape[0] == 4
    off.append((t1 - t0) * 1e3)
    on.append((t2 - t1) * 1e3)
  report("pooled_placebo_off", off, note="placebo=True and aggregates, the pooled placebo stubbed out", **shape)
  report("pooled_placebo_on", on, **shape)
  sess, w = block_session(model, values, index, pre, post, a.draws, B)
  try:
    sess.run()
    prep, origins, horizon = w["prep"], w["origins"], w["horizon"]
    plan = dict(state=w["state"], origins=int(origins.shape[1]), horizon=int(horizon[0]), entries=int(w["csr"][0][-1]),
                kernel=sess.kernel_name())
    pooled = lambda: sess.pool_placebo_blocks(prep.outcome_sd, prep.outcome_mean, w["groups"], origins, int(horizon[0]), seen=w["seen"])   # pylint: disable=unnecessary-lambda-assignment
    single = lambda: sess.summarize_placebo_blocks(prep.outcome_sd, prep.outcome_mean, origins, horizon)   # pylint: disable=unnecessary-lambda-assignment
    pooled(), single()                                      # warm-up: the scratch
    times = ([], [])
    for _ in range(a.runs):
      for leg, call in enumerate((pooled, single)):
        t0 = time.perf_counter()
        call()
        times[leg].append((time.perf_counter() - t0) * 1e3)
    report("device_call", times[0], note="Session.pool_placebo_blocks with seen: one filter pass per chunk of entries, "
           "the accumulators, the three means", **shape, **plan)
    report("device_call_yardstick", times[1], note="Session.summarize_placebo_blocks, all three outputs (three filter "
           "passes over the series), same session", ratio_pooled_to_yardstick=statistics.median(times[0]) / statistics.median(times[1]),
           **shape, **plan)
    # the host twin on a stated share: the entries of the group of all series over the first `share`
    # series, `twin_origins` origins each -- nothing is scaled
    share, few = min(a.share, B), a.twin_origins
    out = sess.fetch(list(DRAWS))
    t0 = time.perf_counter()
    for b in range(share):
      lib._placebo_entry_host(w["inputs"][b], {k: out[k][b, 0] for k in DRAWS}, prep.outcome_sd[b],   # pylint: disable=protected-access
                              prep.outcome_mean[b], prep.observed[b], origins[b, :few], int(horizon[0]))
    host = (time.perf_counter() - t0) * 1e3
    report("numpy_share_filter", [host], note="lib._placebo_entry_host, the parent's filter of a pooled entry",
           share_entries=share, share_origins=few, per_entry_ms=host / share, **shape, state=w["state"], horizon=int(horizon[0]))
  finally:
    sess.close()
  if a.baseline_root:
    small = dict(shape, series=a.baseline_series, origins=a.baseline_origins)
    got = alternate(a, "package", a.baseline_runs,
                    ["--series", str(a.baseline_series), "--baseline-origins", str(a.baseline_origins)])
    for tree in ("parent", "branch"):
      times = [g["ms"] for t, _, g in got if t == tree]
      report("package_call_" + tree, times, note="fit_causalimpact_batch with placebo and aggregates, one child process "
             "per run after a warm-up without the pooled placebo, parent and branch alternating; REDUCED shape: "
             f"{a.baseline_series} series, {a.baseline_origins} origins", checksums=[g["checksum"] for t, _, g in got if t == tree],
             **small)
  if a.baseline_root and a.stock:
    got = alternate(a, "stock", 5, ["--series", str(B)])
    for tree, run, g in got:
      LINES.append(json.dumps(dict(tree=tree, run=run, leg=f"Session.summarize_placebo_blocks, {model}, {B} series, stock path", **g)))
    for tree in ("parent", "branch"):
      medians = [g["median_ms"] for t, _, g in got if t == tree]
      report("stock_path_" + tree, medians, note="the medians of the five runs above", model=model,
             min_ms=min(medians), max_ms=max(medians), checksums_equal=len({g["checksum"] for _, _, g in got}) == 1)
  with open(a.out, "a", encoding="utf-8") as f:
    f.write("\n".join(LINES) + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--seasons", choices=sorted(MODELS), default=None, help="a block list: the block-model route")
  ap.add_argument("--twin-origins", type=int, default=4, help="(--seasons) origins per entry of the numpy share")
  ap.add_argument("--baseline-root", default=None, help="(--seasons) a built checkout of the parent commit")
  ap.add_argument("--baseline-series", type=int, default=16)
  ap.add_argument("--baseline-origins", type=int, default=4)
  ap.add_argument("--baseline-runs", type=int, default=5)
  ap.add_argument("--stock", action="store_true", help="(--baseline-root) the stock path too, five runs of each tree")
  ap.add_argument("--root", default=ROOT, help="(child runs) the tree whose package is imported")
  ap.add_argument("--child", choices=("package", "stock"), default=None, help="(child runs) one run, one JSON line")
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
  a.out = a.out or os.path.join(ROOT, "profiles", "aggregate_placebo_blocks.jsonl" if blocks else "aggregate_placebo.jsonl")
  B, T = a.series, a.steps
  values = np.stack([np.column_stack(syn.make_raw_series(T, a.covariates, b)) for b in range(B)])
  index = pd.RangeIndex(T)
  pre, post = (0, int(0.7 * T) - 1), (int(0.7 * T), T - 1)
  if a.child:
    return (package_child if a.child == "package" else stock_child)(a, values, index, pre, post)
  if blocks:
    return blocks_main(a, values, index, pre, post)

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
