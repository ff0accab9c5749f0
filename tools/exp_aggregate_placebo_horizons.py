"""What the pooled placebo forecasts at SEVERAL HORIZONS cost: at the shape of BASELINE cfg5 (512 series,
T = 500, 5 covariates, 1 chain x 1000 draws; four aggregates -- all series, two halves, a weighted
quarter: 1152 entries -- `--origins` 32, H = 116) the device call `Session.pool_placebo_horizons` with
`seen` on a finished session of the whole batch next to its yardstick, K calls of `Session.pool_placebo`
on the same session with the same origins (equal checksums asserted), for K = 8 and K = 16 horizons;
and `fit_causalimpact_batch` with `placebo=Placebo()` and with 8 and 16 horizons.  Medians of interleaved
rounds after one warm-up of each leg.

With `--seasons MODEL` (a block list as in tools/exp_aggregate_placebo.py) the same for a model the
one-lane filter does not take: 64 series (144 entries), `pool_placebo_horizons(blocks=True)` next to K
calls of `Session.pool_placebo_blocks`.

With `--baseline-root DIR` (a built checkout of the parent commit) the stock paths, parent and branch
alternating, one child process per run, `--baseline-runs` (5) runs of each: `Session.pool_placebo` and
`Session.summarize_placebo_horizons` (with `--seasons`: `Session.pool_placebo_blocks`), the median of
`--runs` calls per process and the checksum of the outputs; the ranges are reported side by side and the
checksums must be equal.

Lines are written to `--out` (default profiles/aggregate_placebo_horizons.jsonl, with `--seasons`
profiles/aggregate_placebo_horizons_blocks.jsonl): wall-clock ms of every run, their median and their
spread (max - min).

  python tools/exp_aggregate_placebo_horizons.py [--series 512] [--steps 500] [--covariates 5] [--draws 1000]
      [--origins 32] [--runs 5] [--skip-batch] [--baseline-root DIR] [--baseline-runs 5]
  python tools/exp_aggregate_placebo_horizons.py --seasons weekly+monthly|seasons52 [--series 64] ...
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


def horizons_of(count, H):
  """`count` horizons up to H, ascending, as `Placebo(horizons=count)` spaces them."""
  return np.array(sorted({max(1, (H * i) // count) for i in range(1, count + 1)}), np.int32)


def checksum(got):
  return float(sum(np.abs(v).sum() for v in got.values()))


def open_session(a, values, index, pre, post):
  """A finished session of the batch under the model of the run, and what its pooled calls need."""
  B = a.series
  mo = MODELS[a.seasons] if a.seasons else dict(local_linear_trend=False, seasons=[])
  prep = batch.prepare_batch(values[:B], index, pre, post)
  T, P = prep.y.shape[1], prep.design.shape[2]
  num_seasons, sc = _model.expand_seasons(mo["seasons"], T)
  hs = mo["local_linear_trend"]
  state = lib.prediction_state_dim(hs, num_seasons)
  params = [_model.series_params(prep.y[b], prep.mask[b], prep.design[b], has_slope=hs,
                                 num_seasonal_blocks=len(num_seasons),
                                 outcome_sd=float(np.nanstd(prep.y[b, :prep.num_pre], ddof=1))) for b in range(B)]
  n_post = int(np.count_nonzero(prep.flags & 2))
  origins, horizon = batch.placebo_plans(lib.Placebo(max_origins=a.origins), [prep.num_pre] * B, [n_post] * B, state)
  names, csr = batch.aggregate_groups(aggregates_of(B), range(B))
  groups = [dict(zip(csr[1][csr[0][g]:csr[0][g + 1]].tolist(), csr[2][csr[0][g]:csr[0][g + 1]].tolist()))
            for g in range(len(names))]
  pb = _native.make_problem(T=T, P=P, has_slope=hs, num_warmup=-(-a.draws // 9), num_results=a.draws,
                            num_series=B, seed=(0, 1), num_seasons=num_seasons)
  sess = _native.Session(pb, prep.y, prep.mask, prep.design, sc if len(num_seasons) else None, _native.make_params(params))
  sess.run()
  return sess, dict(prep=prep, origins=origins, horizon=horizon, groups=groups, entries=int(csr[0][-1]), state=state,
                    kernel=sess.kernel_name())


def device_legs(a, values, index, pre, post):
  """`pool_placebo_horizons` against K calls of `pool_placebo` (`pool_placebo_blocks`) on one session."""
  sess, w = open_session(a, values, index, pre, post)
  blocks = a.seasons is not None
  single = sess.pool_placebo_blocks if blocks else sess.pool_placebo
  try:
    prep, origins, H = w["prep"], w["origins"], int(w["horizon"][0])
    G, O = len(w["groups"]), origins.shape[1]
    shape = dict(model=a.seasons or "trend", series=a.series, steps=a.steps, covariates=a.covariates, draws=a.draws,
                 aggregates=G, entries=w["entries"], origins=int(O), horizon=H, state=w["state"], kernel=w["kernel"])
    for count in a.horizons:
      hz = horizons_of(count, H)
      K = len(hz)
      seen = 50.0 + np.arange(G * O * K, dtype=np.float64).reshape(G, O, K)

      def one_pass():
        return sess.pool_placebo_horizons(prep.outcome_sd, prep.outcome_mean, w["groups"], origins, hz, seen=seen,
                                          blocks=blocks)

      def k_calls():
        return [single(prep.outcome_sd, prep.outcome_mean, w["groups"], origins, int(h),
                       seen=np.ascontiguousarray(seen[:, :, k])) for k, h in enumerate(hz)]

      got, want = one_pass(), k_calls()                       # warm-up: the scratch; and the contract
      for k, one in enumerate(want):
        for name, v in one.items():
          assert np.array_equal(got[name][:, :, k], v), (count, k, name)
      # both checksums column by column in the same order, so that equal bits give equal sums
      sums = (float(sum(checksum({name: np.ascontiguousarray(got[name][:, :, k]) for name in one}) for k, one in enumerate(want))),
              float(sum(checksum(one) for one in want)))
      times = ([], [])
      for _ in range(a.runs):
        for leg, call in enumerate((one_pass, k_calls)):
          t0 = time.perf_counter()
          call()
          times[leg].append((time.perf_counter() - t0) * 1e3)
      ratio = statistics.median(times[1]) / statistics.median(times[0])
      report("one_pass", times[0], note="Session.pool_placebo_horizons with seen: one filter pass per chunk of entries",
             horizons=K, checksum=sums[0], **shape)
      report("k_calls", times[1], note=f"{K} calls of Session.{single.__name__} with seen, same session, same origins",
             horizons=K, checksum=sums[1], checksums_equal=sums[0] == sums[1], every_column_bit_equal=True,
             k_calls_over_one_pass=ratio, **shape)
  finally:
    sess.close()


def batch_legs(a, values, index, pre, post):
  """`fit_causalimpact_batch` with aggregates: `Placebo()` and with 8 and 16 horizons, interleaved."""
  B = a.series
  mo = ci.ModelOptions(**MODELS[a.seasons]) if a.seasons else ci.ModelOptions()
  options = [("placebo", ci.Placebo(max_origins=a.origins))] + [
      (f"placebo_{count}_horizons", ci.Placebo(max_origins=a.origins, horizons=count)) for count in a.horizons]

  def fit(placebo):
    return ci.fit_causalimpact_batch(values, pre, post, seed=1, index=index, placebo=placebo, aggregates=aggregates_of(B),
                                     model_options=mo, inference_options=ci.InferenceOptions(num_results=a.draws))

  for _, placebo in options:
    fit(placebo)                                              # warm-up: library load, scratch, pools
  times = {name: [] for name, _ in options}
  rows = {}
  for _ in range(a.runs):                                     # interleaved: drift hits all alike
    for name, placebo in options:
      t0 = time.perf_counter()
      res = fit(placebo)
      times[name].append((time.perf_counter() - t0) * 1e3)
      rows[name] = None if res.aggregate_placebo_profile is None else len(res.aggregate_placebo_profile)
  for name, _ in options:
    report("batch_" + name, times[name], profile_rows=rows[name], model=a.seasons or "trend", series=B, steps=a.steps,
           covariates=a.covariates, draws=a.draws, aggregates=4, origins=a.origins)


def stock_child(a, values, index, pre, post):
  """One process of the stock paths: the median of `--runs` calls of each and its checksum."""
  sess, w = open_session(a, values, index, pre, post)
  try:
    prep, origins, H = w["prep"], w["origins"], int(w["horizon"][0])
    G, O = len(w["groups"]), origins.shape[1]
    seen = 50.0 + np.arange(G * O, dtype=np.float64).reshape(G, O)
    if a.seasons:
      calls = {"pool_placebo_blocks": lambda: sess.pool_placebo_blocks(prep.outcome_sd, prep.outcome_mean, w["groups"],
                                                                       origins, H, seen=seen)}
    else:
      hz = horizons_of(8, H)
      calls = {"pool_placebo": lambda: sess.pool_placebo(prep.outcome_sd, prep.outcome_mean, w["groups"], origins, H, seen=seen),
               "summarize_placebo_horizons": lambda: sess.summarize_placebo_horizons(prep.outcome_sd, prep.outcome_mean,
                                                                                     origins, hz)}
    out = {}
    for name, call in calls.items():
      got = call()                                            # warm-up: the scratch
      times = []
      for _ in range(a.runs):
        t0 = time.perf_counter()
        got = call()
        times.append((time.perf_counter() - t0) * 1e3)
      out[name] = dict(median_ms=statistics.median(times), checksum=checksum(got))
    print(json.dumps(out), flush=True)
  finally:
    sess.close()


def stock_legs(a):
  """Parent and branch alternating, one child process per run."""
  got = []
  for run in range(1, a.baseline_runs + 1):
    for tree, root in (("parent", a.baseline_root), ("branch", ROOT)):
      cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--child", "--series", str(a.series),
             "--steps", str(a.steps), "--covariates", str(a.covariates), "--draws", str(a.draws),
             "--origins", str(a.origins), "--runs", str(a.runs)] + (["--seasons", a.seasons] if a.seasons else [])
      line = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1]
      got.append((tree, run, json.loads(line)))
      print(json.dumps(dict(progress=f"stock {tree} run {run}", **got[-1][2])), flush=True)
  for name in got[0][2]:
    sums = {g[name]["checksum"] for _, _, g in got}
    assert len(sums) == 1, (name, sums)
    for tree in ("parent", "branch"):
      medians = [g[name]["median_ms"] for t, _, g in got if t == tree]
      report(f"stock_{name}_{tree}", medians, note=f"Session.{name}: the medians of {a.runs} calls in each of "
             f"{a.baseline_runs} processes, parent and branch alternating", min_ms=min(medians), max_ms=max(medians),
             checksums_equal=True, model=a.seasons or "trend", series=a.series, origins=a.origins)
    parent = [g[name]["median_ms"] for t, _, g in got if t == "parent"]
    branch = statistics.median(g[name]["median_ms"] for t, _, g in got if t == "branch")
    LINES.append(json.dumps(dict(leg=f"stock_{name}_verdict", branch_median_ms=branch, parent_min_ms=min(parent),
                                 parent_max_ms=max(parent), branch_median_inside_parent_range=min(parent) <= branch <= max(parent))))
    print(LINES[-1], flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--seasons", choices=sorted(MODELS), default=None, help="a block list: the block-model route")
  ap.add_argument("--baseline-root", default=None, help="a built checkout of the parent commit: the stock paths")
  ap.add_argument("--baseline-runs", type=int, default=5)
  ap.add_argument("--root", default=ROOT, help="(child runs) the tree whose package is imported")
  ap.add_argument("--child", action="store_true", help="(child runs) one process of the stock paths, one JSON line")
  ap.add_argument("--series", type=int, default=None, help="512; 64 with --seasons")
  ap.add_argument("--steps", type=int, default=500)
  ap.add_argument("--covariates", type=int, default=5)
  ap.add_argument("--draws", type=int, default=1000)
  ap.add_argument("--origins", type=int, default=32)
  ap.add_argument("--horizons", type=int, nargs="+", default=[8, 16])
  ap.add_argument("--runs", type=int, default=5)
  ap.add_argument("--skip-batch", action="store_true")
  ap.add_argument("--skip-device", action="store_true")
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  a.series = a.series or (64 if a.seasons else 512)
  a.out = a.out or os.path.join(ROOT, "profiles", "aggregate_placebo_horizons_blocks.jsonl" if a.seasons
                                else "aggregate_placebo_horizons.jsonl")
  B, T = a.series, a.steps
  values = np.stack([np.column_stack(syn.make_raw_series(T, a.covariates, b)) for b in range(B)])
  index = pd.RangeIndex(T)
  pre, post = (0, int(0.7 * T) - 1), (int(0.7 * T), T - 1)
  if a.child:
    return stock_child(a, values, index, pre, post)
  if not a.skip_device:
    device_legs(a, values, index, pre, post)
  if not a.skip_batch:
    batch_legs(a, values, index, pre, post)
  if a.baseline_root:
    stock_legs(a)
  with open(a.out, "w", encoding="utf-8") as f:
    f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
  main()
