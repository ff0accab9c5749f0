"""What `fit_causalimpact_panel` buys: a 512-series panel (P = 6, lengths uniform in 257..512 -- one
steps-per-thread class --, own periods, 1 chain x 1000 draws as BASELINE cfg5) against
  (a) the same series fitted one by one with `fit_causalimpact` (what the panel replaces), and
  (b) `fit_causalimpact_batch` on 512 series of length 512 (the ceiling: same launch shape, no
      padding).
Every leg runs in a fresh child process under its own time limit; a leg that fails ends the script.
Prints one JSON line per leg (wall-clock ms of the whole call, data preparation and frames
included; retained draws per second) and a closing line with the three figures.

  python tools/exp_panel.py [--series 512] [--draws 1000] [--timeout 600]

--seasons N adds one seasonal block of N seasons (`Seasons(num_seasons=N)`; 7: daily data with a
weekly cycle) to the model and a cycle of that period to the data: the panel then takes the ragged
build of the time-parallel seasonal kernel, one launch per class of its grid.  The one-by-one leg
is left out in that mode (the comparison there is the same call on the parent commit, which runs
one session per distinct length).  --min-length / --max-length / --covariates / --chains change
the shape, e.g. the small panel `--series 8 --min-length 1000 --max-length 2000 --covariates 9
--chains 4`.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tfp-causalimpact_amd")):
  if p not in sys.path:
    sys.path.insert(0, p)


def _data(B, ragged, a):
  import numpy as np  # pylint: disable=import-outside-toplevel
  import pandas as pd  # pylint: disable=import-outside-toplevel
  from causalimpact import _synthetic as syn  # pylint: disable=import-outside-toplevel
  rng = np.random.default_rng(2024)
  lengths = rng.integers(a.min_length, a.max_length + 1, size=B) if ragged else np.full(B, a.max_length)
  frames, periods = [], []
  for b, T in enumerate(lengths):
    T = int(T)
    y, X = syn.make_raw_series(T, a.covariates, b)
    if a.seasons:
      y = y + 3.0 * np.sin(2 * np.pi * (np.arange(T) + b) / a.seasons)
    frames.append(pd.DataFrame(np.column_stack([y, X]), index=pd.RangeIndex(T),
                               columns=["y"] + [f"x{j}" for j in range(a.covariates)]))
    n_pre = int(0.7 * T)
    periods.append(((0, n_pre - 1), (n_pre, T - 1)))
  return frames, periods, lengths


def leg(name, a):
  import causalimpact as ci  # pylint: disable=import-outside-toplevel
  B, S = a.series, a.draws
  kw = dict(seed=1, inference_options=ci.InferenceOptions(num_results=S, num_chains=a.chains))
  if a.seasons:
    kw["model_options"] = ci.ModelOptions(seasons=[ci.Seasons(num_seasons=a.seasons)])
  frames, periods, lengths = _data(B, name != "batch", a)
  if name == "panel":
    run = lambda: ci.fit_causalimpact_panel(frames, periods, **kw).summary
  elif name == "batch":
    run = lambda: ci.fit_causalimpact_batch(frames, periods[0][0], periods[0][1], **kw).summary
  elif name == "single":
    def run():
      return [ci.fit_causalimpact(f, *p, **kw).summary for f, p in zip(frames, periods)]
    for f, p in list(zip(frames, periods))[:4]:            # warm-up: library load, first launches
      ci.fit_causalimpact(f, *p, **kw)
  else:
    raise SystemExit(f"unknown leg {name!r}")
  times = []
  for _ in range(1 if name == "single" else 3):            # (the first one-launch call warms up)
    t0 = time.perf_counter()
    run()
    times.append((time.perf_counter() - t0) * 1e3)
  ms = min(times)
  print(json.dumps({"leg": name, "series": B, "draws": S, "chains": a.chains, "seasons": a.seasons,
                    "covariates": a.covariates, "mean_length": float(lengths.mean()),
                    "wall_ms": ms, "all_wall_ms": times, "samples_per_s": B * S * a.chains / ms * 1e3}), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--leg", choices=("panel", "single", "batch"), default=None)
  ap.add_argument("--series", type=int, default=512)
  ap.add_argument("--draws", type=int, default=1000)
  ap.add_argument("--timeout", type=int, default=600, help="seconds per leg")
  ap.add_argument("--seasons", type=int, default=0, help="seasons of one seasonal block (0: trend model)")
  ap.add_argument("--min-length", type=int, default=257)
  ap.add_argument("--max-length", type=int, default=512)
  ap.add_argument("--covariates", type=int, default=5)
  ap.add_argument("--chains", type=int, default=1)
  a = ap.parse_args()
  if a.leg:
    leg(a.leg, a)
    return
  got = {}
  for name in ("panel", "batch") if a.seasons else ("panel", "batch", "single"):
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--leg", name,
           "--series", str(a.series), "--draws", str(a.draws), "--seasons", str(a.seasons),
           "--min-length", str(a.min_length), "--max-length", str(a.max_length),
           "--covariates", str(a.covariates), "--chains", str(a.chains)]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=False)
    sys.stdout.write(res.stdout)
    if res.returncode != 0:
      raise SystemExit(f"leg {name} ended with status {res.returncode}: stopping")
    got[name] = json.loads(res.stdout.strip().splitlines()[-1])
  out = {"panel_ms": got["panel"]["wall_ms"],
         "batch_of_%d_steps_ms" % a.max_length: got["batch"]["wall_ms"],
         "panel_vs_batch": got["panel"]["wall_ms"] / got["batch"]["wall_ms"],
         "mean_length_over_%d" % a.max_length: got["panel"]["mean_length"] / a.max_length}
  if "single" in got:
    out["one_by_one_ms"] = got["single"]["wall_ms"]
    out["panel_vs_one_by_one"] = got["single"]["wall_ms"] / got["panel"]["wall_ms"]
  print(json.dumps(out))


if __name__ == "__main__":
  main()
