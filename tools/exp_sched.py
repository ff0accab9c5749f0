"""Experiment: kernel time of cfg2 for helper-wave schedule words (CI_DBG)."""
import os, sys, itertools
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tfp-causalimpact_amd")]
from causalimpact import _model, _native
from causalimpact import _synthetic as syn
y, mask, X, _ = syn.make_sampler_inputs(1000, 10, 2024)
spec = _model.series_params(y, mask, X, has_slope=True)
pb = _native.make_problem(T=1000, P=11, has_slope=1, num_warmup=112, num_results=1000, num_chains=8, seed=(0, 1))
params = _native.make_params([spec])
def word(p3, p4, pa, c3, c4, ca): return (p3 << 4) | (p4 << 6) | (pa << 8) | (c3 << 10) | (c4 << 12) | (ca << 14)
def timed(w, n):
  # the word is read when a session is created (ci_gibbs.hip plan_route): one session per word
  os.environ["CI_SCHED_WORD"] = str(w)
  sess = _native.Session(pb, y[None], mask[None], X[None], None, params)
  sess.run()
  ms = float(np.median([sess.run() for _ in range(n)]))
  sess.close()
  return ms
res = []
for p3, p4, pa, c3, c4, ca in itertools.product((2, 3), (0, 1, 2), (0, 1), (1, 2, 3), (0, 1, 2, 3), (0,)):
  res.append((timed(word(p3, p4, pa, c3, c4, ca), 3), (p3, p4, pa, c3, c4, ca)))
res.sort()
for ms, w in res[:15]: print(f"{ms:.3f} ms  p3,p4,pa,c3,c4,ca = {w}")
print("...")
for ms, w in res[-3:]: print(f"{ms:.3f} ms  {w}")
print("default", timed(0, 5))
