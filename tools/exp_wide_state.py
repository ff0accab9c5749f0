"""Per-iteration time of the multi-wavefront seasonal kernel (csrc/ci_seasonal_mw.h): 8 chains,
kernel only (HIP events of a session run), T = 1344 (eight weeks of hourly data), states of
72-256 components with P = 3 and P = 20 design columns.  Output: profiles/wide_state_times.txt."""
import sys

sys.path.insert(0, "tfp-causalimpact_amd"); sys.path.insert(0, ".")
from causalimpact import _model, _native  # noqa: E402
from causalimpact import _synthetic as syn  # noqa: E402

T, C, W, S = 1344, 8, 2, 8
# (name, has_slope, seasons): D_full = 72, 130, 170, 256
MODELS = (("Seasons(7) + Seasons(52, 7) + Seasons(12, 28)", 0, ((7, 1), (52, 7), (12, 28))),
          ("Seasons(128)", 1, ((128, 1),)),
          ("Seasons(168)", 1, ((168, 1),)),
          ("Seasons(254)", 1, ((254, 1),)))
print(f"T={T}, {C} chains, {W + S} iterations per run, best of 2 runs after a warm-up", flush=True)
for name, has_slope, seasons in MODELS:
  D = 1 + has_slope + sum(n for n, _ in seasons)
  for P in (3, 20):
    y, mask, X, _ = syn.make_sampler_inputs(T, P - 1, 2024)
    spec = _model.series_params(y, mask, X, num_seasonal_blocks=len(seasons), has_slope=bool(has_slope))
    counts, flg = _model.expand_seasons(seasons, T)
    pb = _native.make_problem(T=T, P=P, has_slope=has_slope, num_seasons=counts, num_warmup=W,
                              num_results=S, num_chains=C, seed=(0, 1))
    try:
      sess = _native.Session(pb, y[None], mask[None], X[None], flg, _native.make_params([spec]))
    except Exception as e:  # pylint: disable=broad-except
      print(f"D={D} P={P} {name}: not run: {e}", flush=True)
      continue
    sess.run()
    ms = min(sess.run() for _ in range(2))
    print(f"D={D} P={P} {name}: {sess.kernel_name()}  {ms / (W + S):.3f} ms per iteration", flush=True)
    sess.close()
