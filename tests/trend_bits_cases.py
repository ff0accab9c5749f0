"""Cases of tests/test_gpu_trend_kernel_bits.py and of the generator of its fixture
(tests/golden/trend_kernel_bits/make_trend_kernel_bits.py): one short fit per case through `_native.Session`, the
SHA-256 of every array `fetch()` returns, and the build `kernel_name()` reports.

Every non-instrumented build of the trend Gibbs kernels that the library holds and the routing can
reach is run at least once, for D in {1, 2} and L in {1, 2, 4, 8, 16} steps per thread:

  four     gibbs_kernel<D, L, PM>             PM 0, 1, 2 and -- L >= 8 -- 3 (CI_FLAG_FOUR_WAVES where
                                              the launch would otherwise take the eight-wave kernel)
  ragged   gibbs_kernel<D, L, PM, ragged>     the same, four series of their own lengths
  eight    gibbs_kernel8<D, L> (L <= 8), gibbs_kernel8<D, L, L2> (L >= 8)

Lengths: T = 100, 300, 1000, 1300, 4096 give the five L; T = 4094 is not a multiple of 4 (guarded
scalar rows wherever a row is read from global memory).  Columns: P = 0, 2, 11, 16, 17, 24, 33, 52
reach every branch of the regression block (none; register-resident; the one-wave LDS draw up to
31 columns; the all-wave draw), with the design in LDS or streamed as the LDS budget of that (P, L)
has it (45 instead of 52 at L = 16, the widest design the kernel's LDS layout takes there).  The
streamed builds are also run at the SMALLEST P that reaches them at their L
(make_layout's and Lay8's budgets: see STREAMED_FROM).
"""
import functools
import hashlib

import numpy as np

from causalimpact import _model
from causalimpact import _native
from causalimpact import _synthetic as syn

WARMUP, RESULTS, CHAINS, SEED = 8, 24, 2, (11, 7)
LENGTHS = (100, 300, 1000, 1300, 4096, 4094)
COLUMNS_FOUR = (0, 2, 11, 16, 17, 24, 33, 52)
COLUMNS_EIGHT = (2, 11, 16)
MAX_COLUMNS_L16 = 45
# smallest P at which kernel_name() reports the streamed build, read from a run of P = 1 .. 16
# per (D, L); absent: no P <= 16 reaches it at that L.  The test checks both sides of each boundary,
# so a moved LDS budget fails it instead of leaving a case that is no longer the smallest.
STREAMED_FROM = {
    "four": {(1, 8): 11, (2, 8): 11, (1, 16): 4, (2, 16): 4},          # gibbs_kernel<D, L, 3>
    "eight": {(1, 8): 13, (2, 8): 12, (1, 16): 1, (2, 16): 1},         # gibbs_kernel8<D, L, L2>
}
KINDS = ("four", "ragged", "eight")


def steps_per_thread(T):
  return next(L for L in (1, 2, 4, 8, 16) if 256 * L >= T)


def columns(kind, D, T):
  base = COLUMNS_EIGHT if kind == "eight" else COLUMNS_FOUR
  if kind != "eight" and steps_per_thread(T) == 16:
    # 16 steps per thread: the LDS layout of the four-wave kernel holds at most 45 columns (46 and
    # more are refused when the session is created) -- the widest design it takes stands in for 52
    base = tuple(min(P, MAX_COLUMNS_L16) for P in base)
  first = STREAMED_FROM["eight" if kind == "eight" else "four"].get((D, steps_per_thread(T)))
  return tuple(sorted(set(base) | ({first} if first is not None else set())))


def case_id(kind, D, T, P):
  return f"{kind}-D{D}-T{T}-P{P}"


def groups():
  """The parametrisation: (kind, D, T), each a handful of sessions of one L."""
  return [(k, D, T) for k in KINDS for D in (1, 2) for T in LENGTHS]


def expected_names():
  """Every build the cases must reach, as kernel_name() spells it."""
  names = set()
  for D in (1, 2):
    for L in (1, 2, 4, 8, 16):
      for pm in (0, 1, 2) + ((3,) if L >= 8 else ()):
        names.add(f"ci::gibbs_kernel<{D},{L},{pm},false>")
        names.add(f"ci::gibbs_kernel<{D},{L},{pm},false,ragged>")
      if L <= 8:
        names.add(f"ci::gibbs_kernel8<{D},{L}>")
      if L >= 8:
        names.add(f"ci::gibbs_kernel8<{D},{L},L2>")
  return names


def ragged_lengths(T):
  """T, T - 1, T - 37 and 3 T / 4 -- the last one raised to the shortest length of T's
  steps-per-thread class where it falls below it (T = 300, 1300): a ragged session takes series
  of one class only.  There T - 37 is the series that ends furthest below the stride."""
  L = steps_per_thread(T)
  return [T, T - 1, T - 37, max(3 * T // 4, 256 * (L // 2) + 1)]


@functools.lru_cache(maxsize=None)
def _series(T, P, b):
  y, mask, X, _ = syn.make_sampler_inputs(T, max(P - 1, 0), 100 + b)
  if P == 1:
    X = np.ones((T, 1))          # the intercept alone (the generator appends it to covariates only)
  return y, mask, X


def _spec(s, D):
  y, mask, X = s
  return _model.series_params(np.where(mask, np.nan, y), mask, X, has_slope=D == 2)


def _pad(arrs, T, fill):
  out = np.full((len(arrs), T) + arrs[0].shape[1:], fill, arrs[0].dtype)
  for b, a in enumerate(arrs):
    out[b, :a.shape[0]] = a
  return out


def _session(kind, D, T, P):
  four = kind == "four" and 0 < P <= 16
  if kind == "ragged":
    lengths = ragged_lengths(T)
    series = [_series(n, P, b) for b, n in enumerate(lengths)]
    pb = _native.make_problem(T=T, P=P, has_slope=D == 2, num_warmup=WARMUP, num_results=RESULTS,
                              num_chains=CHAINS, num_series=len(series), seed=SEED)
    X = None if P == 0 else _pad([s[2] for s in series], T, 7.5)        # (padding rows are never read)
    return _native.Session.ragged(pb, lengths, _pad([s[0] for s in series], T, np.nan),
                                  _pad([s[1] for s in series], T, True), X,
                                  _native.make_params([_spec(s, D) for s in series]),
                                  series_ids=list(range(len(series))))
  s = _series(T, P, 0)
  pb = _native.make_problem(T=T, P=P, has_slope=D == 2, num_warmup=WARMUP, num_results=RESULTS,
                            num_chains=CHAINS, seed=SEED,
                            flags=_native.FLAG_FOUR_WAVES if four else 0)
  return _native.Session(pb, s[0][None], s[1][None], None if P == 0 else s[2][None], None,
                         _native.make_params([_spec(s, D)]))


def route_name(kind, D, T, P):
  """The build a session of this case reports (nothing is run)."""
  sess = _session(kind, D, T, P)
  try:
    return sess.kernel_name()
  finally:
    sess.close()


def is_streamed(name):
  """gibbs_kernel<D, L, 3> or gibbs_kernel8<D, L, L2>: the design read from L2."""
  return ",3,false" in name or name.endswith(",L2>")


def run_case(kind, D, T, P):
  """(kernel name, {array name: sha256 of its bytes}) of one case; arrays without elements (the
  seasonal outputs of a trend model, the weights at P = 0) are left out."""
  sess = _session(kind, D, T, P)
  try:
    name = sess.kernel_name()
    sess.run()
    got = sess.fetch()
  finally:
    sess.close()
  return name, {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()
                for k, v in sorted(got.items()) if v.size}
