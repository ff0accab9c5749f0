"""The eight-wave Gibbs kernel's turn-around from (B5) to (B2) (csrc/ci_kernels8.h) against the
four-wave kernel, bit for bit, at every number of columns at which the split of X~'targets over
the helper waves takes another shape.

Between (B1) and (B2) the builds chosen by helpers_sum (two state components with one or four
steps per thread, one with two) let the four helper waves sum all P features -- the regression
wave floor(P / 4) of them, the randomness waves one more each while the remainder lasts, from
design rows they hold in registers, y'y with the last -- while the time waves sum only their
increments and fetch the normals of the window that follows.  A feature's sum does not depend on
who forms it (xt_sums_wave), so none of this may change a bit: the four-wave kernel
(CI_FLAG_FOUR_WAVES) gives each of its waves four features.  The other builds keep two slots per
wave over all eight waves and are pinned here too.

The issue's first row (T = 40, no covariate) has no design at all and is not dispatched to the
eight-wave kernel; its P = 1 is kept with a single covariate column instead (_inputs).
"""
import numpy as np
import pytest

from causalimpact import _native
from causalimpact import _synthetic as syn
from oracle import ci_oracle as orc

pytestmark = pytest.mark.gpu

CHAINS, SEED = 2, (6, 2)

# (T, p, has_slope, draws, data_seed): P = p + 1 columns
SHAPES = [
    (40, 0, 0, 60, 81),      # P = 1: one helper has work
    (64, 1, 1, 60, 82),      # P = 2
    (100, 3, 0, 60, 83),     # P = 4: one feature each
    (100, 4, 1, 60, 84),     # P = 5: a remainder of one
    (200, 8, 0, 60, 85),     # P = 9
    (300, 10, 1, 60, 86),    # P = 11, two steps per thread (two slots per wave kept)
    (1000, 10, 1, 60, 87),   # the headline build, four steps per thread
    (999, 12, 0, 60, 88),    # P = 13, T % 4 != 0
    (300, 15, 1, 60, 89),    # P = 16: every share full
    (1028, 5, 1, 30, 90),    # eight steps per thread: two slots per wave kept
    (1600, 12, 0, 20, 91),   # the design read from L2
    # the same numbers of columns in builds where the helper waves take the sums, whatever
    # helpers_sum leaves to the other builds above
    (40, 0, 1, 60, 93),      # P = 1
    (100, 3, 1, 60, 94),     # P = 4
    (200, 8, 1, 60, 95),     # P = 9
    (250, 12, 1, 60, 96),    # P = 13, T % 4 != 0
    (256, 15, 1, 60, 97),    # P = 16
    (1000, 15, 1, 30, 98),   # P = 16, four steps per thread: four rows held per wave
    (400, 5, 0, 60, 99),     # local level, two steps per thread
]


def _inputs(T, p, data_seed):
  """P = p + 1 columns.  With no covariate the synthetic inputs carry no design at all and the
  session takes the kernel without a regression block, so the P = 1 row keeps the single
  covariate of the one-covariate inputs and drops their intercept."""
  if p == 0:
    y, mask, X, _ = syn.make_sampler_inputs(T, 1, data_seed)
    return y, mask, np.ascontiguousarray(X[:, :1])
  y, mask, X, _ = syn.make_sampler_inputs(T, p, data_seed)
  return y, mask, X


def _run(y, mask, X, has_slope, draws, flags=0):
  spec = orc.default_spec(y, mask, X, has_slope=bool(has_slope))
  pb = _native.make_problem(T=len(y), P=X.shape[1], has_slope=has_slope, num_warmup=0,
                            num_results=draws, num_chains=CHAINS, seed=SEED, flags=flags)
  sess = _native.Session(pb, y[None], mask[None], X[None], None, _native.make_params([spec]))
  name = sess.kernel_name()
  sess.run()
  res = sess.fetch()
  sess.close()
  return name, res


def _assert_same_bits(y, mask, X, has_slope, draws):
  name8, eight = _run(y, mask, X, has_slope, draws)
  name4, four = _run(y, mask, X, has_slope, draws, _native.FLAG_FOUR_WAVES)
  assert "gibbs_kernel8" in name8
  assert "gibbs_kernel<" in name4
  assert set(eight) == set(four)
  for k, v in four.items():
    np.testing.assert_array_equal(eight[k], v, err_msg=k)
  w = eight["weights"][0]                                   # [chains, draws, P]
  assert np.isfinite(w).all() and (w != 0).any()


@pytest.mark.parametrize("T,p,has_slope,draws,data_seed", SHAPES)
def test_turnaround_of_the_eight_wave_kernel_has_the_bits_of_the_four_wave_kernel(
    T, p, has_slope, draws, data_seed):
  """Every output of every draw equal (the post-period of the synthetic inputs is missing)."""
  y, mask, X = _inputs(T, p, data_seed)
  assert mask.any()
  _assert_same_bits(y, mask, X, has_slope, draws)


def test_turnaround_with_the_first_observation_missing():
  """P = 11 with step 0 masked by hand: the first time thread's first target and increment."""
  y, mask, X = _inputs(300, 10, 92)
  mask = mask.copy()
  mask[0] = 1
  _assert_same_bits(y, mask, X, 1, 60)


def test_turnaround_does_not_depend_on_where_the_helper_work_is_scheduled(monkeypatch):
  """The helper waves reach (B1) with whatever their schedule left them: every step right after
  (Bs) ($CI_SCHED_WORD=1), every step after (B5) (2), the default quotas (0).  The word is read when
  a session is created: one session per word."""
  y, mask, X = _inputs(300, 10, 86)
  out = {}
  for word in ("0", "1", "2"):
    monkeypatch.setenv("CI_SCHED_WORD", word)
    name, out[word] = _run(y, mask, X, 1, 60)
    assert "gibbs_kernel8" in name
  for word in ("1", "2"):
    for k, v in out["0"].items():
      np.testing.assert_array_equal(out[word][k], v, err_msg=f"schedule {word}: {k}")
