"""The eight-wave Gibbs kernel's serial section (csrc/ci_kernels8.h, spike_slab_draw_pre) against
the four-wave kernel, bit for bit, at every size of the regression block where it takes another
path.

Between (B2) and (Bs) the regression wave alone is the critical path of an iteration.  Its
right-hand-side product runs as two chains (even and odd members of the included set).  With
more than 8 columns rows 0-1 of the wave's lanes run one, rows 2-3 the other, from a copy of the
swept block laid out by chain; up to 8 columns every lane runs both from the row-major copy; in
groups of four members either way, with the groups beyond P skipped.  The constants of the flip proposals
and the reciprocal that sigma^2_obs ends with are formed outside it.  None of this may change a
bit: the four-wave kernel (CI_FLAG_FOUR_WAVES) evaluates the same expressions in place, on one
wave.
"""
import numpy as np
import pytest

from causalimpact import _native
from causalimpact import _synthetic as syn
from oracle import ci_oracle as orc

pytestmark = pytest.mark.gpu

CHAINS, DRAWS, SEED = 2, 120, (6, 2)

# (T, p, has_slope, data_seed): P = p + 1 columns
SHAPES = [
    (40, 1, 0, 71),     # all features always in (no flip loop), P = 2
    (64, 3, 1, 72),     # P = 4: exactly one group of four
    (100, 4, 0, 73),    # P = 5: second group with one live row
    (100, 5, 1, 74),
    (200, 7, 0, 75),    # P = 8
    (120, 8, 1, 76),    # P = 9
    (300, 10, 1, 77),   # the headline configuration's P = 11
    (256, 12, 0, 78),   # P = 13
    (300, 15, 1, 79),   # P = 16: full
    (257, 15, 0, 80),   # P = 16, two steps per thread, T % 4 != 0
]


def _session(T, p, has_slope, data_seed, flags=0):
  y, mask, X, _ = syn.make_sampler_inputs(T, p, data_seed)
  spec = orc.default_spec(y, mask, X, has_slope=bool(has_slope))
  pb = _native.make_problem(T=T, P=p + 1, has_slope=has_slope, num_warmup=0, num_results=DRAWS,
                            num_chains=CHAINS, seed=SEED, flags=flags)
  return _native.Session(pb, y[None], mask[None], X[None], None, _native.make_params([spec]))


@pytest.mark.parametrize("T,p,has_slope,data_seed", SHAPES)
def test_serial_section_of_the_eight_wave_kernel_has_the_bits_of_the_four_wave_kernel(
    T, p, has_slope, data_seed):
  """Every output of every draw equal, and -- so that neither route of the serial section goes
  untested -- for P >= 4 at least 2 draws whose included set differs from the previous draw's (an
  accepted flip: further rounds of proposals, the un-sweep route of the weights) and at least 60
  whose set does not (the replay route: the weights drawn by a randomness wave).  The float64
  oracle on these inputs gives at least 5 changed and 145 unchanged draws at every shape."""
  out = {}
  for flags in (0, _native.FLAG_FOUR_WAVES):
    sess = _session(T, p, has_slope, data_seed, flags)
    name = sess.kernel_name()
    sess.run()
    out[flags] = (name, sess.fetch())
    sess.close()
  assert "gibbs_kernel8" in out[0][0]
  assert "gibbs_kernel<" in out[_native.FLAG_FOUR_WAVES][0]
  eight, four = out[0][1], out[_native.FLAG_FOUR_WAVES][1]
  assert set(eight) == set(four)
  for k, v in four.items():
    np.testing.assert_array_equal(eight[k], v, err_msg=k)
  w = eight["weights"][0]                                   # [chains, draws, P]
  assert np.isfinite(w).all() and (w != 0).any()
  if p + 1 >= 4:
    incl = w != 0
    changed = (incl[:, 1:] != incl[:, :-1]).any(axis=-1)    # [chains, draws - 1]
    n_changed, n_same = int(changed.sum()), int((~changed).sum())
    print(f"P={p + 1}: {n_changed} draws with a changed set, {n_same} with the same set")
    assert n_changed >= 2
    assert n_same >= 60


def test_serial_section_does_not_depend_on_where_the_helper_work_is_scheduled(monkeypatch):
  """What the serial section takes over from the iteration before -- the precompute's tables and
  registers, the randomness drawn ahead -- is the same wherever the helper waves' schedule places
  that work: every step right after (Bs) ($CI_SCHED_WORD=1), every step after (B5) (2), the default
  quotas (0).  The word is read when a session is created: one session per word."""
  out = {}
  for word in ("0", "1", "2"):
    monkeypatch.setenv("CI_SCHED_WORD", word)
    sess = _session(200, 7, 0, 75)
    assert "gibbs_kernel8" in sess.kernel_name()
    sess.run()
    out[word] = sess.fetch()
    sess.close()
  for word in ("1", "2"):
    for k, v in out["0"].items():
      np.testing.assert_array_equal(out[word][k], v, err_msg=f"schedule {word}: {k}")
