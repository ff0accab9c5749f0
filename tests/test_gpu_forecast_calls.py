"""State between calls of the Kalman-filter entries of a session (csrc/ci_forecast.hip): prediction
errors, placebo, simulated placebo, pooled placebo and pooled simulated placebo share one call set-up
and the summary's scratch, so a call must not see what another one left there -- scale and shift, the
ranks, the regression term, the tables of a longer call.  Every comparison is bit for bit.

Sessions of 2 chains x 8 kept draws (N = 16), 3 warm-up iterations, P = 2 and a slope:
  one-lane: B = 3, T = 48, one block of 7 seasons (it takes the _blocks entries too);
  ragged:   lengths 48 and 41, trend only (the one-lane entries only);
  blocks:   B = 3, T = 48, the blocks 7 and 4 x 7: a state of 11 components (the _blocks entries only).
A twin is a session created and run again from the same inputs and seed."""
import functools

import numpy as np
import pytest

from causalimpact import _model
from causalimpact import _native

import test_gpu_placebo_simulated as base

pytestmark = pytest.mark.gpu

C_, S, SEED = 2, 8, (5, 9)
N = C_ * S
RANKS = [0, 7, 15]
FETCHED = base.PARAM_FIELDS + ["posterior_trajectories"]
# kind: (seasons as (num_seasons, num_steps_per_season), the series' lengths, ragged, the entries it admits)
KINDS = {
    "one-lane": (((7, 1),), (48, 48, 48), False, ("", "_blocks")),
    "ragged": ((), (48, 41), True, ("",)),
    "blocks": (((7, 1), (4, 7)), (48, 48, 48), False, ("_blocks",)),
}
LOG = (0.5, 2.0)                      # scale, shift of the simulated entries under LINK_LOG: z is O(1)
DATA = (3.7, -12.25)                  # scale, shift of the others


def _open(kind):
  """A finished session of the kind."""
  seasons, lengths, ragged, _ = KINDS[kind]
  series = [base._series(Tb, 2, 42 + 7 * b, True, seasons, b) for b, Tb in enumerate(lengths)]   # pylint: disable=protected-access
  T = max(lengths)
  num_seasons, sc = _model.expand_seasons(seasons, T)
  pb = _native.make_problem(T=T, P=2, has_slope=True, num_warmup=3, num_results=S, num_chains=C_,
                            num_series=len(lengths), seed=SEED, num_seasons=num_seasons)
  y = base._pad([s[0] for s in series], T, np.nan)                          # pylint: disable=protected-access
  mask = base._pad([s[1] for s in series], T, True)                         # pylint: disable=protected-access
  X = base._pad([s[2] for s in series], T, 7.5)                             # pylint: disable=protected-access
  params = _native.make_params([s[3] for s in series])
  sess = (_native.Session.ragged(pb, list(lengths), y, mask, X, params) if ragged
          else _native.Session(pb, y, mask, X, sc, params))
  sess.run()
  return sess


def _groups(B):
  """all (weights 1), the one member 1, a weighted pair: K = B + 3 entries, two chunks of a default call."""
  return [{b: 1.0 for b in range(B)}, {1: 1.0}, {0: 0.5, B - 1: 2.0}]


def _plan(B, O=3, T=48):
  """origins [B, O]: O = 3 the steps 3, 8, 20; O = 1 the step 8; O = T the step 3 and T - 1 unused slots."""
  row = {3: [3, 8, 20], 1: [8]}.get(O, [3] + [-1] * (T - 1))
  return np.array([row] * B, np.int32)


def _calls(kind):
  """name -> call(session): every entry the kind's session admits, with fixed arguments."""
  _, lengths, _, suffixes = KINDS[kind]
  B = len(lengths)
  org, H, groups = _plan(B), 5, _groups(B)
  seen, gseen, gcnt = np.full((B, 3), 20.0), np.full((3, 3), 20.0), np.ones((3, 3), np.int32)

  def of(sfx):
    return {
        "predictions" + sfx: lambda s: getattr(s, "summarize_predictions" + sfx)(*DATA, RANKS),
        "placebo" + sfx: lambda s: getattr(s, "summarize_placebo" + sfx)(*DATA, org, H),
        "simulated" + sfx: lambda s: getattr(s, "simulate_placebo" + sfx)(
            *LOG, org, H, _native.LINK_LOG, seen, RANKS, want=list(_native.PLACEBO_SIM_OUTPUTS)),
        "pooled" + sfx: lambda s: getattr(s, "pool_placebo" + sfx)(*DATA, groups, org, H, None, gseen),
        "pooled simulated" + sfx: lambda s: getattr(s, "pool_simulated_placebo" + sfx)(
            *LOG, groups, org, H, _native.LINK_LOG, None, gseen, gcnt, RANKS),
    }
  calls = {}
  for sfx in suffixes:
    calls.update(of(sfx))
  return calls


def _assert_same(got, want, what):
  assert list(got) == list(want), what
  for k in want:
    np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


@functools.lru_cache(maxsize=None)
def _alone(kind):
  """(the fetched draws of the kind's session, name -> the outputs of the entry called as the first and
  only call on a twin of its own); the twins' draws are checked to be the session's first."""
  first = _open(kind)
  try:
    draws = first.fetch(FETCHED)
  finally:
    first.close()
  out = {}
  for name, call in _calls(kind).items():
    twin = _open(kind)
    try:
      _assert_same(twin.fetch(FETCHED), draws, f"{kind}: the draws of the twin for {name}")
      out[name] = call(twin)
    finally:
      twin.close()
  return draws, out


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_entry_in_one_order_and_the_reverse_equals_its_call_alone_on_a_twin(kind):
  """(1)"""
  draws, alone = _alone(kind)
  calls = _calls(kind)
  sess = _open(kind)
  try:
    _assert_same(sess.fetch(FETCHED), draws, f"{kind}: the draws")
    forward = {name: call(sess) for name, call in calls.items()}
    backward = {name: calls[name](sess) for name in reversed(list(calls))}
  finally:
    sess.close()
  for name in calls:
    _assert_same(backward[name], forward[name], f"{kind} {name}: the second round against the first")
    _assert_same(forward[name], alone[name], f"{kind} {name}: among the others against alone on a twin")
    assert all(np.isfinite(v).all() for v in alone[name].values()), name


def _variations(kind, sfx):
  """name -> the calls of one entry: the first one, then others with O = 1 and O = T (one used slot per
  row), other ranks, another scale and shift and, for the simulated entries, another link."""
  B = len(KINDS[kind][1])
  groups, H = _groups(B), 5
  other = (1.5, 0.25)

  def seen(O, G=None):
    return np.full((G or B, O), 20.0)

  def cnt(O):
    return np.ones((3, O), np.int32)
  pred = lambda s, sc, rk: getattr(s, "summarize_predictions" + sfx)(*sc, rk)      # pylint: disable=unnecessary-lambda-assignment
  plac = lambda s, sc, O: getattr(s, "summarize_placebo" + sfx)(*sc, _plan(B, O), H)   # pylint: disable=unnecessary-lambda-assignment
  sim = lambda s, sc, O, rk, link: getattr(s, "simulate_placebo" + sfx)(           # pylint: disable=unnecessary-lambda-assignment
      *sc, _plan(B, O), H, link, seen(O), rk, want=list(_native.PLACEBO_SIM_OUTPUTS))
  pool = lambda s, sc, O: getattr(s, "pool_placebo" + sfx)(*sc, groups, _plan(B, O), H, None, seen(O, 3))   # pylint: disable=unnecessary-lambda-assignment
  psim = lambda s, sc, O, rk, link: getattr(s, "pool_simulated_placebo" + sfx)(    # pylint: disable=unnecessary-lambda-assignment
      *sc, groups, _plan(B, O), H, link, None, seen(O, 3), cnt(O), rk)
  log, ident = _native.LINK_LOG, _native.LINK_IDENTITY
  return {
      "predictions": [lambda s: pred(s, DATA, [0]), lambda s: pred(s, DATA, RANKS), lambda s: pred(s, other, [0])],
      "placebo": [lambda s: plac(s, DATA, 3), lambda s: plac(s, DATA, 1), lambda s: plac(s, DATA, 48),
                  lambda s: plac(s, other, 3)],
      "simulated": [lambda s: sim(s, LOG, 3, [0], log), lambda s: sim(s, LOG, 1, [0], log),
                    lambda s: sim(s, LOG, 48, [0], log), lambda s: sim(s, LOG, 3, RANKS, log),
                    lambda s: sim(s, other, 3, [0], log), lambda s: sim(s, LOG, 3, [0], ident)],
      "pooled": [lambda s: pool(s, DATA, 3), lambda s: pool(s, DATA, 1), lambda s: pool(s, DATA, 48),
                 lambda s: pool(s, other, 3)],
      "pooled simulated": [lambda s: psim(s, LOG, 3, [0], log), lambda s: psim(s, LOG, 1, [0], log),
                           lambda s: psim(s, LOG, 48, [0], log), lambda s: psim(s, LOG, 3, RANKS, log),
                           lambda s: psim(s, other, 3, [0], log), lambda s: psim(s, LOG, 3, [0], ident)],
  }


@pytest.mark.parametrize("kind,sfx", [("one-lane", ""), ("ragged", ""), ("blocks", "_blocks")])
def test_the_first_call_repeated_after_calls_with_other_arguments_returns_the_same_bits(kind, sfx):
  """(2)"""
  sess = _open(kind)
  try:
    for name, calls in _variations(kind, sfx).items():
      first = calls[0](sess)
      others = [call(sess) for call in calls[1:]]
      _assert_same(calls[0](sess), first, f"{kind} {name}{sfx}")
      # (the other calls did ask for something else)
      assert all(list(o) == list(first) for o in others)
      assert any(o[k].shape != first[k].shape or (o[k] != first[k]).any() for o in others for k in first), name
  finally:
    sess.close()


@pytest.mark.parametrize("kind,sfx", [("one-lane", ""), ("ragged", ""), ("blocks", "_blocks")])
def test_a_group_table_without_entries_returns_init_or_zeros_and_leaves_the_session_usable(kind, sfx):
  """(3): every member has the weight 0, so the table has no entry (K = 0) while P = 2 > 0: no regression
  launch, no filter launch.  The calls afterwards equal the twins' first calls."""
  _, alone = _alone(kind)
  calls = _calls(kind)
  B = len(KINDS[kind][1])
  empty = [{0: 0.0}, {b: 0.0 for b in range(B)}]
  assert _native.groups_csr(empty, B)[0].tolist() == [0, 0, 0]
  rng = np.random.default_rng(3)
  sess = _open(kind)
  try:
    for name, shape, extra in (("pooled", (2, 3, 2, N), ()), ("pooled simulated", (2, 3, N), (_native.LINK_LOG,))):
      entry = getattr(sess, {"pooled": "pool_placebo", "pooled simulated": "pool_simulated_placebo"}[name] + sfx)
      init = rng.normal(size=shape)
      got = entry(*DATA, empty, _plan(B), 5, *extra)
      assert list(got) == ["acc"] and got["acc"].shape == shape and (got["acc"] == 0.0).all(), name
      np.testing.assert_array_equal(entry(*DATA, empty, _plan(B), 5, *extra, init)["acc"], init, err_msg=name)
      _assert_same(calls[name + sfx](sess), alone[name + sfx], f"{kind} {name}{sfx} after the empty table")
    _assert_same(calls["predictions" + sfx](sess), alone["predictions" + sfx], f"{kind}: predictions afterwards")
  finally:
    sess.close()


@pytest.mark.parametrize("kind,sfx", [("one-lane", ""), ("ragged", ""), ("blocks", "_blocks")])
def test_a_call_that_asks_for_no_output_succeeds_and_the_next_call_is_unaffected(kind, sfx):
  """(4): every optional output pointer NULL (the pooled entries' `out` is no option: they return it)."""
  _, alone = _alone(kind)
  calls = _calls(kind)
  B = len(KINDS[kind][1])
  org, groups = _plan(B), _groups(B)
  nothing = {
      "predictions": lambda s: getattr(s, "summarize_predictions" + sfx)(*DATA, RANKS, want=[]),
      "placebo": lambda s: getattr(s, "summarize_placebo" + sfx)(*DATA, org, 5, want=[]),
      "simulated": lambda s: getattr(s, "simulate_placebo" + sfx)(*LOG, org, 5, _native.LINK_LOG, None, RANKS, want=[]),
      "pooled": lambda s: getattr(s, "pool_placebo" + sfx)(*DATA, groups, org, 5),
      "pooled simulated": lambda s: getattr(s, "pool_simulated_placebo" + sfx)(*LOG, groups, org, 5, _native.LINK_LOG),
  }
  sess = _open(kind)
  try:
    for name, call in nothing.items():
      got = call(sess)                                                       # (a failing entry raises NativeError)
      assert list(got) == (["acc"] if name.startswith("pooled") else []), name
      for after in calls:
        _assert_same(calls[after](sess), alone[after], f"{kind}: {after} after {name}{sfx} without outputs")
  finally:
    sess.close()
