"""ci_session_pool_simulated_placebo and ci_session_pool_simulated_placebo_blocks on the device -- the
simulated totals of `simulate_placebo` of the members of every group, added draw by draw with the
group's weights -- against numpy's sum over the device's own per-series totals bit for bit, against the
numpy twins (`_placebo_simulated_host`, `pool_simulated_placebo_host`, `finish_simulated_placebo_host`)
at rtol 1e-8, atol 1e-8 (the project's float64 contract; all weights positive, so nothing cancels),
across chunks and sessions, against the analytic pooled placebo under the identity, and through
`fit_causalimpact_batch` / `fit_causalimpact_panel` with `Placebo(simulate=True, pool=True)`.

The shapes are those of tests/test_gpu_placebo_simulated.py, whose helpers this imports: T = 48 (60 for
the 52-season model), 2 chains x 37 draws (N = 74: a partial wavefront and a chain boundary), three
series with the ids 0, 1, 2, the steps 11 and 12 missing, the post-period masked, origins [3, 4, 8, 11,
20, T - H, -1], H in {1, 5, 9}.  Groups: `all` (weights 1), `one` = {1: 1.0}, `weighted` = {0: 0.5,
2: 2.0}: K = 6 entries against B = 3, so the default call already takes two chunks.  Member 2 of
`weighted` has an origin row of its own."""
import functools

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _native
from causalimpact import batch
from causalimpact import causalimpact_lib as lib

import test_gpu_placebo_simulated as base

pytestmark = pytest.mark.gpu

TOL = base.TOL
C_, S, N, SEED, RANKS, LINKS = base.C_, base.S, base.N, base.SEED, base.RANKS, base.LINKS
STATS = ("predicted_mean", "spread_mean", "below", "total_order")
# name: (has_slope, seasons as (num_seasons, num_steps_per_season), P, T, the block-model entry)
MODELS = {
    "level": (False, (), 0, 48, False),
    "level+slope+7": (True, ((7, 1),), 2, 48, False),
    "3+4 G=8": (False, ((3, 1), (4, 1)), 0, 48, True),
    "7+4x7 slope G=16": (True, ((7, 1), (4, 7)), 2, 48, True),
    "24 G=32": (False, ((24, 1),), 0, 48, True),
    "52 slope G=64": (True, ((52, 1),), 0, 60, True),
    "level+slope": (True, (), 2, 48, False),           # (the ragged session: trend models only)
}
GROUPS = [{0: 1.0, 1: 1.0, 2: 1.0}, {1: 1.0}, {0: 0.5, 2: 2.0}]      # all, one, weighted
CSR = _native.groups_csr(GROUPS, 3)
ENTRIES = [(g, int(b)) for g in range(3) for b in CSR[1][CSR[0][g]:CSR[0][g + 1]]]      # (group, member) per entry


def _open(name, lengths=None, ragged=False, only=None):
  """`base._open` for the models of this file."""
  saved = base.MODELS
  base.MODELS = MODELS
  try:
    return base._open(name, lengths, ragged, only)                           # pylint: disable=protected-access
  finally:
    base.MODELS = saved


def _rows(lengths, H):
  """The origin row of every entry, as one mapping per group: the series' own `base._origins`; member 2
  of `weighted` one step earlier wherever that is still a step in front of its neighbour."""
  rows = []
  for g, members in enumerate(GROUPS):
    rows.append({})
    for b in members:
      row = np.array(base._origins(lengths[b], H[g]), np.int32)             # pylint: disable=protected-access
      if g == 2 and b == 2:
        row = np.where(row >= 0, row - np.array([1, 0, 1, 1, 1, 1, 0]), -1).astype(np.int32)   # 2, 4, 7, 10, 19, T-H-1
      rows[g][b] = row
  return rows


def _counted(mask, row, H):
  return np.array([0 if o < 0 else int((~mask[o:o + H]).sum()) for o in row], np.int32)


def _entry(sess, blocks):
  return sess.pool_simulated_placebo_blocks if blocks else sess.pool_simulated_placebo


@functools.lru_cache(maxsize=None)
def _run(name, H, links=tuple(LINKS)):
  """One session of three series: its parameter draws and per link the members' own totals (one
  `simulate_placebo` call per distinct (origin row, horizon)), the pooled call without statistics,
  `seen` = draw 7's own pooled total, and the pooled call with every statistic."""
  blocks = MODELS[name][4]
  sess, inp = _open(name)
  try:
    sess.run()
    draws = sess.fetch(base.PARAM_FIELDS)
    Hg = np.array([H] * 3, np.int32)
    rows = _rows(inp["lengths"], Hg)
    counted = np.zeros((3, 7), np.int32)
    for g, b in ENTRIES:
      counted[g] += _counted(inp["mask"][b], rows[g][b], H)
    sim = sess.simulate_placebo_blocks if blocks else sess.simulate_placebo
    out = {}
    for link in links:
      code, scale, shift = LINKS[link]
      plain = sim(scale, shift, np.stack([rows[0][b] for b in range(3)]), H, code, None, RANKS, want=["totals"])["totals"]
      other = sim(scale, shift, np.stack([rows[0][0], rows[0][1], rows[2][2]]), H, code, None, RANKS,
                  want=["totals"])["totals"]
      totals = np.stack([other[b] if (g, b) == (2, 2) else plain[b] for g, b in ENTRIES])      # [K, O, N]
      acc = _entry(sess, blocks)(scale, shift, GROUPS, rows, Hg, code)
      assert list(acc) == ["acc"]
      seen = np.ascontiguousarray(acc["acc"][:, :, 7])
      got = _entry(sess, blocks)(scale, shift, GROUPS, rows, Hg, code, None, seen, counted, RANKS)
      out[link] = dict(got, totals=totals, seen=seen, per_series=plain)
    return dict(draws=draws, out=out, inp=inp, rows=rows, horizon=Hg, counted=counted, kernel=sess.kernel_name())
  finally:
    sess.close()


def _twin_totals(run, name, link):
  """[K, O, N]: `_placebo_simulated_host` of every entry's member at the entry's origins."""
  has_slope = MODELS[name][0]
  inp = run["inp"]
  code, scale, shift = LINKS[link]
  out = []
  for g, b in ENTRIES:
    Tb = inp["lengths"][b]
    out.append(lib._placebo_simulated_host(                                  # pylint: disable=protected-access
        inp["y"][b, :Tb], inp["mask"][b, :Tb], None if inp["X"] is None else inp["X"][b, :Tb], inp["sc"][:, :Tb],
        inp["num_seasons"], has_slope, inp["specs"][b], base._pooled(run["draws"], b), scale, shift,   # pylint: disable=protected-access
        run["rows"][g][b], int(run["horizon"][g]), code, lib.placebo_stream(SEED, inp["ids"][b], range(C_)))["totals"])
  return np.stack(out)


CASES = [(name, H) for name in MODELS if name != "level+slope" for H in (1, 5, 9)]


@pytest.mark.parametrize("name,H", CASES)
def test_the_sums_equal_numpy_over_the_devices_own_totals_bit_for_bit(name, H):
  """(1), (3), (4): acc = acc + w * t in numpy over `simulate_placebo`'s totals; the group of one member
  of weight 1 is that member's own row; the statistics are numpy's on the device's own sums."""
  run = _run(name, H)
  for link, got in run["out"].items():
    np.testing.assert_array_equal(got["acc"], _native.pool_simulated_placebo_host(got["totals"], CSR), err_msg=link)
    np.testing.assert_array_equal(got["acc"][1], got["per_series"][1], err_msg=link)
    want = _native.finish_simulated_placebo_host(got["acc"], got["seen"], run["counted"], RANKS)
    for k in STATS:
      np.testing.assert_array_equal(got[k], want[k], err_msg=f"{link} {k}")
    # a window no member counts a step of, and the unused slot, read 0 everywhere
    empty = run["counted"] == 0
    assert empty[:, -1].all() and (H > 1 or empty[1, 3])
    for k in STATS + ("acc",):
      rows = np.moveaxis(got[k], 1, 2)[empty] if k == "total_order" else got[k][empty]
      assert (rows == 0.0).all(), (k, link)
    some = ~empty
    assert (got["below"][some] >= 1).all() and (got["below"][some] < N).any()     # (draw 7 ties with `seen`)


@pytest.mark.parametrize("name,H", [("level", 5), ("level+slope+7", 9), ("3+4 G=8", 5), ("7+4x7 slope G=16", 9)])
def test_the_group_of_one_member_equals_simulate_placebo_in_every_statistic(name, H):
  """(3): group `one` against `simulate_placebo`'s row of series 1 with the group's `seen`, bit for bit."""
  blocks = MODELS[name][4]
  run = _run(name, H)
  sess, _ = _open(name)
  try:
    sess.run()
    for link, got in run["out"].items():
      code, scale, shift = LINKS[link]
      seen = np.zeros((3, 7))
      seen[1] = got["seen"][1]
      one = sess.simulate_placebo(scale, shift, np.stack([run["rows"][0][b] for b in range(3)]), H, code, seen, RANKS,
                                  want=list(_native.PLACEBO_SIM_OUTPUTS), blocks=blocks)
      np.testing.assert_array_equal(got["acc"][1], one["totals"][1], err_msg=link)
      for k in STATS:
        np.testing.assert_array_equal(got[k][1], one[k][1], err_msg=f"{link} {k}")
  finally:
    sess.close()


@pytest.mark.parametrize("name,H", CASES)
def test_sums_and_statistics_equal_the_twins_pooled_by_the_host_twin(name, H):
  """(2): `below` may differ by the number of pooled totals of the twin within TOL of `seen`; `seen`
  is draw 7's own pooled total, so exactly one such tie is expected per window."""
  run = _run(name, H)
  for link, got in run["out"].items():
    acc = _native.pool_simulated_placebo_host(_twin_totals(run, name, link), CSR)
    dev = float(np.abs(got["acc"] - acc).max())
    print(f"{name} H={H} [{run['kernel']}] {link}: largest deviation of a pooled total {dev:.2e}, "
          f"largest pooled total {np.abs(acc).max():.3g}")
    np.testing.assert_allclose(got["acc"], acc, err_msg=link, **TOL)
    want = _native.finish_simulated_placebo_host(acc, got["seen"], run["counted"], RANKS)
    for k in ("predicted_mean", "spread_mean", "total_order"):
      np.testing.assert_allclose(got[k], want[k], err_msg=f"{link} {k}", **TOL)
    seen = got["seen"][:, :, None]
    near = np.where(run["counted"] > 0,
                    np.count_nonzero(np.abs(acc - seen) <= TOL["atol"] + TOL["rtol"] * np.abs(seen), axis=2), 0)
    print(f"{name} H={H} {link}: pooled totals within TOL of `seen` per window, at most {near.max()}")
    assert (near <= 1).all()
    assert (np.abs(got["below"] - want["below"]) <= near).all()


@pytest.mark.parametrize("name", ["level+slope+7", "3+4 G=8", "52 slope G=64"])
def test_every_chunk_size_gives_the_same_bits(name):
  """(5): chunk_entries 1, 2 and B against the default call (two chunks of B = 3 and 3 entries)."""
  blocks = MODELS[name][4]
  run = _run(name, 5)
  sess, _ = _open(name)
  try:
    sess.run()
    for link in ("log", "identity"):
      code, scale, shift = LINKS[link]
      want = run["out"][link]
      for chunk in (1, 2, 3):
        got = sess.pool_simulated_placebo(scale, shift, GROUPS, run["rows"], run["horizon"], code, None, want["seen"],
                                          run["counted"], RANKS, blocks=blocks, chunk_entries=chunk)
        for k in STATS + ("acc",):
          np.testing.assert_array_equal(got[k], want[k], err_msg=f"{link} chunk_entries={chunk} {k}")
  finally:
    sess.close()


@pytest.mark.parametrize("name", ["level+slope+7", "7+4x7 slope G=16"])
def test_sessions_of_one_series_each_hand_the_sums_on_to_the_bits_of_one_session(name):
  """(6): series b alone at series_offset b; `out` handed on as `init`; then a finish-only call."""
  blocks = MODELS[name][4]
  run = _run(name, 9)
  acc = {link: None for link in LINKS}
  last = None
  for b in range(3):
    sess, _ = _open(name, only=b)
    try:
      sess.run()
      groups = [({0: w[b]} if b in w else {}) for w in GROUPS]
      rows = [({0: run["rows"][g][b]} if b in w else {}) for g, w in enumerate(GROUPS)]
      for link in LINKS:
        code, scale, shift = LINKS[link]
        acc[link] = _entry(sess, blocks)(scale, shift, groups, rows, run["horizon"], code, acc[link])["acc"]
      if b == 2:
        for link in LINKS:
          code, scale, shift = LINKS[link]
          want = run["out"][link]
          np.testing.assert_array_equal(acc[link], want["acc"], err_msg=link)
          last = _entry(sess, blocks)(scale, shift, [{}] * 3, np.full((1, 7), -1, np.int32), 1, code, acc[link],
                                      want["seen"], run["counted"], RANKS)
          for k in STATS + ("acc",):
            np.testing.assert_array_equal(last[k], want[k], err_msg=f"finish only {link} {k}")
    finally:
      sess.close()
  assert last is not None


def test_a_ragged_session_pools_the_members_own_session_totals_bit_for_bit():
  """(7): lengths 70, 41 and 64 in one ragged launch, every entry with its own origins, every group
  with its own horizon (9, 1, 5); each member alone on its own length gives the totals that are pooled."""
  lengths, Hg = (70, 41, 64), np.array([9, 1, 5], np.int32)
  rows = _rows(lengths, Hg)
  totals = {}
  for b in range(3):
    one, _ = _open("level+slope", lengths=lengths, ragged=True, only=b)
    try:
      one.run()
      for g, members in enumerate(GROUPS):
        if b in members:
          for link, (code, scale, shift) in LINKS.items():
            totals[link, g, b] = one.simulate_placebo(scale, shift, rows[g][b][None], int(Hg[g]), code, None, RANKS,
                                                      want=["totals"])["totals"][0]
    finally:
      one.close()
  sess, inp = _open("level+slope", lengths=lengths, ragged=True)
  try:
    sess.run()
    assert "ragged" in sess.kernel_name()
    counted = np.zeros((3, 7), np.int32)
    for g, b in ENTRIES:
      counted[g] += _counted(inp["mask"][b, :lengths[b]], rows[g][b], int(Hg[g]))
    for link, (code, scale, shift) in LINKS.items():
      want = _native.pool_simulated_placebo_host(np.stack([totals[link, g, b] for g, b in ENTRIES]), CSR)
      seen = np.ascontiguousarray(want[:, :, 7])
      got = sess.pool_simulated_placebo(scale, shift, GROUPS, rows, Hg, code, None, seen, counted, RANKS)
      np.testing.assert_array_equal(got["acc"], want, err_msg=link)
      stats = _native.finish_simulated_placebo_host(want, seen, counted, RANKS)
      for k in STATS:
        np.testing.assert_array_equal(got[k], stats[k], err_msg=f"{link} {k}")
    with pytest.raises(_native.NativeError, match="ci_session_pool_simulated_placebo_blocks takes no ragged session"):
      sess.pool_simulated_placebo_blocks(1.0, 0.0, GROUPS, rows, Hg, 0)
    with pytest.raises(_native.NativeError, match=r"group 1, entry 3 \(member 1\): the origin 40 of slot 5 with horizon 2 "
                                                  r"reaches beyond the series' 41 steps"):
      sess.pool_simulated_placebo(1.0, 0.0, GROUPS, rows, [9, 2, 5], 0)
  finally:
    sess.close()


@pytest.mark.parametrize("name", ["level+slope+7", "7+4x7 slope G=16"])
def test_the_other_entries_of_the_session_return_the_same_bits_before_and_after(name):
  """(8): the scratch is shared with `simulate_placebo` and `pool_placebo`."""
  blocks = MODELS[name][4]
  sess, inp = _open(name)
  try:
    sess.run()
    code, scale, shift = LINKS["log"]
    Hg = np.array([5] * 3, np.int32)
    rows = _rows(inp["lengths"], Hg)
    per_series = np.stack([rows[0][b] for b in range(3)])

    def others():
      sim = sess.simulate_placebo(scale, shift, per_series, 5, code, np.full((3, 7), 20.0), RANKS,
                                  want=list(_native.PLACEBO_SIM_OUTPUTS), blocks=blocks)
      pool = (sess.pool_placebo_blocks if blocks else sess.pool_placebo)(3.7, -12.25, GROUPS, rows, Hg, None,
                                                                        np.full((3, 7), 1.0))
      return {**{"sim " + k: v for k, v in sim.items()}, **{"pool " + k: v for k, v in pool.items()}}
    before = others()
    first = _entry(sess, blocks)(scale, shift, GROUPS, rows, Hg, code, None, np.full((3, 7), 20.0),
                                 np.ones((3, 7), np.int32), RANKS)
    after = others()
    again = _entry(sess, blocks)(scale, shift, GROUPS, rows, Hg, code, None, np.full((3, 7), 20.0),
                                 np.ones((3, 7), np.int32), RANKS)
    for k in before:
      np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    for k in first:
      np.testing.assert_array_equal(again[k], first[k], err_msg=k)
  finally:
    sess.close()


@pytest.mark.parametrize("name,H", [("level+slope+7", 9), ("7+4x7 slope G=16", 5)])
def test_under_the_identity_the_mean_is_the_analytic_pooled_placebos_within_its_monte_carlo_error(name, H):
  """(9): given draw n the pooled total is N(S_n, U_n) with independent members, so the mean over the
  draws of one pooled simulated total each differs from the mean of S by a variable of standard
  deviation sqrt(mean_n(U) / N); five of them over about 20 windows fail with probability below 1e-5."""
  blocks = MODELS[name][4]
  code, scale, shift = LINKS["identity"]
  run = _run(name, H)
  sess, _ = _open(name)
  try:
    sess.run()
    ana = (sess.pool_placebo_blocks if blocks else sess.pool_placebo)(scale, shift, GROUPS, run["rows"], run["horizon"],
                                                                      None, np.zeros((3, 7)))
  finally:
    sess.close()
  sim = run["out"]["identity"]["predicted_mean"]
  bound = 5.0 * np.sqrt(ana["acc"][:, :, 1].mean(axis=2) / N)
  some = run["counted"] > 0
  print(f"{name}: |sim - analytic| / bound =", (np.abs(sim - ana["predicted_mean"]) / np.where(bound > 0, bound, 1.0))[some])
  assert (np.abs(sim - ana["predicted_mean"]) <= bound).all()
  assert (sim[some] != ana["predicted_mean"][some]).all()                     # (a simulation, not the moments)


def test_errors_are_reported_before_any_device_work():
  """(10)"""
  sess, _ = _open("level")
  good = np.array([[3, 9], [3, -1], [3, 9]], np.int32)
  seen, cnt = np.zeros((3, 2)), np.ones((3, 2), np.int32)
  call = lambda *a, **k: sess.pool_simulated_placebo(1.0, 0.0, *a, **k)   # pylint: disable=unnecessary-lambda-assignment
  try:
    with pytest.raises(_native.NativeError, match="ci_session_pool_simulated_placebo needs a finished ci_session_run"):
      call(GROUPS, good, 5, 0)
    sess.run()
    fn = _native.load().ci_session_pool_simulated_placebo
    one, hz, rk, out = np.ones(3), np.full(3, 5, np.int32), np.zeros(1, np.int32), np.zeros((3, 2, N))
    org = np.ascontiguousarray(good[CSR[1]])
    ptr = lambda a: None if a is None else a.ctypes.data   # pylint: disable=unnecessary-lambda-assignment
    full = dict(scale=one, shift=one, offsets=CSR[0], members=CSR[1], weights=CSR[2], origins=org, horizon=hz, out=out,
                ranks=rk)
    for missing in full:
      a = dict(full, **{missing: None})
      rc = fn(sess._h, ptr(a["scale"]), ptr(a["shift"]), 3, ptr(a["offsets"]), ptr(a["members"]), ptr(a["weights"]), 2,   # pylint: disable=protected-access
              ptr(a["origins"]), ptr(a["horizon"]), 0, None, ptr(a["out"]), None, None, 1, ptr(a["ranks"]),
              None, None, None, None)
      assert rc != 0 and "NULL argument" in _native.load().ci_last_error().decode(), missing
    # no statistic without both `seen` and `counted`
    stat = np.zeros((3, 2))
    for s_, c_ in ((None, cnt), (seen, None), (None, None)):
      rc = fn(sess._h, ptr(one), ptr(one), 3, ptr(CSR[0]), ptr(CSR[1]), ptr(CSR[2]), 2, ptr(org), ptr(hz), 0, None,   # pylint: disable=protected-access
              ptr(out), ptr(s_), ptr(c_), 1, ptr(rk), ptr(stat), None, None, None)
      assert rc != 0 and "need `seen` and `counted`" in _native.load().ci_last_error().decode()
    with pytest.raises(ValueError, match="`seen` and `counted` go together"):
      call(GROUPS, good, 5, 0, None, seen)
    for link in (-1, 3):
      with pytest.raises(_native.NativeError, match=f"link must be CI_LINK_IDENTITY, CI_LINK_LOG or CI_LINK_LOG1P .*got {link}"):
        call(GROUPS, good, 5, link)
    for ranks in ([], list(range(9))):
      with pytest.raises(_native.NativeError, match=rf"num_ranks must be in \[1, 8\], got {len(ranks)}"):
        call(GROUPS, good, 5, 0, None, seen, cnt, ranks)
    with pytest.raises(_native.NativeError, match=rf"rank {N} out of range \[0, {N}\)"):
      call(GROUPS, good, 5, 0, None, seen, cnt, [N])
    for chunk in (0, 4):
      with pytest.raises(_native.NativeError, match=rf"chunk_entries must be in \[1, 3\] \(the session's series\), got {chunk}"):
        call(GROUPS, good, 5, 0, chunk_entries=chunk)
    # the checks of the analytic pooled entry, with its messages
    with pytest.raises(_native.NativeError, match=r"max_origins must be in \[1, 48\], got 49"):
      call(GROUPS, np.full((3, 49), -1), 5, 0)
    with pytest.raises(_native.NativeError, match="group 1: the horizon must be at least 1, got 0"):
      call(GROUPS, good, [5, 0, 5], 0)
    with pytest.raises(_native.NativeError, match=r"group 0, entry 1 \(member 1\): the origins must be strictly ascending"):
      call(GROUPS, [[3, 9], [3, 3], [3, 9]], 5, 0)
    with pytest.raises(_native.NativeError, match=r"group 2, entry 5 \(member 2\): slot 0 must hold a step or -1"):
      call(GROUPS, [{0: [3], 1: [3], 2: [3]}, {1: [3]}, {0: [3], 2: [-2]}], 5, 0)
    with pytest.raises(_native.NativeError, match=r"group 0, entry 0 \(member 0\): the origin 44 of slot 1 with horizon 5 "
                                                  r"reaches beyond the series' 48 steps"):
      call(GROUPS, [[3, 44], [3, -1], [3, 9]], 5, 0)
    with pytest.raises(_native.NativeError, match="group 0: member 3 out of range"):
      sess.pool_simulated_placebo(1.0, 0.0, (np.array([0, 1], np.int32), np.array([3], np.int32), np.ones(1)),
                                  [{3: [3]}], 5, 0)
    with pytest.raises(ValueError, match=rf"`init` must be \[3, 2, {N}\]"):
      call(GROUPS, good, 5, 0, np.zeros((3, 2, 2, N)))
    with pytest.raises(ValueError, match=r"`counted` must be \[3, 2\]"):
      call(GROUPS, good, 5, 0, None, seen, np.ones((3, 3), np.int32))
    with pytest.raises(ValueError, match="unknown pooled simulated placebo outputs"):
      call(GROUPS, good, 5, 0, None, seen, cnt, [0], want=["pit_mean"])
    # (the block entry takes this session too; without `seen` only the sums come back)
    assert list(sess.pool_simulated_placebo_blocks(1.0, 0.0, GROUPS, good, 5, 0)) == ["acc"]
    assert sess.pool_simulated_placebo_blocks(1.0, 0.0, GROUPS, good, 5, 0, None, seen, cnt, [0])["total_order"].shape == (3, 1, 2)
  finally:
    sess.close()
  two, _ = _open("24 G=32")
  try:
    two.run()
    with pytest.raises(_native.NativeError, match=r"ci_session_pool_simulated_placebo takes a trend with at most "
                                                  r"one block of 2 to 7 seasons.*\(24\)"):
      two.pool_simulated_placebo(1.0, 0.0, GROUPS, good, 5, 0)
  finally:
    two.close()


# ---- package level: Placebo(simulate=True, pool=True) under a log link -----------------------------------

ALPHA, FIT_SEED, OPTS = base.ALPHA, base.FIT_SEED, base.OPTS
POOL = ci.Placebo(max_origins=6, simulate=True, pool=True)
AGGREGATES = {"all": "all", "one": [1], "weighted": {0: 0.5, 2: 2.0}}
NUMERIC = base.NUMERIC


def _without_device_entries(monkeypatch):
  """The host route of the pooled simulated placebo: the session loses the two entries."""
  monkeypatch.delattr(_native.Session, "pool_simulated_placebo")
  monkeypatch.delattr(_native.Session, "pool_simulated_placebo_blocks")


def _pooled_near(monkeypatch):
  """Counts, on the host route, the pooled totals within TOL of the pooled observed total per window."""
  near = []
  twin = batch.SimulatedPool.finish_host

  def spy(self, acc, seen, counted):
    s_ = np.asarray(seen, np.float64)[..., None]
    near.append(np.where(np.asarray(counted) > 0,
                         np.count_nonzero(np.abs(acc - s_) <= TOL["atol"] + TOL["rtol"] * np.abs(s_), axis=-1), 0))
    return twin(self, acc, seen, counted)
  monkeypatch.setattr(batch.SimulatedPool, "finish_host", spy)
  return near


def _assert_aggregates_agree(got, want, near, what):
  assert list(got.aggregates) == list(want.aggregates) == list(AGGREGATES)
  for g, name in enumerate(AGGREGATES):
    a, b = got.aggregates[name].placebo, want.aggregates[name].placebo
    assert list(a.columns) == list(lib.PLACEBO_COLUMNS + lib.PLACEBO_SIMULATED_COLUMNS), (what, name)
    assert a.index.equals(b.index) and len(a) >= 3
    print(what, name, "largest deviation per column:", (a[NUMERIC] - b[NUMERIC]).abs().max().to_dict(),
          "pooled totals within TOL of `seen`:", int(near[g].max()))
    np.testing.assert_allclose(a[NUMERIC].to_numpy(np.float64), b[NUMERIC].to_numpy(np.float64),
                               err_msg=f"{what} {name}", **TOL)
    assert list(a["horizon_end"]) == list(b["horizon_end"])
    # (the allowance of tests/test_gpu_placebo_simulated.py: none, the data have no tie)
    assert near[g].max() == 0, "choose other data: a pooled total of the twin ties with the observed one"
    np.testing.assert_allclose(a["pit"], b["pit"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(a["p"], b["p"], rtol=0, atol=1e-15)
    assert list(a["significant"]) == list(b["significant"])
    assert ((a["pit"] > 0) & (a["pit"] < 1)).all() and (a["predicted_lower"] < a["predicted_upper"]).all()
    np.testing.assert_allclose(got.aggregates[name].placebo_quality.to_numpy(),
                               want.aggregates[name].placebo_quality.to_numpy(), **TOL)
  np.testing.assert_allclose(got.aggregate_placebo_quality.to_numpy(), want.aggregate_placebo_quality.to_numpy(), **TOL)
  assert list(got.aggregate_placebo_quality.index) == list(AGGREGATES)


def test_batch_aggregates_on_the_device_equal_the_host_route_and_disturb_nothing(monkeypatch):
  """(11), batch."""
  frames = base._frames()                                                    # pylint: disable=protected-access
  periods = base._periods(frames[0], 0)                                      # pylint: disable=protected-access
  kw = dict(alpha=ALPHA, seed=FIT_SEED, outcome_link="log", inference_options=ci.InferenceOptions(**OPTS))
  on = ci.fit_causalimpact_batch(frames, *periods, placebo=POOL, aggregates=AGGREGATES, **kw)
  assert type(on) is ci.CausalImpactBatchAnalysis                          # (the one-launch route)
  sim = ci.fit_causalimpact_batch(frames, *periods, placebo=base.SIM, **kw)
  off = ci.fit_causalimpact_batch(frames, *periods, aggregates=AGGREGATES, **kw)
  for b in range(3):
    pd.testing.assert_frame_equal(on[b].placebo, sim[b].placebo, check_exact=True)
    pd.testing.assert_frame_equal(on[b].series, off[b].series, check_exact=True)
  pd.testing.assert_frame_equal(on.placebo_quality, sim.placebo_quality, check_exact=True)
  pd.testing.assert_frame_equal(on.summary, off.summary, check_exact=True)
  assert off.aggregate_placebo_quality is None and sim.aggregate_placebo_quality is None
  for name in AGGREGATES:
    assert off.aggregates[name].placebo is None and off.aggregates[name].placebo_quality is None
    pd.testing.assert_frame_equal(on.aggregates[name].series, off.aggregates[name].series, check_exact=True)
    pd.testing.assert_frame_equal(on.aggregates[name].summary, off.aggregates[name].summary, check_exact=True)
  # the group of one member of weight 1 is that member's own simulated placebo
  pd.testing.assert_frame_equal(on.aggregates["one"].placebo[NUMERIC], on[1].placebo[NUMERIC], check_exact=True)
  near = _pooled_near(monkeypatch)
  _without_device_entries(monkeypatch)
  host = ci.fit_causalimpact_batch(frames, *periods, placebo=POOL, aggregates=AGGREGATES, **kw)
  assert len(near) == 1
  _assert_aggregates_agree(on, host, near[0], "batch")


def test_panel_event_aggregates_on_the_device_equal_the_host_route(monkeypatch):
  """(11), panel: lengths 70, 41 and 64 with their own periods in the ragged launch."""
  frames = base._frames(base.PANEL_LENGTHS)                                  # pylint: disable=protected-access
  every = [base._periods(f, b) for b, f in enumerate(frames)]              # pylint: disable=protected-access
  kw = dict(alpha=ALPHA, seed=FIT_SEED, outcome_link="log", inference_options=ci.InferenceOptions(**OPTS))
  on = ci.fit_causalimpact_panel(frames, every, placebo=POOL, event_aggregates=AGGREGATES, **kw)
  assert type(on) is ci.CausalImpactPanelAnalysis
  sim = ci.fit_causalimpact_panel(frames, every, placebo=base.SIM, **kw)
  off = ci.fit_causalimpact_panel(frames, every, event_aggregates=AGGREGATES, **kw)
  for b in range(3):
    pd.testing.assert_frame_equal(on[b].placebo, sim[b].placebo, check_exact=True)
  pd.testing.assert_frame_equal(on.summary, off.summary, check_exact=True)
  assert off.aggregate_placebo_quality is None
  for name in AGGREGATES:
    assert off.aggregates[name].placebo is None
    pd.testing.assert_frame_equal(on.aggregates[name].summary, off.aggregates[name].summary, check_exact=True)
    assert on.aggregates[name].placebo.index.name == "origin"
  near = _pooled_near(monkeypatch)
  _without_device_entries(monkeypatch)
  host = ci.fit_causalimpact_panel(frames, every, placebo=POOL, event_aggregates=AGGREGATES, **kw)
  assert len(near) == 1
  _assert_aggregates_agree(on, host, near[0], "panel")
