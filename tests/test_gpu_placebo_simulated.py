"""ci_session_simulate_placebo and ci_session_simulate_placebo_blocks on the device -- one simulated
path of every placebo window per posterior draw, linked step by step and summed -- against the numpy
twin `_placebo_simulated_host` on the parameter draws fetched from the same session, the device's
row statistics against plain numpy on the device's own totals, bit for bit across launches, sessions
and chunks, against the analytic placebo under the identity, and through the three fit functions.

T = 48, 2 chains x 37 kept draws: N = 74 fills no wavefront and no group count evenly.  Three series
with distinct Philox keys (series ids 0, 1, 2) and distinct prior records (tests/prior_cases.py).  The
steps 11 and 12 are missing and the post-period (from 0.7 T on) is masked.  H = 1 is the single-step
edge, 5 and 9 cross a Philox call's four normals.  Every comparison to the twin is at rtol 1e-8, atol
1e-8, the project's float64 contract (tests/test_gpu_placebo.py); outcomes are O(1) to O(100) on the
data scale under every link."""
import functools

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _model
from causalimpact import _native
from causalimpact import _synthetic as syn
from causalimpact import causalimpact_lib as lib

import prior_cases

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-8, atol=1e-8)
C_, S = 2, 37
N = C_ * S
SEED = (5, 9)
RANKS = [0, 1, 36, 37, 72, 73]
PARAM_FIELDS = ["observation_noise_scale", "level_scale", "slope_scale", "seasonal_drift_scales", "weights"]
STATS = ("predicted_mean", "spread_mean", "below", "total_order")
# link: (the `_native.LINK_*`, scale, shift) -- z = y * scale + shift is O(1) under the two links
LINKS = {"identity": (_native.LINK_IDENTITY, 3.7, -12.25), "log": (_native.LINK_LOG, 0.5, 2.0),
         "log1p": (_native.LINK_LOG1P, 0.5, 2.0)}
# name: (has_slope, seasons as (num_seasons, num_steps_per_season), P, T, the block-model entry)
MODELS = {
    "level": (False, (), 0, 48, False),
    "level+slope": (True, (), 2, 48, False),
    "level+slope+7": (True, ((7, 1),), 2, 48, False),
    "2 seasons": (False, ((2, 1),), 0, 48, False),
    "7+4x7 slope G=16": (True, ((7, 1), (4, 7)), 2, 48, True),
    "12 G=16": (False, ((12, 1),), 0, 48, True),
    "24 G=32": (False, ((24, 1),), 0, 48, True),
    "52 slope G=64": (True, ((52, 1),), 0, 60, True),
}


def _origins(Tb, H):
  """3 and 4 adjacent; 8 (its window reaches the gap 11, 12 for H = 5 and 9); the missing step 11 (a
  window without observation for H = 1, one with a gap else); 20; the last admissible one, whose
  window lies in the masked post-period; one unused slot."""
  return [3, 4, 8, 11, 20, Tb - H, -1]


def _series(T, P, seed, has_slope, seasons, distinct):
  y, mask, X, _ = syn.standardize_for_sampler(*syn.make_raw_series(T, max(P - 1, 0), seed), int(0.7 * T))
  if P == 0:
    X = None
  if seasons:
    y = y + 0.8 * np.sin(2 * np.pi * np.arange(T) / 7.0)
  mask = mask.copy()
  mask[[11, 12]] = True
  spec = _model.series_params(np.where(mask, np.nan, y), mask, X, has_slope=has_slope,
                              num_seasonal_blocks=len(seasons))
  return y, mask, X, prior_cases.filter_record(spec, P, has_slope, distinct)


def _pad(arrs, T, fill):
  out = np.full((len(arrs), T) + arrs[0].shape[1:], fill, arrs[0].dtype)
  for b, a in enumerate(arrs):
    out[b, :a.shape[0]] = a
  return out


def _open(name, lengths=None, ragged=False, only=None):
  """(session, inputs): three series of the model, or with `only` = b that series alone at
  series_offset b -- the same series id, hence the same Philox key."""
  has_slope, seasons, P, T, _ = MODELS[name]
  lengths = list(lengths or [T] * 3)
  series = [_series(Tb, P, 40 + 7 * b + P, has_slope, seasons, b) for b, Tb in enumerate(lengths)]
  which = list(range(len(lengths))) if only is None else [only]
  T = max(lengths[b] for b in which)
  num_seasons, sc = _model.expand_seasons(seasons, T)
  pb = _native.make_problem(T=T, P=P, has_slope=has_slope, num_warmup=3, num_results=S, num_chains=C_,
                            num_series=len(which), seed=SEED, series_offset=which[0], num_seasons=num_seasons)
  y = _pad([series[b][0] for b in which], T, np.nan)
  mask = _pad([series[b][1] for b in which], T, True)
  X = None if P == 0 else _pad([series[b][2] for b in which], T, 7.5)       # (padding rows are never read)
  specs = [series[b][3] for b in which]
  if ragged:
    sess = _native.Session.ragged(pb, [lengths[b] for b in which], y, mask, X, _native.make_params(specs))
  else:
    sess = _native.Session(pb, y, mask, X, sc, _native.make_params(specs))
  inputs = dict(y=np.where(mask, 0, y).astype(np.float32), mask=mask, sc=sc, num_seasons=num_seasons, specs=specs,
                X=None if X is None else X.astype(np.float32), lengths=[lengths[b] for b in which], ids=which)
  return sess, inputs


def _seen_from(totals):
  """A `seen` inside every window's simulated totals: the total of draw 7 itself, so that the count
  below has a tie to decide."""
  return np.ascontiguousarray(totals[:, :, 7])


@functools.lru_cache(maxsize=None)
def _run(name, H, lengths=None, ragged=False, only=None, links=tuple(LINKS)):
  """One session: its parameter draws and, per link, the simulated placebo with every output."""
  _, _, _, _, blocks = MODELS[name]
  sess, inp = _open(name, lengths, ragged, only)
  try:
    sess.run()
    draws = sess.fetch(PARAM_FIELDS)
    Hs = np.array(H if np.ndim(H) else [H] * len(inp["lengths"]), np.int32)
    origins = np.array([_origins(Tb, h) for Tb, h in zip(inp["lengths"], Hs)], np.int32)
    entry = sess.simulate_placebo_blocks if blocks else sess.simulate_placebo
    out = {}
    for link in links:
      code, scale, shift = LINKS[link]
      totals = entry(scale, shift, origins, Hs, code, None, RANKS, want=["totals"])["totals"]
      seen = _seen_from(totals)
      out[link] = dict(entry(scale, shift, origins, Hs, code, seen, RANKS, want=list(_native.PLACEBO_SIM_OUTPUTS)),
                       seen=seen)
      np.testing.assert_array_equal(out[link]["totals"], totals)          # (the same call twice: the same bits)
    return dict(draws=draws, out=out, inp=inp, origins=origins, horizon=Hs, kernel=sess.kernel_name())
  finally:
    sess.close()


def _pooled(draws, b):
  return {k: v[b].reshape((v.shape[1] * v.shape[2],) + v.shape[3:]) for k, v in draws.items()}


def _twin(run, name, b, link, seen=None):
  has_slope = MODELS[name][0]
  inp = run["inp"]
  Tb = inp["lengths"][b]
  code, scale, shift = LINKS[link]
  stream = lib.placebo_stream(SEED, inp["ids"][b], range(C_))
  return lib._placebo_simulated_host(                                       # pylint: disable=protected-access
      inp["y"][b, :Tb], inp["mask"][b, :Tb], None if inp["X"] is None else inp["X"][b, :Tb], inp["sc"][:, :Tb],
      inp["num_seasons"], has_slope, inp["specs"][b], _pooled(run["draws"], b), scale, shift, run["origins"][b],
      int(run["horizon"][b]), code, stream, seen=seen, ranks=RANKS)


def _check_totals(run, name, what):
  B = len(run["inp"]["lengths"])
  for link in run["out"]:
    got = run["out"][link]
    assert got["totals"].shape == (B, run["origins"].shape[1], N)
    for b in range(B):
      want = _twin(run, name, b, link, got["seen"][b])
      dev = float(np.abs(got["totals"][b] - want["totals"]).max())
      print(f"{what} [{run['kernel']}] {link} series {b}: largest deviation of a total {dev:.2e}, "
            f"largest total {np.abs(want['totals']).max():.3g}")
      np.testing.assert_allclose(got["totals"][b], want["totals"], err_msg=f"{what} {link} series {b}", **TOL)
      # a window without observation and the unused slot read 0 everywhere
      empty = want["cnt"] == 0
      assert empty[-1] and empty[-2] and (int(run["horizon"][b]) > 1 or empty[3])
      for k in STATS + ("totals",):
        rows = got[k][b][:, empty] if k == "total_order" else got[k][b][empty]
        assert (rows == 0.0).all(), (k, link, b)
      assert (np.abs(got["totals"][b][~empty]).min(axis=1) > 0).all()
      for k in ("predicted_mean", "spread_mean", "total_order"):
        np.testing.assert_allclose(got[k][b], want[k], err_msg=f"{what} {link} series {b} {k}", **TOL)


@pytest.mark.parametrize("H", [1, 5, 9])
@pytest.mark.parametrize("name", [n for n, m in MODELS.items() if not m[4]])
def test_one_lane_totals_equal_the_twin_on_the_fetched_draws(name, H):
  _check_totals(_run(name, H), name, f"{name} H={H}")


@pytest.mark.parametrize("H", [1, 5, 9])
@pytest.mark.parametrize("name", [n for n, m in MODELS.items() if m[4]])
def test_block_model_totals_equal_the_twin_on_the_fetched_draws(name, H):
  _check_totals(_run(name, H), name, f"{name} H={H}")


@pytest.mark.parametrize("name,H", [("level+slope+7", 9), ("level", 1), ("7+4x7 slope G=16", 5), ("24 G=32", 9)])
def test_the_statistics_equal_numpy_on_the_devices_own_totals_bit_for_bit(name, H):
  run = _run(name, H)
  counted = np.array([[0 if o < 0 else int((~run["inp"]["mask"][b, o:o + int(run["horizon"][b])]).sum())
                       for o in run["origins"][b]] for b in range(3)])
  for link, got in run["out"].items():
    totals, seen = got["totals"], got["seen"]
    some = counted > 0
    np.testing.assert_array_equal(got["predicted_mean"], _native.row_means_host(totals), err_msg=link)
    np.testing.assert_array_equal(got["total_order"], np.sort(totals, axis=2)[:, :, RANKS].transpose(0, 2, 1),
                                  err_msg=link)
    below = np.where(some, np.count_nonzero(totals <= seen[:, :, None], axis=2), 0)
    np.testing.assert_array_equal(got["below"], below.astype(np.float64), err_msg=link)
    assert (below[some] >= 1).all() and (below[some] < N).any()            # (draw 7 ties with `seen`)
    dev = totals - seen[:, :, None]
    np.testing.assert_array_equal(got["spread_mean"], np.where(some, _native.row_means_host(dev * dev), 0.0),
                                  err_msg=link)


@pytest.mark.parametrize("name", ["level+slope", "7+4x7 slope G=16"])
def test_a_batch_and_its_series_one_by_one_agree_bit_for_bit(name):
  whole = _run(name, 9)
  for b in range(3):
    one = _run(name, 9, only=b)
    for link in LINKS:
      np.testing.assert_array_equal(one["out"][link]["totals"][0], whole["out"][link]["totals"][b],
                                    err_msg=f"series {b} {link}")
      # (the statistics with the batch's `seen` are those of the same rows)
      for k in ("predicted_mean", "total_order"):
        np.testing.assert_array_equal(one["out"][link][k][0], whole["out"][link][k][b], err_msg=f"series {b} {link} {k}")


def test_a_ragged_sessions_series_agree_with_their_own_sessions_bit_for_bit_and_with_the_twin():
  """Lengths 48, 41 and 45 in one ragged launch, every series with its own horizon and origins; each
  one alone, on its own length as the stride, gives the same bits."""
  lengths, H = (48, 41, 45), (9, 1, 5)
  whole = _run("level+slope", H, lengths=lengths, ragged=True)
  assert "ragged" in whole["kernel"]
  _check_totals(whole, "level+slope", "ragged")
  for b in range(3):
    one = _run("level+slope", H[b], lengths=lengths, ragged=True, only=b)
    for link in LINKS:
      np.testing.assert_array_equal(one["out"][link]["totals"][0], whole["out"][link]["totals"][b],
                                    err_msg=f"series {b} {link}")


@pytest.mark.parametrize("name", ["level+slope+7", "12 G=16"])
def test_several_chunks_give_the_bits_of_one(name):
  blocks = MODELS[name][4]
  sess, inp = _open(name)
  try:
    sess.run()
    origins = np.array([_origins(Tb, 5) for Tb in inp["lengths"]], np.int32)
    O = origins.shape[1]
    code, scale, shift = LINKS["log"]
    want = list(_native.PLACEBO_SIM_OUTPUTS)
    seen = _seen_from(sess.simulate_placebo(scale, shift, origins, 5, code, None, RANKS, want=["totals"],
                                            blocks=blocks)["totals"])
    plain = sess.simulate_placebo(scale, shift, origins, 5, code, seen, RANKS, want=want, blocks=blocks)
    for max_rows, chunks in ((0, 1), (2 * O, 2), (2 * O + 3, 2), (O, 3)):
      got = sess.simulate_placebo(scale, shift, origins, 5, code, seen, RANKS, want=want, blocks=blocks,
                                  max_rows=max_rows)
      assert got.pop("num_chunks") == chunks
      for k in want:
        np.testing.assert_array_equal(got[k], plain[k], err_msg=f"{chunks} chunks {k}")
    with pytest.raises(_native.NativeError, match=f"max_rows must hold the {O} rows of one series, got {O - 1}"):
      sess.simulate_placebo(scale, shift, origins, 5, code, seen, RANKS, blocks=blocks, max_rows=O - 1)
  finally:
    sess.close()


@pytest.mark.parametrize("name,H", [("level+slope+7", 9), ("7+4x7 slope G=16", 5)])
def test_under_the_identity_the_mean_is_the_analytic_placebos_within_its_monte_carlo_error(name, H):
  """Given draw n the analytic total is N(C_n, V_n): the mean over the draws of one simulated total
  each has the analytic predicted_mean as its expectation and mean_n(V_n scale^2) / N as its variance."""
  has_slope, _, _, _, blocks = MODELS[name]
  code, scale, shift = LINKS["identity"]
  sess, inp = _open(name)
  try:
    sess.run()
    draws = sess.fetch(PARAM_FIELDS)
    origins = np.array([_origins(Tb, H) for Tb in inp["lengths"]], np.int32)
    sim = sess.simulate_placebo(scale, shift, origins, H, code, None, RANKS, blocks=blocks)["predicted_mean"]
    entry = sess.summarize_placebo_blocks if blocks else sess.summarize_placebo
    ana = entry(scale, shift, origins, H, want=["predicted_mean"])["predicted_mean"]
  finally:
    sess.close()
  for b in range(3):
    host = lib._placebo_summary_host(                                        # pylint: disable=protected-access
        inp["y"][b], inp["mask"][b], None if inp["X"] is None else inp["X"][b], inp["sc"], inp["num_seasons"],
        has_slope, inp["specs"][b], _pooled(draws, b), scale, shift, origins[b], H, per_draw=True)
    bound = 5.0 * np.sqrt((host["V"] * scale * scale).mean(axis=1) / N)
    print(f"{name} series {b}: |sim - analytic| / bound =", np.abs(sim[b] - ana[b]) / np.where(bound > 0, bound, 1.0))
    assert (np.abs(sim[b] - ana[b]) <= bound).all()
    assert (sim[b][host["cnt"] > 0] != ana[b][host["cnt"] > 0]).all()          # (a simulation, not the moments)


def test_errors_are_reported_before_any_device_work():
  sess, _ = _open("level")
  good = np.array([[3, 9], [3, -1], [3, 9]], np.int32)
  seen = np.zeros((3, 2))
  try:
    with pytest.raises(_native.NativeError, match="ci_session_simulate_placebo needs a finished ci_session_run"):
      sess.simulate_placebo(1.0, 0.0, good, 5, 0, seen, [0])
    sess.run()
    fn = _native.load().ci_session_simulate_placebo
    one, out, hz, rk = np.ones(3), np.zeros((3, 2)), np.full(3, 5, np.int32), np.zeros(1, np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data
    for args in ((None, one, good, hz, rk), (one, None, good, hz, rk), (one, one, None, hz, rk),
                 (one, one, good, None, rk), (one, one, good, hz, None)):
      sc, sh, org, h, r = args
      rc = fn(sess._h, ptr(sc), ptr(sh), 2, ptr(org), ptr(h), 0, seen.ctypes.data, 1, ptr(r),  # pylint: disable=protected-access
              out.ctypes.data, None, None, None, None)
      assert rc != 0 and "NULL argument" in _native.load().ci_last_error().decode()
    for want in (["spread_mean"], ["below"]):
      with pytest.raises(_native.NativeError, match="spread_mean and below need `seen`"):
        sess.simulate_placebo(1.0, 0.0, good, 5, 0, None, [0], want=want)
    assert list(sess.simulate_placebo(1.0, 0.0, good, 5, 0, None, [0])) == ["predicted_mean", "total_order"]
    for link in (-1, 3):
      with pytest.raises(_native.NativeError, match=f"link must be CI_LINK_IDENTITY, CI_LINK_LOG or CI_LINK_LOG1P .*got {link}"):
        sess.simulate_placebo(1.0, 0.0, good, 5, link, seen, [0])
    for ranks in ([], list(range(9))):
      with pytest.raises(_native.NativeError, match=rf"num_ranks must be in \[1, 8\], got {len(ranks)}"):
        sess.simulate_placebo(1.0, 0.0, good, 5, 0, seen, ranks)
    with pytest.raises(_native.NativeError, match=rf"rank {N} out of range \[0, {N}\)"):
      sess.simulate_placebo(1.0, 0.0, good, 5, 0, seen, [N])
    # the checks of the analytic entry, with its messages
    with pytest.raises(_native.NativeError, match=r"max_origins must be in \[1, 48\], got 49"):
      sess.simulate_placebo(1.0, 0.0, np.full((3, 49), -1), 5, 0, None, [0])
    with pytest.raises(_native.NativeError, match=r"horizon\[1\] must be at least 1, got 0"):
      sess.simulate_placebo(1.0, 0.0, good, [5, 0, 5], 0, seen, [0])
    with pytest.raises(_native.NativeError, match="strictly ascending with the unused slots"):
      sess.simulate_placebo(1.0, 0.0, [[3, 3], [3, -1], [3, 9]], 5, 0, seen, [0])
    with pytest.raises(_native.NativeError, match="must be a step or -1"):
      sess.simulate_placebo(1.0, 0.0, [[3, 9], [-2, -1], [3, 9]], 5, 0, seen, [0])
    with pytest.raises(_native.NativeError, match=r"origins\[0, 1\] = 44 with horizon 5 reaches beyond the series' 48 steps"):
      sess.simulate_placebo(1.0, 0.0, [[3, 44], [3, -1], [3, 9]], 5, 0, seen, [0])
    with pytest.raises(ValueError, match="unknown simulated placebo outputs"):
      sess.simulate_placebo(1.0, 0.0, good, 5, 0, seen, [0], want=["pit_mean"])
    with pytest.raises(ValueError, match=r"`seen` must be \[3, 2\]"):
      sess.simulate_placebo(1.0, 0.0, good, 5, 0, np.zeros((3, 3)), [0])
    # (the block entry takes this session too)
    assert sess.simulate_placebo_blocks(1.0, 0.0, good, 5, 0, seen, [0])["below"].shape == (3, 2)
  finally:
    sess.close()
  two, _ = _open("12 G=16")
  try:
    two.run()
    with pytest.raises(_native.NativeError, match=r"ci_session_simulate_placebo takes a trend with at most "
                                                  r"one block of 2 to 7 seasons.*\(12\)"):
      two.simulate_placebo(1.0, 0.0, good, 5, 0, seen, [0])
  finally:
    two.close()
  rag, _ = _open("level", lengths=(48, 41, 45), ragged=True)
  try:
    rag.run()
    with pytest.raises(_native.NativeError, match=r"origins\[1, 0\] = 37 with horizon 5 reaches beyond the series' 41 steps"):
      rag.simulate_placebo(1.0, 0.0, [[3], [37], [3]], 5, 0, None, [0])
    with pytest.raises(_native.NativeError, match="ci_session_simulate_placebo_blocks takes no ragged session"):
      rag.simulate_placebo_blocks(1.0, 0.0, [[3], [36], [3]], 5, 0, None, [0])
  finally:
    rag.close()


# ---- package level: Placebo(simulate=True) under a log link ----------------------------------------------

ALPHA, FIT_SEED = 0.1, (0, 11)
OPTS = dict(num_chains=2, num_results=37)
SIM = ci.Placebo(max_origins=6, simulate=True)
PANEL_LENGTHS = (70, 41, 64)
NUMERIC = [c for c in lib.PLACEBO_COLUMNS + lib.PLACEBO_SIMULATED_COLUMNS if c not in ("horizon_end", "significant", "pit", "p")]


def _frames(lengths=(70, 70, 70)):
  """Positive outcomes around 20 that move multiplicatively, one missing value inside the pre-period."""
  idx = pd.date_range("2022-03-01", periods=max(lengths), freq="D")
  frames = []
  for b, Tb in enumerate(lengths):
    y, X = syn.make_raw_series(max(lengths), 2, 70 + b, effect=4.0 + b)
    y = np.exp(3.0 + 0.25 * (y - y.mean()) / y.std())
    frame = pd.DataFrame(np.column_stack([y, X]), index=idx, columns=["y", "x0", "x1"]).iloc[:Tb].copy()
    frame.iloc[9 + b, 0] = np.nan
    frames.append(frame)
  return frames


def _periods(frame, b):
  last_pre = (6 * len(frame)) // 10 + b
  return ((frame.index[1 + b], frame.index[last_pre]), (frame.index[last_pre + 2], frame.index[len(frame) - 1 - b]))


def _host_fit(monkeypatch, frame, periods, seed):
  """The single fit on the route that pools the draws on the host (the numpy twin), and the number of
  simulated totals of the twin that lie within TOL of the observed total they are compared with."""
  near = []
  twin = lib._placebo_simulated_host                                        # pylint: disable=protected-access

  def spy(*args, **kw):
    out = twin(*args, **kw)
    counted = out["cnt"] > 0
    seen = np.asarray(kw["seen"], np.float64)[counted, None]
    near.append(int(np.count_nonzero(np.abs(out["totals"][counted] - seen) <= TOL["atol"] + TOL["rtol"] * np.abs(seen))))
    return out
  monkeypatch.setattr(lib, "_placebo_simulated_host", spy)
  one = ci.fit_causalimpact(frame, *periods, alpha=ALPHA, seed=seed, outcome_link="log", placebo=SIM,
                            inference_options=ci.InferenceOptions(summarize_on_device=False, **OPTS))
  monkeypatch.setattr(lib, "_placebo_simulated_host", twin)
  assert len(near) == 1
  return one, near[0]


def _assert_frames_agree(got, want, near, what):
  assert list(got.columns) == list(lib.PLACEBO_COLUMNS + lib.PLACEBO_SIMULATED_COLUMNS), what
  assert got.index.equals(want.index) and len(got) >= 3
  print(what, "largest deviation per column:", (got[NUMERIC] - want[NUMERIC]).abs().max().to_dict(),
        "draws within TOL of `seen`:", near)
  np.testing.assert_allclose(got[NUMERIC].to_numpy(np.float64), want[NUMERIC].to_numpy(np.float64), err_msg=what, **TOL)
  assert list(got["horizon_end"]) == list(want["horizon_end"])
  # pit = (below + 0.5) / (N + 1) may differ by one count per draw whose total lies within TOL of `seen`
  assert near == 0, "choose other data: a simulated total of the twin ties with the observed one"
  np.testing.assert_allclose(got["pit"], want["pit"], rtol=0, atol=near / (N + 1.0) + 1e-15)
  np.testing.assert_allclose(got["p"], want["p"], rtol=0, atol=2 * near / (N + 1.0) + 1e-15)
  assert list(got["significant"]) == list(want["significant"])
  assert ((got["pit"] > 0) & (got["pit"] < 1)).all() and (got["predicted_lower"] < got["predicted_upper"]).all()


def test_single_fit_on_the_device_equals_the_host_route_and_disturbs_nothing(monkeypatch):
  frame = _frames()[0]
  periods = _periods(frame, 0)
  kw = dict(alpha=ALPHA, seed=FIT_SEED, outcome_link="log", inference_options=ci.InferenceOptions(**OPTS))
  on = ci.fit_causalimpact(frame, *periods, placebo=SIM, **kw)
  off = ci.fit_causalimpact(frame, *periods, **kw)
  host, near = _host_fit(monkeypatch, frame, periods, FIT_SEED)
  _assert_frames_agree(on.placebo, host.placebo, near, "single fit")
  np.testing.assert_allclose(on.placebo_quality.to_numpy(), host.placebo_quality.to_numpy(), **TOL)
  assert off.placebo is None and off.placebo_quality is None
  pd.testing.assert_frame_equal(on.series, off.series, check_exact=True)
  pd.testing.assert_frame_equal(on.summary, off.summary, check_exact=True)
  for name in ("observation_noise_scale", "level_scale", "weights"):
    np.testing.assert_array_equal(np.asarray(getattr(on.posterior_samples, name)),
                                  np.asarray(getattr(off.posterior_samples, name)))


def test_batch_frames_equal_the_host_route_of_every_series_own_fit(monkeypatch):
  frames = _frames()
  periods = _periods(frames[0], 0)
  kw = dict(alpha=ALPHA, seed=FIT_SEED, outcome_link="log", inference_options=ci.InferenceOptions(**OPTS))
  got = ci.fit_causalimpact_batch(frames, *periods, placebo=SIM, **kw)
  assert type(got) is ci.CausalImpactBatchAnalysis             # (the one-launch route)
  assert got.placebo_quality.shape == (3, len(lib.PLACEBO_QUALITY_ENTRIES))
  for b in range(3):
    host, near = _host_fit(monkeypatch, frames[b], periods, _native.series_stream_key(FIT_SEED, b))
    _assert_frames_agree(got[b].placebo, host.placebo, near, f"batch series {b}")
    np.testing.assert_allclose(got.placebo_quality.iloc[b].to_numpy(), host.placebo_quality.to_numpy(), **TOL)
  off = ci.fit_causalimpact_batch(frames, *periods, **kw)
  assert off.placebo_quality is None and off[1].placebo is None
  pd.testing.assert_frame_equal(off.summary, got.summary, check_exact=True)
  pd.testing.assert_frame_equal(off[1].series, got[1].series, check_exact=True)


def test_panel_frames_equal_the_host_route_of_every_series_own_fit(monkeypatch):
  """Lengths 70, 41 and 64 with their own periods in the ragged launch."""
  frames = _frames(PANEL_LENGTHS)
  every = [_periods(f, b) for b, f in enumerate(frames)]
  kw = dict(alpha=ALPHA, seed=FIT_SEED, outcome_link="log", inference_options=ci.InferenceOptions(**OPTS))
  got = ci.fit_causalimpact_panel(frames, every, placebo=SIM, **kw)
  assert type(got) is ci.CausalImpactPanelAnalysis
  horizons = set()
  for b in range(3):
    host, near = _host_fit(monkeypatch, frames[b], every[b], _native.series_stream_key(FIT_SEED, b))
    _assert_frames_agree(got[b].placebo, host.placebo, near, f"panel series {b}")
    horizons.add(got.placebo_quality.iloc[b]["horizon"])
  assert len(horizons) > 1
  off = ci.fit_causalimpact_panel(frames, every, **kw)
  assert off.placebo_quality is None
  pd.testing.assert_frame_equal(off.summary, got.summary, check_exact=True)
