"""A session made from draws on the device (ci_session_create_from_draws[_f64], `_native.DrawsSession`):
the ten prediction-error and placebo entries on uploaded parameter draws.

 1. On the draws a Gibbs session fetched, with its problem record, every entry returns the bits of
    that session -- the simulated totals and the pooled accumulators included, also at
    chain_offset 3 and series_offset 5.
 2. The float64 entry on those float32 values widened to float64 returns the same bits.
 3. The float64 entry reads float64: on inputs float32 cannot hold (`draws_cases.f64_case`, whose
    power tests/test_draws_session.py asserts) every output agrees with its numpy twin at the
    tolerance, the counts `below` exactly.
 4. The entries in two different orders on one session return the same bits.
 5. Every entry that needs a fit refuses the session with its message, and the session still answers.

Shapes and tolerance: tests/draws_cases.py."""
import functools

import numpy as np
import pytest

from causalimpact import _comm
from causalimpact import _native
from causalimpact import causalimpact_lib as lib

import draws_cases as dc

pytestmark = pytest.mark.gpu

SCALE, SHIFT = 3.7, -12.25
LOG_SCALE, LOG_SHIFT = 0.05, 2.0          # z = y * scale + shift stays inside the log link's domain
SIM_SEEN = np.full(dc.ORIGINS.shape, 18.0)
POOL_SEEN = np.asarray([[1.0, -2.0, 0.5], [3.0, 0.0, -1.0]])
POOL_COUNTED = np.asarray([[18, 18, 9], [12, 12, 6]], np.int32)
CALLS = ("predictions", "placebo", "simulated", "pooled", "pooled_simulated")


def _call(sess, kind, blocks, scale=SCALE, shift=SHIFT, link=_native.LINK_LOG, sim_scale=LOG_SCALE,
          sim_shift=LOG_SHIFT, sim_seen=SIM_SEEN):
  """The outputs of one entry kind of `sess` (with `blocks` its _blocks entry), every output asked for."""
  tail = "_blocks" if blocks else ""
  if kind == "predictions":
    return getattr(sess, "summarize_predictions" + tail)(scale, shift, dc.RANKS)
  if kind == "placebo":
    return getattr(sess, "summarize_placebo" + tail)(scale, shift, dc.ORIGINS, dc.HORIZON)
  if kind == "simulated":
    return getattr(sess, "simulate_placebo" + tail)(sim_scale, sim_shift, dc.ORIGINS, dc.HORIZON, link, sim_seen,
                                                     dc.RANKS, want=list(dc.SIM) + ["totals"])
  if kind == "pooled":
    return getattr(sess, "pool_placebo" + tail)(scale, shift, dc.GROUPS, dc.ORIGINS, dc.GROUP_HORIZON, None, POOL_SEEN)
  return getattr(sess, "pool_simulated_placebo" + tail)(sim_scale, sim_shift, dc.GROUPS, dc.ORIGINS, dc.GROUP_HORIZON,
                                                        link, None, POOL_SEEN, POOL_COUNTED, dc.RANKS)


def _all(sess, blocks, order=CALLS, **kw):
  return {kind: _call(sess, kind, blocks, **kw) for kind in order}


def _same_bits(got, want, what):
  assert sorted(got) == sorted(want)
  for kind in want:
    assert sorted(got[kind]) == sorted(want[kind]), (what, kind)
    for k, v in want[kind].items():
      np.testing.assert_array_equal(got[kind][k], v, err_msg=f"{what}: {kind} {k}")


@functools.lru_cache(maxsize=None)
def _fit(name, chain_offset=0, series_offset=0):
  """One Gibbs session of model `name`: its parameter draws and the outputs of its five entry kinds."""
  inp, blocks = dc.inputs(name), dc.MODELS[name][2]
  sess = _native.Session(dc.problem(name, chain_offset, series_offset), inp["y"], inp["mask"], inp["X"], inp["sc"],
                         _native.make_params(inp["specs"]))
  try:
    sess.run()
    return dict(draws=sess.fetch(dc.DRAW_FIELDS), out=_all(sess, blocks), inp=inp, blocks=blocks)
  finally:
    sess.close()


def _drawn(name, fit, dtype, chain_offset=0, series_offset=0, draws=None, inp=None):
  inp = fit["inp"] if inp is None else inp
  return _native.DrawsSession(dc.problem(name, chain_offset, series_offset, num_warmup=0), inp["y"], inp["mask"],
                              inp["X"], inp["sc"], _native.make_params(inp["specs"]),
                              fit["draws"] if draws is None else draws, dtype=dtype)


@pytest.mark.parametrize("offsets", [(0, 0), (3, 5)])
@pytest.mark.parametrize("name", list(dc.MODELS))
def test_the_draws_session_returns_the_bits_of_the_fit_session(name, offsets):
  fit = _fit(name, *offsets)
  assert all(np.isfinite(v).all() for out in fit["out"].values() for v in out.values())
  assert (fit["out"]["simulated"]["totals"] != 0).any() and (fit["out"]["pooled_simulated"]["acc"] != 0).any()
  sess = _drawn(name, fit, np.float32, *offsets)
  try:
    _same_bits(_all(sess, fit["blocks"]), fit["out"], f"{name} at offsets {offsets}")
  finally:
    sess.close()
  if offsets != (0, 0):           # (the streams are part of the address: other offsets, other totals)
    assert (fit["out"]["simulated"]["totals"] != _fit(name)["out"]["simulated"]["totals"]).any()


@pytest.mark.parametrize("name", list(dc.MODELS))
def test_the_float64_build_is_the_float32_build_on_widened_values(name):
  fit = _fit(name)
  wide = {k: v.astype(np.float64) for k, v in fit["draws"].items()}
  inp = dict(fit["inp"], y=fit["inp"]["y"].astype(np.float32).astype(np.float64),
             X=fit["inp"]["X"].astype(np.float32).astype(np.float64))
  sess = _drawn(name, fit, np.float64, draws=wide, inp=inp)
  try:
    _same_bits(_all(sess, fit["blocks"]), fit["out"], name)
  finally:
    sess.close()


def _pool_terms(inp, draws, scale, shift, simulated_link=None):
  """Per entry of `GROUPS` (groups ascending, members ascending) the twin's terms [K, O, N]: (s, v) of
  the analytic pool, or the simulated totals on every member's own stream; and the counted steps."""
  sums, variances, counted = [], [], np.zeros((len(dc.GROUPS), dc.ORIGINS.shape[1]), np.int32)
  for g, (members, horizon) in enumerate(zip(dc.GROUPS, dc.GROUP_HORIZON)):
    for b in sorted(members):
      if simulated_link is None:
        got = dc.twin_placebo(inp, draws, b, scale, shift, horizon=horizon, per_draw=True)
        s, v = _native.placebo_terms_host(got["C"], got["V"], got["cnt"], scale, shift)
        sums.append(s)
        variances.append(v)
      else:
        stream = lib.placebo_stream(dc.SEED, b, range(dc.C))
        got = dc.twin_simulated(inp, draws, b, scale, shift, simulated_link, stream, horizon=horizon)
        sums.append(got["totals"])
      counted[g] += np.asarray(got["cnt"], np.int32)
  return np.stack(sums), (np.stack(variances) if variances else None), counted


@pytest.mark.parametrize("name", list(dc.MODELS))
def test_the_float64_build_reads_float64(name):
  inp, draws = dc.f64_case(name)
  blocks = dc.MODELS[name][2]
  scale, shift, link = dc.F64_SCALE, dc.F64_SHIFT, _native.LINK_IDENTITY
  sess = _native.DrawsSession(dc.problem(name, num_warmup=0), inp["y"], inp["mask"], inp["X"], inp["sc"],
                              _native.make_params(inp["specs"]), draws, dtype=np.float64)
  try:
    # the twins first: `seen` lies between two of the twin's simulated totals, so that `below` is a
    # count no last bit decides
    streams = [lib.placebo_stream(dc.SEED, b, range(dc.C)) for b in range(dc.B)]
    free = [dc.twin_simulated(inp, draws, b, scale, shift, link, streams[b])["totals"] for b in range(dc.B)]
    ordered = np.sort(np.stack(free), axis=2)
    seen = 0.5 * (ordered[:, :, 30] + ordered[:, :, 31])
    assert (ordered[:, :2, 31] - ordered[:, :2, 30] > 1e-6).all()
    got = _all(sess, blocks, scale=scale, shift=shift, link=link, sim_scale=scale, sim_shift=shift, sim_seen=seen)
    worst = {}

    def close(kind, k, have, want):
      worst[f"{kind}.{k}"] = max(worst.get(f"{kind}.{k}", 0.0), float(np.abs(have - want).max()))
      np.testing.assert_allclose(have, want, err_msg=f"{name}: {kind} {k}", **dc.TOL)

    for b in range(dc.B):
      pred = dc.twin_predictions(inp, draws, b, scale, shift)
      for k in dc.PRED:
        close("predictions", k, got["predictions"][k][b], pred[k])
      plac = dc.twin_placebo(inp, draws, b, scale, shift)
      for k in dc.PLAC:
        close("placebo", k, got["placebo"][k][b], plac[k])
      sim = dc.twin_simulated(inp, draws, b, scale, shift, link, streams[b], seen=seen[b])
      for k in ("predicted_mean", "spread_mean", "total_order", "totals"):
        close("simulated", k, got["simulated"][k][b], sim[k])
      np.testing.assert_array_equal(got["simulated"]["below"][b], sim["below"], err_msg=f"{name}: below of series {b}")
      used = dc.ORIGINS[b] >= 0
      assert (sim["below"][used] == 31).all() and (got["simulated"]["totals"][b][~used] == 0).all()
    # a float32 reading of the same inputs is out of tolerance (the power check, on the device's own output)
    narrow = dc.twin_predictions(inp, draws, 0, scale, shift, np.float32)["forecast_mean"]
    assert dc.beyond(narrow, got["predictions"]["forecast_mean"][0])
    # the pooled entries against the host pools of the twins' terms
    csr = _native.groups_csr(dc.GROUPS, dc.B)
    sums, variances, _ = _pool_terms(inp, draws, scale, shift)
    acc = _native.pool_placebo_host(sums, variances, csr, None)
    close("pooled", "acc", got["pooled"]["acc"], acc)
    for k, v in _native.finish_placebo_host(acc, POOL_SEEN).items():
      close("pooled", k, got["pooled"][k], v)
    totals, _, _ = _pool_terms(inp, draws, scale, shift, link)
    acc = _native.pool_simulated_placebo_host(totals, csr, None)
    close("pooled_simulated", "acc", got["pooled_simulated"]["acc"], acc)
    fin = _native.finish_simulated_placebo_host(acc, POOL_SEEN, POOL_COUNTED, dc.RANKS)
    for k in ("predicted_mean", "spread_mean", "total_order"):
      close("pooled_simulated", k, got["pooled_simulated"][k], fin[k])
    print(f"{name}: largest deviations " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
  finally:
    sess.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["slope+7 d=8", "slope+12 d=13"])
def test_calls_leave_nothing_behind(name, dtype):
  fit = _fit(name)
  sess = _drawn(name, fit, dtype)
  try:
    first = _all(sess, fit["blocks"])
    again = _all(sess, fit["blocks"], order=("pooled_simulated", "placebo", "pooled", "predictions", "simulated"))
    _same_bits(again, first, f"{name} in another order")
    if dtype == np.float32:          # (the float64 session reads the unrounded outcome and design)
      _same_bits(first, fit["out"], name)
  finally:
    sess.close()


def test_the_entries_that_need_a_fit_refuse_the_session(tmp_path):
  name = "slope+7 d=8"
  fit = _fit(name)
  sess = _drawn(name, fit, np.float32)
  comm = _comm.Comm(0, 1, device=0, transport="host", path=str(tmp_path / "rendezvous"))
  observed, flags = np.zeros((dc.B, dc.T)), np.zeros((dc.B, dc.T), np.uint8)
  first, count = np.zeros((dc.B, 1), np.int32), np.ones((dc.B, 1), np.int32)
  fit_only = {
      "ci_session_run": sess.run,
      "ci_session_run_streamed": lambda: sess.run_streamed(pinned=False),
      "ci_session_fetch": lambda: sess.fetch(["level_scale"]),
      "ci_session_summarize": lambda: sess.summarize(1.0, 0.0, observed, flags, dc.RANKS),
      "ci_session_summarize_components": lambda: sess.summarize_components(1.0, 0.0, dc.RANKS),
      "ci_session_summarize_windows": lambda: sess.summarize_windows(1.0, 0.0, observed, first, count, dc.RANKS),
      "ci_session_summarize_paths": lambda: sess.summarize_paths(1.0, 0.0, observed, first, count, dc.RANKS),
      "ci_session_pool_trajectories": lambda: sess.pool_trajectories(1.0, 0.0, [{0: 1.0}]),
      "ci_session_pool_event_trajectories": lambda: sess.pool_event_trajectories(1.0, 0.0, [({0: (1.0, 0)}, 5)]),
      "ci_session_value_mean": lambda: sess.value_mean(1.0, 0.0),
      "ci_session_profile": sess.profile,
      "ci_session_kernel_name": sess.kernel_name,
      "ci_session_algorithmic_bytes": sess.algorithmic_bytes,
      "ci_comm_session_all_gather": lambda: comm.session_all_gather(sess, "level_scale"),
  }
  try:
    for entry, call in fit_only.items():
      with pytest.raises(_native.NativeError, match=entry + r": the session was made from draws \(ci_session_create_from_draws\)"):
        call()
    _same_bits({"placebo": _call(sess, "placebo", False)}, {"placebo": fit["out"]["placebo"]}, "after the refusals")
  finally:
    comm.close()
    sess.close()
