"""Every float32 reader of the prior record `ci_series_params` against the float64 oracle on a record in
which no two fields agree and every upper bound clips about half of the draws (tests/prior_cases.py;
tests/test_prior_cases.py shows on the oracle alone that reading any field for its sibling moves a
compared output by at least three tolerances).  One chain, W = 0 -- the *_scale0 and init_* fields
show in draw 1 -- and 12 draws (6 from T = 4096 on) on the oracle's Philox stream: identical
inclusion patterns, draws 1-4 at the tolerances of the per-draw tests of tests/test_gpu_gibbs.py,
later draws at 2e-2, and a device draw on the bound wherever the oracle's is.

Where the record is read and clipped, and the case that executes the site:

  csrc/ci_stage.hip   dev_series_params, dev_seasonal_params, prior_chol_reduced_d   every case
                      dev_seasonal_params(inert = true)                              wide-long, bigp-wide
  csrc/ci_gibbs.hip   wps[b] = params[b].weights_prior_scale; params[b] per series   every case; the batches
  csrc/ci_kernels.h   spike_slab_draw_regs (P <= 16; variance clip)                  trend-4w, batch-4w, ragged-trend, seq-weekly,
                                                                                     seq-d13, seq-workspace, wide-weekly,
                                                                                     wide-long, tp-ref, tp-d10, mw-d53
                      spike_slab_draw (17-52 columns in LDS; variance clip)          seq-p21, tp-p21
                      spike_slab_draw_big (53+ columns, one wavefront)               bigp-seq
                      spike_slab_draw_block (17-52 columns; variance clip)           block-wave, block-workgroup, wide-p21
                      gibbs_kernel: clipped_scale level / slope / obs (P = 0: scale) trend-p0, trend-4w(-p0)
                      init_level_loc, init_*_scale, *_scale0 at the kernel's head    every trend case
  csrc/ci_kernels8.h  regression wave's variance clip (design in LDS; from L2)       trend-8w, trend-8w-L8
                      clipped_scale level / slope, both kernels (D = 1, D = 2)       trend-8w (D = 2), trend-8w-L8 (D = 1)
  csrc/ci_bigp.h      variance clip of the workspace regression block                bigp-wide, bigp-tp, bigp-seq, bigp-weekly
  csrc/ci_wide.h      scale_from_gamma level / slope, drift clip, scale_draw obs     wide-weekly (P > 0), wide-weekly-p0
                      (P = 0: obs scale), one block; inert block                     (P = 0), wide-long, bigp-weekly,
                                                                                     batch-wide, ragged-wide
  csrc/ci_seasonal.h  scale_draw level / slope / obs, drift clip per block           seq-weekly, seq-d13, seq-d64 (P = 0),
                                                                                     seq-workspace (three blocks), bigp-seq
  csrc/ci_seasonal_tp.h  scale_draw level / slope / obs, drift clip per block        tp-ref (three blocks), tp-d10 (two,
                                                                                     slope), bigp-tp
  csrc/ci_seasonal_mw.h  the multi-wave build of ci_seasonal.h's iteration           mw-d53
  csrc/ci_ll.hip, ci_score_seq.h, ci_wide_score.h   init_level_loc, init_*_scale     test_loglik_and_score_...
  csrc/ci_predict.h, ci_placebo.h   the same four fields                             tests/test_gpu_predictions.py,
                                                                                     tests/test_gpu_placebo.py

P = 0 has a single trend build (four wavefronts; the eight-wave kernel exists for models with a
regression only), so `trend-p0` and `trend-4w-p0` name the same kernel with and without the flag.
HMC's log-prior of the scales and the float64 kernels (tests/test_gpu_float64_routes.py) are not
covered here."""
import functools

import numpy as np
import pytest

from causalimpact import _model, _native
from oracle import ci_oracle as orc

import prior_cases as pc

pytestmark = pytest.mark.gpu

SCALES = (("obs_scale", "obs_ub"), ("level_scale", "level_ub"), ("slope_scale", "slope_ub"),
          ("drift_scales", "drift_ub"))


def _pad(arrs, T, fill):
  out = np.full((len(arrs), T) + arrs[0].shape[1:], fill, arrs[0].dtype)
  for b, a in enumerate(arrs):
    out[b, :a.shape[0]] = a
  return out


def _fit(c, series, stride=None, lengths=None, series_offset=0, kernel=None):
  """One launch of the series [(y, mask, X, spec)] on case c's model and flags; `lengths`: a ragged session."""
  T = stride or series[0][0].shape[0]
  P = series[0][3]["P"]
  counts, _ = _model.expand_seasons(c.seasons, 1)
  flg = _model.expand_seasons(c.seasons, T)[1] if c.seasons else None
  pb = _native.make_problem(T=T, P=P, has_slope=c.has_slope, num_seasons=counts, num_warmup=0, num_results=c.S,
                            num_series=len(series), series_offset=series_offset, seed=pc.SEED, flags=c.flags)
  y = _pad([s[0] for s in series], T, np.nan)
  mask = _pad([s[1] for s in series], T, True)
  X = None if P == 0 else _pad([s[2] for s in series], T, 7.5)       # (padding rows are never read)
  params = _native.make_params([s[3] for s in series])
  if lengths is not None:
    sess = _native.Session.ragged(pb, lengths, y, mask, X, params, season_change=flg)
  else:
    sess = _native.Session(pb, y, mask, X, flg, params)
  try:
    if kernel is not None:
      assert kernel in sess.kernel_name(), sess.kernel_name()
    sess.run()
    return sess.fetch()
  finally:
    sess.close()


def _assert_follows_the_oracle(a, name, variant=0, T=None, what=""):
  """The fit `a` (oracle names) of a case member against its reference: every output within its tolerance,
  the same inclusion pattern, and on the bound where the oracle is."""
  c = pc.CASE_BY_NAME[name]
  spec, w = pc.case_inputs(name, variant, T)[3], pc.oracle_reference(name, variant, T)
  dev = pc.case_deviations(name, a, variant, T)
  print(f"{what or name}: deviation / tolerance " + ", ".join(f"{k} {v:.3f}" for k, v in dev.items()))
  if spec["P"]:
    np.testing.assert_array_equal(a["weights"] != 0, w["weights"] != 0, err_msg=f"{what or name}: inclusion")
  clipped = 0
  for key, ub in SCALES:
    if key not in dev:
      continue
    bound = spec[ub] if (key != "obs_scale" or spec["P"] == 0) else np.sqrt(spec[ub])
    on = np.isclose(w[key], bound, rtol=1e-12, atol=0.0)
    rtol = np.where(np.arange(c.S) >= pc.EARLY, 2e-2, 2e-2 if key == "drift_scales" else 5e-3)
    rtol = rtol.reshape((c.S,) + (1,) * (w[key].ndim - 1)) * np.ones(w[key].shape)
    assert on.sum() >= 2 and (~on).sum() >= 2, (name, key)
    assert (np.abs(a[key] - bound)[on] <= rtol[on] * bound).all(), (name, key, a[key], bound)
    clipped += int(on.sum())
  assert clipped >= 4
  assert max(dev.values()) <= 1.0, (what or name, dev)


@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_build_follows_the_oracle_on_a_record_of_distinct_fields_with_binding_bounds(name):
  c = pc.CASE_BY_NAME[name]
  got = _fit(c, [pc.case_inputs(name)], kernel=c.kernel)
  _assert_follows_the_oracle(pc.from_device(got), name)


# ---- three series with three records in one launch ----------------------------------------------
def _members(bc):
  return [pc.case_inputs(bc.case, b, T) for b, T in enumerate(bc.lengths)]


@functools.lru_cache(maxsize=None)
def _batch_fit(batch):
  bc = pc.BATCH_BY_NAME[batch]
  c = pc.CASE_BY_NAME[bc.case]
  stride = max(bc.lengths)
  if bc.ragged and c.seasons:
    stride = (stride + 3) & ~3
  # a ragged trend session is the four-wave kernel whatever the flags; ragged sessions take no route flag
  c = c._replace(flags=0) if bc.ragged else c
  got = _fit(c, _members(bc), stride=stride, lengths=list(bc.lengths) if bc.ragged else None, kernel=bc.kernel)
  for v in got.values():
    v.setflags(write=False)
  return got


@pytest.mark.parametrize("batch", [b.name for b in pc.BATCH_CASES])
def test_series_of_one_launch_follow_the_oracle_each_on_its_own_record_and_stream(batch):
  bc = pc.BATCH_BY_NAME[batch]
  got = _batch_fit(batch)
  for b, T in enumerate(bc.lengths):
    a = {k: (v[..., :T] if k in ("level", "slope", "trajectories", "pred_mean") else
             v[:, :T] if k == "seasonal" else v) for k, v in pc.from_device(got, b).items()}
    _assert_follows_the_oracle(a, bc.case, b, T, what=f"{batch} series {b}")
  for k in ("observation_noise_scale", "level_scale", "level"):
    assert not np.array_equal(got[k][0], got[k][1]) and not np.array_equal(got[k][1], got[k][2])


@pytest.mark.parametrize("batch", [b.name for b in pc.BATCH_CASES])
def test_series_of_one_launch_equal_their_single_launches_bit_for_bit(batch):
  """Series b of the launch and series b alone at series_offset b (a stock session of its own length):
  the same bits, so no series reads another's record."""
  bc = pc.BATCH_BY_NAME[batch]
  c = pc.CASE_BY_NAME[bc.case]
  got = _batch_fit(batch)
  for b, (one, T) in enumerate(zip(_members(bc), bc.lengths)):
    alone = _fit(c, [one], series_offset=b)
    assert sorted(alone) == sorted(got)
    for k, v in alone.items():
      g = got[k][b]
      if k in ("level", "slope", "posterior_trajectories", "posterior_means"):
        assert not g[..., T:].any(), (k, b)
        g = g[..., :T]
      elif k == "seasonal_levels":
        assert not g[:, :, T:].any(), (k, b)
        g = g[:, :, :T]
      np.testing.assert_array_equal(g, v[0], err_msg=f"{batch} {k} series {b}")


# ---- the other readers of the record: log-likelihood and score --------------------------------------
@pytest.mark.parametrize("T,p,has_slope,seasons,route,kernel", [
    (200, 3, 1, (), "auto", "hmc_kernel<2,1>"),               # ci_ll.hip: the time-parallel trend evaluator
    (5000, 2, 1, (), "auto", "hmc_wide_kernel"),              # ci_wide_score.h with the inert block
    (5000, 2, 1, (), "sequential", "hmc_seq_kernel"),         # ci_score_seq.h
    (120, 2, 0, pc.WEEK, "auto", "hmc_wide_kernel"),
    (120, 2, 0, pc.WEEK, "sequential", "hmc_seq_kernel"),
])
def test_loglik_and_score_read_the_initial_state_of_the_record(T, p, has_slope, seasons, route, kernel):
  """LogLikSession.evaluate against the oracle's analytic log-likelihood and score at the tolerances of
  tests/test_gpu_components.py::test_sequential_loglik_and_score_match_the_oracle, with init_level_loc
  and the three init_*_scale of the distinct record -- and far from the oracle's value under the
  default record, so that a reader of the wrong field cannot pass."""
  y, mask, X, base = pc.make_series(T, p, has_slope, seasons, data_seed=21)
  spec = pc.distinct_spec(base)
  counts, flg = _model.expand_seasons(seasons, T)
  P, K = spec["P"], len(seasons)
  rng = np.random.default_rng(1)
  E = 4
  theta = np.zeros((E, 3 + K + P))
  theta[:, 0] = rng.uniform(0.3, 0.9, E)
  theta[:, 1] = rng.uniform(0.02, 0.2, E)
  theta[:, 2] = rng.uniform(0.005, 0.03, E) if has_slope else 0.0
  theta[:, 3:3 + K] = rng.uniform(0.01, 0.1, (E, K))
  theta[:, 3 + K:] = 0.3 * rng.normal(size=(E, P))
  pb = _native.make_problem(T=T, P=P, has_slope=has_slope, num_seasons=counts, num_warmup=0, num_results=1,
                            flags=_native.FLAG_SEQUENTIAL_SEASONAL if route == "sequential" else 0)
  sess = _native.LogLikSession(pb, _native.make_params([spec]), y, mask, X, max_evals=8,
                               season_change=flg if K else None)
  try:
    assert kernel in sess.kernel_name(), sess.kernel_name()
    ll, grad = sess.evaluate(theta)
  finally:
    sess.close()

  def oracle(record, th):
    ssm = orc.make_ssm(record, mask, obs_scale=th[0], level_scale=th[1], slope_scale=th[2],
                       drift_scale=th[3:3 + K])
    resid = np.where(mask, 0.0, y) - X @ th[3 + K:]
    want_ll, ee, gs = orc.loglik_score(ssm, resid)
    want = np.concatenate([gs[:3], gs[3:3 + K], X.T @ ee])
    if not has_slope:
      want[2] = 0.0
    return want_ll, want

  for e in range(E):
    want_ll, want = oracle(spec, theta[e])
    np.testing.assert_allclose(ll[e], want_ll, rtol=3e-5, atol=3e-3)
    scale = np.maximum(np.abs(want), 1e-2 * np.abs(want).max())
    assert (np.abs(grad[e] - want) <= 2e-2 * scale + 1e-2).all(), (grad[e], want)
    # each of the fields this evaluator reads, replaced by its sibling or the default: three tolerances away
    swaps = dict(init_level_loc=base["init_level_loc"], init_level_scale=spec["init_slope_scale"])
    if has_slope:
      swaps["init_slope_scale"] = spec["init_level_scale"]
    if K:
      swaps["init_seasonal_scale"] = spec["init_level_scale"]
    for f, v in swaps.items():
      other_ll, _ = oracle(dict(spec, **{f: v}), theta[e])
      assert abs(other_ll - want_ll) >= 3 * (3e-5 * abs(want_ll) + 3e-3), (f, other_ll, want_ll)
