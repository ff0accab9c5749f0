"""`placebo=` without a GPU: the origin and horizon rules on hand-worked cases, `_placebo_summary_host`
against the joint Gaussian of the window built from dense products, its agreement with the one-step
filter at horizon 1, the frames, and the refusals before any fit."""
import math

import numpy as np
import pandas as pd
import pytest

import causalimpact as ci
from causalimpact import _model
from causalimpact import _native
from causalimpact import batch
from causalimpact import causalimpact_lib as lib
from oracle import ci_oracle as orc


# ---- the rules -----------------------------------------------------------------------------------

def test_horizon_history_and_origins_by_hand():
  P = lib.Placebo
  # horizon: the option, else min(n_post, n_pre // 3)
  assert lib.placebo_horizon(P(), 90, 20) == 20 and lib.placebo_horizon(P(), 45, 20) == 15
  assert lib.placebo_horizon(P(horizon=7), 45, 20) == 7
  # history: the option, else max(H, state_dim + 1)
  assert lib.placebo_min_history(P(), 20, 8) == 20 and lib.placebo_min_history(P(), 3, 8) == 9
  assert lib.placebo_min_history(P(min_history=2), 20, 8) == 2
  # n_pre 100, H 20: lo 20, hi 80, 61 admissible origins, 32 of them evenly: 20 + (60 i) // 31
  H, o = lib.placebo_plan(P(), 100, 20, 2)
  assert H == 20 and len(o) == 32 and o[0] == 20 and o[-1] == 80 and o[1] == 21 and o[2] == 23
  assert (np.diff(o) > 0).all() and o.dtype == np.int32
  # fewer admissible origins than max_origins: every one of them
  np.testing.assert_array_equal(lib.placebo_plan(P(), 45, 20, 2)[1], np.arange(15, 31))
  # max_origins 4 over lo 10 .. hi 40: 10 + (30 i) // 3
  np.testing.assert_array_equal(lib.placebo_origins(50, 10, 10, 4), [10, 20, 30, 40])
  # m = 1 is the last admissible origin: by max_origins, and because lo == hi
  np.testing.assert_array_equal(lib.placebo_origins(50, 10, 10, 1), [40])
  np.testing.assert_array_equal(lib.placebo_origins(20, 10, 10, 32), [10])
  # hi < lo: none
  assert lib.placebo_origins(19, 10, 10, 32).size == 0
  assert lib.placebo_plan(P(), 5, 20, 8)[1].size == 0           # H = 1, lo = 9, hi = 4
  assert lib.placebo_plan(P(), 2, 20, 1)[1].size == 0           # H = 0: no window at all


def test_the_argument_and_the_options():
  assert lib.resolve_placebo(None) is None and lib.resolve_placebo(True) == lib.Placebo()
  assert lib.resolve_placebo(lib.Placebo(horizon=3)).horizon == 3 and ci.Placebo is lib.Placebo
  assert lib.Placebo() == lib.Placebo(horizon=None, max_origins=32, min_history=None)
  with pytest.raises(TypeError, match="None, True or a Placebo"):
    lib.resolve_placebo(5)
  with pytest.raises(ValueError, match="horizon must be at least 1"):
    lib.Placebo(horizon=0)
  with pytest.raises(ValueError, match="max_origins must be at least 1"):
    lib.Placebo(max_origins=0)


def test_plans_of_a_panel_pad_with_minus_one_and_keep_a_row_for_a_series_without_room():
  origins, horizon = batch.placebo_plans(lib.Placebo(max_origins=3), [60, 5, 31], [10, 10, 12], 2)
  np.testing.assert_array_equal(horizon, [10, 1, 10])
  np.testing.assert_array_equal(origins, [[10, 30, 50], [3, 4, -1], [10, 15, 21]])
  origins, horizon = batch.placebo_plans(lib.Placebo(), [60, 2], [10, 10], 2)
  assert (origins[1] == -1).all() and horizon[1] == 0 and (origins[0] >= 0).sum() == 32
  origins, _ = batch.placebo_plans(lib.Placebo(), [2, 2], [10, 10], 2)
  assert origins.shape == (2, 1) and (origins == -1).all()


# ---- the numpy route against the joint Gaussian -------------------------------------------------

def _case(T, P, has_slope, seasons, seed=0, num_draws=6):
  """A series whose steps 11, 12, 40 are missing, and random parameter rows rounded to float32."""
  rng = np.random.default_rng(seed)
  y = np.cumsum(rng.normal(scale=0.1, size=T)) + rng.normal(scale=0.3, size=T)
  X = np.concatenate([rng.normal(size=(T, P - 1)), np.ones((T, 1))], axis=1) if P else None
  mask = np.zeros(T, bool)
  mask[[11, 12, 40]] = True
  spec = orc.default_spec(y, mask, X, has_slope=has_slope, seasons=seasons)
  K = len(seasons)
  f32 = lambda a: a.astype(np.float32)
  draws = dict(observation_noise_scale=f32(rng.uniform(0.1, 0.6, num_draws)),
               level_scale=f32(rng.uniform(0.01, 0.2, num_draws)),
               slope_scale=f32(rng.uniform(0.001, 0.02, num_draws)),
               seasonal_drift_scales=f32(rng.uniform(0.01, 0.1, (num_draws, K))),
               weights=f32(rng.normal(scale=0.3, size=(num_draws, P)) * (rng.random((num_draws, P)) < 0.6)))
  return np.where(mask, 0.0, y), mask, X, spec, draws


def _dense_model(spec, draws, n, has_slope, num_seasons, season_change, T):
  """(Z, [T_t], [Q_t], a_0, P_0, H) of draw n as explicit dense matrices."""
  hs = int(has_slope)
  d = 1 + hs + sum(k - 1 for k in num_seasons)
  Z = np.zeros(d)
  Z[0] = 1.0
  a0 = np.zeros(d)
  a0[0] = spec["init_level_loc"]
  P0 = np.zeros((d, d))
  P0[0, 0] = spec["init_level_scale"] ** 2
  if hs:
    P0[1, 1] = spec["init_slope_scale"] ** 2
  off = 1 + hs
  blocks = []
  for k, ns in enumerate(num_seasons):
    Z[off] = 1.0
    P0[off:off + ns - 1, off:off + ns - 1] = spec["init_seasonal_scale"] ** 2 * (np.eye(ns - 1) - 1.0 / ns)
    blocks.append((off, ns))
    off += ns - 1
  Ts, Qs = [], []
  for t in range(T):
    Tm, Q = np.eye(d), np.zeros((d, d))
    if hs:
      Tm[0, 1] = 1.0
      Q[1, 1] = float(draws["slope_scale"][n]) ** 2
    Q[0, 0] = float(draws["level_scale"][n]) ** 2
    for k, (o, ns) in enumerate(blocks):
      if season_change[k, t]:
        C = np.zeros((ns - 1, ns - 1))
        C[:-1, 1:] = np.eye(ns - 2)
        C[-1, :] = -1.0
        Tm[o:o + ns - 1, o:o + ns - 1] = C
        Q[o:o + ns - 1, o:o + ns - 1] = (float(draws["seasonal_drift_scales"][n, k]) / ns) ** 2
    Ts.append(Tm)
    Qs.append(Q)
  return Z, Ts, Qs, a0, P0, float(draws["observation_noise_scale"][n]) ** 2


def _brute_force(y, mask, reg, model, origin, horizon):
  """(C, V) of one draw: a dense filter to the origin, then the joint Gaussian of the window's
  observations from explicit products of T_t and Q_t, summed over the counted steps."""
  Z, Ts, Qs, a, P, H = model
  for t in range(origin):
    if not mask[t]:
      F = Z @ P @ Z + H
      K = P @ Z / F
      a = a + K * (y[t] - Z @ a - reg[t])
      P = P - np.outer(K, Z @ P)
    a, P = Ts[t] @ a, Ts[t] @ P @ Ts[t].T + Qs[t]
  means, covs = [a], [P]                 # the marginal moments of x_{o + h}
  for h in range(1, horizon):
    Tm = Ts[origin + h - 1]
    means.append(Tm @ means[-1])
    covs.append(Tm @ covs[-1] @ Tm.T + Qs[origin + h - 1])
  S = np.zeros((horizon, horizon))
  for h in range(horizon):
    Phi = np.eye(len(Z))               # x_k = Phi x_h + noise after h
    for k in range(h, horizon):
      if k > h:
        Phi = Ts[origin + k - 1] @ Phi
      S[h, k] = S[k, h] = Z @ Phi @ covs[h] @ Z
    S[h, h] += H
  counted = ~mask[origin:origin + horizon]
  mean_y = np.array([Z @ means[h] + reg[origin + h] for h in range(horizon)])
  return mean_y[counted].sum(), S[np.ix_(counted, counted)].sum()


@pytest.mark.parametrize("T,P,has_slope,seasons", [
    (60, 3, False, ()), (60, 0, True, ()), (60, 2, True, ((4, 2),)), (60, 0, False, ((7, 1),)),
    (60, 2, True, ((3, 1), (4, 2))),
])
def test_host_summary_is_the_joint_gaussian_of_the_window(T, P, has_slope, seasons):
  """C and V per draw against the brute-force joint covariance, windows with missing steps inside
  (11, 12 and 40), rtol and atol 1e-10."""
  y, mask, X, spec, draws = _case(T, P, has_slope, seasons)
  num_seasons, season_change = _model.expand_seasons(seasons, T)
  origins, horizon = [5, 9, 10, 33, 47, -1], 13
  scale, shift = 2.5, -3.0
  got = lib._placebo_summary_host(y, mask, X, season_change, num_seasons, has_slope, spec, draws, scale,
                                  shift, origins, horizon, per_draw=True)
  N = draws["level_scale"].shape[0]
  want_C, want_V = np.zeros((5, N)), np.zeros((5, N))
  for n in range(N):
    reg = X @ draws["weights"][n].astype(np.float64) if P else np.zeros(T)
    model = _dense_model(spec, draws, n, has_slope, num_seasons, np.asarray(season_change).reshape(len(num_seasons), T), T)
    for i, o in enumerate(origins[:5]):
      want_C[i, n], want_V[i, n] = _brute_force(y, mask, reg, model, o, horizon)
  np.testing.assert_allclose(got["C"][:5], want_C, rtol=1e-10, atol=1e-10)
  np.testing.assert_allclose(got["V"][:5], want_V, rtol=1e-10, atol=1e-10)
  cnt = np.array([(~mask[o:o + horizon]).sum() for o in origins[:5]])
  np.testing.assert_array_equal(got["cnt"][:5], cnt)
  assert (cnt < horizon).any()                       # some windows do contain gaps
  A = np.array([y[o:o + horizon][~mask[o:o + horizon]].sum() for o in origins[:5]])
  np.testing.assert_allclose(got["A"][:5], A, rtol=1e-14)
  # the three outputs from C, V, A; the unused slot reads 0
  e = A[:, None] - want_C
  np.testing.assert_allclose(got["predicted_mean"][:5], (want_C * scale + cnt[:, None] * shift).mean(axis=1),
                             rtol=1e-10)
  np.testing.assert_allclose(got["spread_mean"][:5], ((want_V + e * e) * scale * scale).mean(axis=1), rtol=1e-9)
  pit = 0.5 * np.vectorize(math.erfc)(-e / np.sqrt(2.0 * want_V))
  np.testing.assert_allclose(got["pit_mean"][:5], pit.mean(axis=1), rtol=1e-9, atol=1e-12)
  for k in ("predicted_mean", "spread_mean", "pit_mean"):
    assert got[k].shape == (6,) and got[k][5] == 0.0


def test_a_window_without_observation_reads_zero_and_bad_origins_are_refused():
  y, mask, X, spec, draws = _case(60, 2, True, ())
  args = (y, mask, X, np.zeros((0, 60)), [], True, spec, draws, 1.0, 0.0)
  got = lib._placebo_summary_host(*args, [11, 20], 2)            # steps 11, 12 are missing
  assert all(got[k][0] == 0.0 and got[k][1] != 0.0 for k in got)
  for bad, H in (([5, 5], 2), ([7, 5], 2), ([-1, 5], 2), ([5, 59], 2), ([5], 0)):
    with pytest.raises(ValueError):
      lib._placebo_summary_host(*args, bad, H)


@pytest.mark.parametrize("has_slope,seasons", [(False, ()), (True, ((7, 1),))])
def test_horizon_one_is_the_one_step_forecast(has_slope, seasons):
  """H = 1, one draw at a time: SUM is the filter's forecast bit for bit, SPREAD - e^2 its variance
  (1e-10) and PIT its pit, at origins that are observed; two adjacent origins among them."""
  T, P = 70, 3
  y, mask, X, spec, draws = _case(T, P, has_slope, seasons)
  num_seasons, season_change = _model.expand_seasons(seasons, T)
  origins, scale, shift = [9, 10, 13, 39, 41, 69], 2.5, -3.0
  for n in range(3):
    one = {k: v[n:n + 1] for k, v in draws.items()}
    ref = lib._prediction_summary_host(y, mask, X, season_change, num_seasons, has_slope, spec, one,
                                       scale, shift, [0])
    got = lib._placebo_summary_host(y, mask, X, season_change, num_seasons, has_slope, spec, one, scale,
                                    shift, origins, 1)
    np.testing.assert_array_equal(got["predicted_mean"], ref["forecast_mean"][origins])
    e = (y[origins] * scale + shift) - got["predicted_mean"]
    np.testing.assert_allclose(got["spread_mean"] - e * e, ref["variance_mean"][origins], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(got["pit_mean"], ref["pit_mean"][origins], rtol=1e-12)


# ---- frames --------------------------------------------------------------------------------------

def _hand_placebo():
  """Four origins over ten model steps, horizon 2; origin 4's window (steps 4, 5) holds no observation."""
  observed = np.array([1.0, 2.0, 3.0, 4.0, np.nan, np.nan, 7.0, np.nan, 9.0, 10.0])
  psum = dict(predicted_mean=np.array([4.0, 0.0, 8.0, 20.0]), spread_mean=np.array([5.0, 0.0, 1.0, 10.0]),
              pit_mean=np.array([0.6, 0.0, 0.2, 0.01]), n_counted=np.array([2.0, 0.0, 1.0, 2.0]),
              seen_sum=np.array([5.0, np.nan, 7.0, 19.0]))
  return psum, np.array([1, 4, 6, 8, -1]), observed


def test_frames_columns_index_and_quality_by_hand():
  psum, origins, observed = _hand_placebo()
  psum = {k: np.append(v, 0.0) for k, v in psum.items()}          # (the unused slot)
  idx = pd.date_range("2024-01-01", periods=10)
  frame, q = lib._placebo_frames(psum, origins, 2, 0.5, observed, idx, 2, -0.3)
  assert list(frame.columns) == list(lib.PLACEBO_COLUMNS) and frame.index.name == "origin"
  assert frame.index.equals(idx[[1, 4, 6, 8]].rename("origin"))
  assert list(frame["horizon_end"]) == list(idx[[2, 5, 7, 9]])
  np.testing.assert_array_equal(frame["n_counted"], [2, 0, 1, 2])
  np.testing.assert_array_equal(frame["actual"], [5.0, np.nan, 7.0, 19.0])
  np.testing.assert_array_equal(frame["predicted"], [4.0, np.nan, 8.0, 20.0])
  np.testing.assert_array_equal(frame["effect"], [1.0, np.nan, -1.0, -1.0])
  np.testing.assert_array_equal(frame["relative_effect"], [0.25, np.nan, -0.125, -0.05])
  np.testing.assert_array_equal(frame["predicted_sd"], [2.0, np.nan, 0.0, 3.0])    # sqrt(max(spread - e^2, 0))
  np.testing.assert_array_equal(frame["pit"], [0.6, np.nan, 0.2, 0.01])
  np.testing.assert_allclose(frame["p"], [0.8, np.nan, 0.4, 0.02])
  assert list(frame["significant"]) == [False, False, True, True]    # alpha 0.5: pit outside [0.25, 0.75]
  assert list(q.index) == list(lib.PLACEBO_QUALITY_ENTRIES)
  assert q["n_origins"] == 3 and q["horizon"] == 2 and q["false_positive_rate"] == 2 / 3
  assert q["mean_relative_effect"] == np.mean([0.25, -0.125, -0.05])
  assert q["mde_relative"] == np.quantile([0.25, 0.125, 0.05], 0.5)
  # |placebo| >= 0.3: none of three -> (1 + 0) / (1 + 3); the horizon is the post-period's (2)
  assert q["empirical_p"] == 0.25
  assert lib._placebo_frames(psum, origins, 2, 0.5, observed, idx, 2, 0.1)[1]["empirical_p"] == 0.75
  # ... and NaN when the horizon is not the post-period's
  assert np.isnan(lib._placebo_frames(psum, origins, 2, 0.5, observed, idx, 3, -0.3)[1]["empirical_p"])


def test_a_series_without_origin_has_an_empty_frame_and_a_nan_row():
  frame, q = lib._placebo_frames(None, np.array([-1, -1]), 0, 0.05, np.zeros(4), pd.RangeIndex(4), 3, 0.1)
  assert len(frame) == 0 and list(frame.columns) == list(lib.PLACEBO_COLUMNS)
  assert q["n_origins"] == 0 and q["horizon"] == 0 and q.iloc[2:].isna().all()


def test_seen_sums_count_the_observed_steps_in_the_samplers_format():
  y32 = np.array([0.1, 0.2, 0.0, 0.4], np.float32)
  mask = np.array([False, False, True, False])
  cnt, seen = lib._placebo_seen(y32, mask, [0, 2, -1], 2, 2.0, 1.0)
  np.testing.assert_array_equal(cnt, [2, 1, 0])
  assert seen[0] == (np.float64(y32[0]) + np.float64(y32[1])) * 2.0 + 2.0
  assert seen[1] == np.float64(y32[3]) * 2.0 + 1.0 and np.isnan(seen[2])


def test_batch_container_hands_out_one_quality_row_per_series_with_the_panels_nan_row():
  psum, origins, observed = _hand_placebo()
  B, T = 2, 10
  res = batch.CausalImpactBatchAnalysis.__new__(batch.CausalImpactBatchAnalysis)
  res._names, res.alpha = ["a", "b"], 0.5
  res._prep = type("P", (), dict(observed=np.stack([observed, observed])))()
  res._series_view = lambda b: (None, None, None, T)
  res.summary = pd.DataFrame({"rel_effect": [0.0, -0.3, 0.0, 0.2]})
  res._placebo_quality = None
  res._placebo = dict(summary={k: np.stack([v, np.zeros(4)]) for k, v in psum.items()},
                      origins=np.stack([origins[:4], np.full(4, -1)]), horizon=np.array([2, 0]),
                      n_post=np.array([2, 2]))
  q = res.placebo_quality
  assert list(q.index) == ["a", "b"] and list(q.columns) == list(lib.PLACEBO_QUALITY_ENTRIES)
  want = lib._placebo_frames(psum, origins[:4], 2, 0.5, observed, pd.RangeIndex(T), 2, -0.3)[1]
  pd.testing.assert_series_equal(q.iloc[0], want, check_names=False)
  assert q.loc["b", "n_origins"] == 0 and q.loc["b"].iloc[2:].isna().all()
  res._placebo = None
  assert res.placebo_quality is None


# ---- the fit functions -------------------------------------------------------------------------

def _fake_float64_fit(monkeypatch):
  """`fit_causalimpact(dtype=float64, summarize_on_device=False)` with the sampler replaced by random
  draws: the route that pools the draws on the host, without a device."""
  def fit(pb, y, mask, design, season_change, params):            # pylint: disable=unused-argument
    C, S, T = pb["num_chains"], pb["num_results"], y.shape[1]
    P, K = pb["P"], len(pb["num_seasons"])
    rng = np.random.default_rng(5)
    level = np.cumsum(rng.normal(scale=0.05, size=(1, C, S, T)), axis=-1)
    return dict(observation_noise_scale=rng.uniform(0.3, 0.6, (1, C, S)),
                level_scale=rng.uniform(0.02, 0.1, (1, C, S)), slope_scale=rng.uniform(0.001, 0.01, (1, C, S)),
                weights=rng.normal(scale=0.1, size=(1, C, S, P)), level=level,
                slope=np.zeros((1, C, S, T)), seasonal_drift_scales=rng.uniform(0.01, 0.1, (1, C, S, K)),
                seasonal_levels=np.zeros((1, C, S, T, K)), posterior_means=level.mean(axis=2),
                posterior_trajectories=level + rng.normal(scale=0.4, size=(1, C, S, T)))
  monkeypatch.setattr(_native, "make_problem", lambda **kw: kw)
  monkeypatch.setattr(_native, "make_params", lambda specs: specs)
  monkeypatch.setattr(_native, "fit_gibbs_f64", fit)


def _frame(T=120, seed=0):
  rng = np.random.default_rng(seed)
  x = rng.normal(size=T)
  y = 10.0 + 0.5 * x + np.cumsum(rng.normal(scale=0.05, size=T)) + rng.normal(scale=0.3, size=T)
  y[[11, 12, 40]] = np.nan
  return pd.DataFrame({"y": y, "x": x}, index=pd.date_range("2024-01-01", periods=T))


def test_fit_causalimpact_frames_on_the_numpy_route(monkeypatch):
  _fake_float64_fit(monkeypatch)
  df = _frame()
  idx = df.index
  kw = dict(data_options=ci.DataOptions(dtype=np.float64), seed=1,
            inference_options=ci.InferenceOptions(num_results=8, summarize_on_device=False))
  periods = ((idx[0], idx[89]), (idx[90], idx[119]))
  off = ci.fit_causalimpact(df, *periods, **kw)
  assert off.placebo is None and off.placebo_quality is None
  on = ci.fit_causalimpact(df, *periods, placebo=True, **kw)
  # placebo=None leaves every other frame as it is
  pd.testing.assert_frame_equal(on.series, off.series)
  pd.testing.assert_frame_equal(on.summary, off.summary)
  # n_pre 90, n_post 30: H = 30, lo 30, hi 60, 31 admissible origins: every one
  assert list(on.placebo.columns) == list(lib.PLACEBO_COLUMNS)
  assert on.placebo.index.equals(idx[30:61].rename("origin"))
  assert list(on.placebo["horizon_end"]) == list(idx[59:90])
  np.testing.assert_array_equal(on.placebo["n_counted"].iloc[:11], 29)       # the windows that hold step 40
  np.testing.assert_array_equal(on.placebo["n_counted"].iloc[11:], 30)
  y = df["y"].to_numpy()
  np.testing.assert_allclose(on.placebo["actual"], [np.nansum(y[o:o + 30]) for o in range(30, 61)], rtol=1e-13)
  np.testing.assert_allclose(on.placebo["effect"], on.placebo["actual"] - on.placebo["predicted"], atol=1e-9)
  assert ((on.placebo["pit"] > 0) & (on.placebo["pit"] < 1)).all() and (on.placebo["predicted_sd"] > 0).all()
  np.testing.assert_allclose(on.placebo["p"], 2 * np.minimum(on.placebo["pit"], 1 - on.placebo["pit"]))
  q = on.placebo_quality
  assert list(q.index) == list(lib.PLACEBO_QUALITY_ENTRIES) and q["n_origins"] == 31 and q["horizon"] == 30
  rel = np.abs(on.placebo["relative_effect"].to_numpy())
  fit_rel = abs(on.summary.loc["cumulative", "rel_effect"])
  assert q["empirical_p"] == (1 + np.count_nonzero(rel >= fit_rel)) / 32
  assert q["false_positive_rate"] == on.placebo["significant"].mean()
  # another horizon than the post-period's: no empirical p
  short = ci.fit_causalimpact(df, *periods, placebo=ci.Placebo(horizon=5, max_origins=4), **kw)
  assert np.isnan(short.placebo_quality["empirical_p"]) and short.placebo_quality["horizon"] == 5
  assert short.placebo.index.equals(idx[[5, 31, 58, 85]].rename("origin"))


def test_refusals_arrive_before_any_fit(monkeypatch):
  def no_fit(*a, **k):
    raise AssertionError("the sampler was reached")
  monkeypatch.setattr(lib, "_run_sampler", no_fit)
  monkeypatch.setattr(batch, "_assemble", no_fit)
  T = 120
  df = _frame(T).reset_index(drop=True)
  opts = ci.InferenceOptions(num_results=5)
  # a pre-period of 20 steps: H = 6, lo = 50, hi = 14
  with pytest.raises(ValueError, match="no room for an origin"):
    ci.fit_causalimpact(df, (0, 19), (20, 119), placebo=ci.Placebo(min_history=50), inference_options=opts)
  with pytest.raises(ValueError, match="no room for an origin"):
    batch.fit_causalimpact_batch([df, df], (0, 19), (20, 119), placebo=ci.Placebo(min_history=50),
                                 inference_options=opts)
  wide = ci.ModelOptions(seasons=[ci.Seasons(40), ci.Seasons(26)])          # 1 + 39 + 25 = 65
  for call in (lambda: ci.fit_causalimpact(df, (0, 79), (80, 119), model_options=wide, placebo=True),
               lambda: batch.fit_causalimpact_batch([df, df], (0, 79), (80, 119), model_options=wide, placebo=True),
               lambda: batch.fit_causalimpact_panel([df, df], [((0, 79), (80, 119))] * 2, model_options=wide,
                                                    placebo=True)):
    with pytest.raises(ValueError, match="at most 64 components, this model has 65"):
      call()
  with pytest.raises(TypeError, match="None, True or a Placebo"):
    ci.fit_causalimpact(df, (0, 79), (80, 119), placebo="yes")
  # ... and a panel lets a series without room through to its fit (the NaN row), as without the option
  for placebo in (None, ci.Placebo(min_history=50)):
    with pytest.raises(AssertionError, match="the sampler was reached"):
      batch.fit_causalimpact_panel([df, df], [((0, 19), (20, 119)), ((0, 79), (80, 119))], placebo=placebo,
                                   inference_options=opts)
