"""Many independent series in one launch (BASELINE "batch of 512 independent series, T=500,
5 covariates").

`fit_causalimpact_batch` is the batched form of `fit_causalimpact` for B series that share an
index and the pre/post periods (the same calendar for many geos / products):
  * data preparation (data.py:105-137, standardize.py:42-55) is vectorised over series in numpy
    -- no per-series pandas;
  * one kernel launch per device runs all B x chains Gibbs fits (one workgroup per
    (series, chain)); series are sharded over `InferenceOptions.devices`, no collective;
  * the T x draws post-processing of every series runs on the device that holds the draws
    (csrc/ci_summary.h); only order statistics and per-draw totals come back;
  * the (B*2) x 15 summary table is assembled with numpy; a per-series `CausalImpactAnalysis`
    (14-column `series` frame) is built lazily on indexing.
Random streams are keyed by (series position in the batch, chain): Monte-Carlo errors are
independent across series; `shared_streams=True` keys them by chain only, which makes series b
of a batch equal `fit_causalimpact` on series b alone with the same seed, draw for draw.
"""
from __future__ import annotations

import concurrent.futures
import dataclasses
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import pandas as pd

from causalimpact import _model
from causalimpact import _native
from causalimpact import causalimpact_lib as lib
from causalimpact import data as cid
from causalimpact import indices
from causalimpact import standardize


@dataclasses.dataclass
class PreparedBatch:
  """What the sampler consumes for B series (the batched CausalImpactData)."""
  values: np.ndarray          # [B, T_all, 1+p] raw data
  index: pd.Index             # [T_all]
  pre_period: Tuple[Any, Any]
  post_period: Tuple[Any, Any]
  standardize_data: bool
  model_rows: np.ndarray      # positions (into index) of the T steps handed to the sampler
  num_pre: int
  y: np.ndarray               # [B, T] standardised outcome, NaN where missing / forecast
  mask: np.ndarray            # [B, T] bool
  design: Optional[np.ndarray]   # [B, T, P] standardised covariates + intercept, or None
  outcome_mean: np.ndarray    # [B] pre-period mean of the outcome (0 if not standardised)
  outcome_sd: np.ndarray      # [B] pre-period sd (ddof=1)     (1 if not standardised)


def prepare_batch(values: np.ndarray, index: pd.Index, pre_period, post_period,
                  standardize_data: bool = True) -> PreparedBatch:
  """Vectorised CausalImpactData.__init__ (data.py:77-137) for [B, T_all, 1+p] values whose
  first column is the outcome."""
  values = np.asarray(values, dtype=np.float64)
  if values.ndim != 3:
    raise ValueError("`values` must be [num_series, num_timesteps, 1 + num_covariates]")
  B, T_all, ncol = values.shape
  index = pd.Index(index)
  if len(index) != T_all:
    raise ValueError("`index` must have one entry per timestep")
  probe = pd.DataFrame({"y": np.zeros(T_all)}, index=index)
  pre, post = indices.parse_and_validate_date_data(data=probe, pre_period=pre_period,
                                                  post_period=post_period)
  outcome = values[:, :, 0]
  with np.errstate(invalid="ignore"):
    if np.any(np.nanstd(outcome, axis=1) == 0):
      raise ValueError("Input response cannot be constant.")
  if np.any(np.sum(~np.isnan(outcome), axis=1) < 3):
    raise ValueError("Input data must have at least 3 observations.")
  if ncol > 1 and np.isnan(values[:, :, 1:]).any():
    raise ValueError("Input data cannot have any missing values.")
  in_pre = np.asarray((index >= pre[0]) & (index <= pre[1]))
  after = np.asarray(index > pre[1])
  rows = np.concatenate([np.flatnonzero(in_pre), np.flatnonzero(after)])
  n_pre = int(in_pre.sum())
  model = values[:, rows, :]                               # [B, T, 1+p]
  if standardize_data:
    scaled, mu, sd = standardize.standardize_batch(model, n_pre)
    o_mu, o_sd = mu[:, 0].copy(), sd[:, 0].copy()
  else:
    scaled = model
    o_mu, o_sd = np.zeros(B), np.ones(B)
  y = scaled[:, :, 0].copy()
  y[:, n_pre:] = np.nan
  mask = np.isnan(y)
  design = None
  if ncol > 1:
    design = np.concatenate([scaled[:, :, 1:], np.ones((B, len(rows), 1))], axis=2)
  return PreparedBatch(values=values, index=index, pre_period=pre, post_period=post,
                       standardize_data=standardize_data, model_rows=rows, num_pre=n_pre, y=y,
                       mask=mask, design=design, outcome_mean=o_mu, outcome_sd=o_sd)


def summary_table(names, alpha, ranks, dsum, *, n_win, n_obs, obs_mean, obs_sum, avg_pred,
                  cum_pred) -> pd.DataFrame:
  """The (series, average|cumulative) x 15 summary table from the statistics of every series'
  own post-period window: n_win (steps in the window; an int when all series share it, else [B]),
  n_obs [B] (observed steps in it), obs_mean / obs_sum [B] (observed outcome over it), avg_pred /
  cum_pred [B] (posterior mean over it), and the device summary `dsum` ("per_draw" [B, 2, N]
  window totals of prediction and point effect per draw; optionally "per_draw_order" [B, 2, R],
  their order statistics `ranks`).  The same numpy reductions as `_summary_rows`, along axis 1."""
  B = len(names)
  quantiles = (alpha / 2.0, 1.0 - alpha / 2.0)
  n_obs = np.asarray(n_obs)
  n_win_d = n_win if np.ndim(n_win) == 0 else np.asarray(n_win)[:, None]    # against [B, N]
  pred_sum, point_sum = dsum["per_draw"][:, 0], dsum["per_draw"][:, 1]   # [B, N]
  with np.errstate(invalid="ignore", divide="ignore"):
    pred_mean = pred_sum / n_win_d
    point_mean = np.where(n_obs[:, None] > 0, point_sum / np.maximum(n_obs, 1)[:, None], np.nan)
    rel = obs_sum[:, None] / pred_sum - 1.0

    # The bands interpolate order statistics of the per-draw totals; the device returned
    # those (per_draw_order), and every banded quantity is a monotone map of the totals, so
    # its order statistics are the mapped ones -- no [B, draws] sort on the host.
    ranks = list(ranks)
    N = pred_sum.shape[1]
    order = dsum.get("per_draw_order")
    if order is None:
      order = np.sort(dsum["per_draw"], axis=2)[:, :, ranks]
    (lo_a, hi_a, g_a), (lo_b, hi_b, g_b) = lib._quantile_ranks(N, quantiles)   # pylint: disable=protected-access
    lerp = lib._lerp_order_stats                                               # pylint: disable=protected-access

    def band_of(by_rank):
      return np.stack([lerp(by_rank, lo_a, hi_a, g_a), lerp(by_rank, lo_b, hi_b, g_b)])

    pred_o = {r: order[:, 0, i] for i, r in enumerate(ranks)}
    point_o = {r: order[:, 1, i] for i, r in enumerate(ranks)}
    need = (lo_a, hi_a, lo_b, hi_b)
    band_pred_sum, band_point_sum = band_of(pred_o), band_of(point_o)
    band_pred_mean = band_of({k: pred_o[k] / n_win for k in need})
    band_point_mean = band_of({k: np.where(n_obs > 0, point_o[k] / np.maximum(n_obs, 1), np.nan)
                               for k in need})
    # rel = obs_sum / pred_sum - 1 is monotone in pred_sum on either side of zero: decreasing
    # when obs_sum > 0 (its k-th smallest comes from the (N-1-k)-th smallest total), else
    # increasing.  Series whose totals straddle zero take the sort.
    down = obs_sum > 0
    band_rel = band_of({k: np.where(down, obs_sum / pred_o[N - 1 - k], obs_sum / pred_o[k]) - 1.0
                        for k in need})
    straddle = ~((pred_sum.min(axis=1) > 0) | (pred_sum.max(axis=1) < 0))
    if straddle.any():
      band_rel[:, straddle] = np.quantile(rel[straddle], quantiles, axis=1)

    def sd(x):
      return np.std(x, axis=1, ddof=1)

    cols = {
        "actual": (obs_mean, obs_sum),
        "predicted": (avg_pred, cum_pred),
        "predicted_lower": (band_pred_mean[0], band_pred_sum[0]),
        "predicted_upper": (band_pred_mean[1], band_pred_sum[1]),
        "predicted_sd": (sd(pred_mean), sd(pred_sum)),
        "abs_effect": (obs_mean - avg_pred, obs_sum - cum_pred),
        "abs_effect_lower": (band_point_mean[0], band_point_sum[0]),
        "abs_effect_upper": (band_point_mean[1], band_point_sum[1]),
        "abs_effect_sd": (sd(point_mean), sd(point_sum)),
        "rel_effect": (rel.mean(axis=1),) * 2,
        "rel_effect_lower": (band_rel[0],) * 2,
        "rel_effect_upper": (band_rel[1],) * 2,
        "rel_effect_sd": (sd(rel),) * 2,
    }
  pool_le = ((obs_sum[:, None] <= pred_sum).sum(axis=1) + 1) / (pred_sum.shape[1] + 1)
  pool_ge = ((obs_sum[:, None] >= pred_sum).sum(axis=1) + 1) / (pred_sum.shape[1] + 1)
  p_value = np.minimum(pool_le, pool_ge)
  data = {k: np.stack(v, axis=1).reshape(-1) for k, v in cols.items()}      # (b, avg|cum) order
  data["p_value"] = np.repeat(p_value, 2)
  data["alpha"] = np.full(2 * B, alpha)
  index = pd.MultiIndex.from_product([list(names), ["average", "cumulative"]], names=["series", None])
  return pd.DataFrame(data, index=index)


# the component-summary arrays whose last axis is the design columns, not time
_PER_COLUMN = ("inclusion_prob", "weight_mean", "weight_order")


class CausalImpactBatchAnalysis:
  """Results for B series.  `summary`: DataFrame indexed by (series, average|cumulative) with the
  reference's 15 summary columns; `analysis[b]` / iteration: per-series CausalImpactAnalysis
  (the `series` frame is assembled on first access); `diagnostics`: split-R-hat / ESS per series
  when more than one chain was run."""

  def __init__(self, prepared, names, alpha, posterior_means, device_summary, ranks, columns,
               diagnostic_draws, component_summary=None):
    self._prep, self._names, self.alpha = prepared, list(names), alpha
    # {name: [B, ...]} of ci_session_summarize_components (InferenceOptions.components), or None
    self._csum = component_summary
    self._means, self._dsum, self._ranks, self._columns = posterior_means, device_summary, ranks, columns
    # {key: [B, chains, draws]} of the scalars the diagnostics rank, or None for one chain.  The
    # diagnostics themselves (three rank / FFT passes per key per series) are computed on access:
    # for thousands of series they would otherwise cost more host time than the device fit.
    self._diag_draws = diagnostic_draws
    self._diag: Dict[int, Dict] = {}
    self._cache: Dict[int, lib.CausalImpactAnalysis] = {}
    self.summary = self._build_summary()

  def diagnostics_of(self, b: int):
    """{"split_rhat" | "ess_bulk" | "ess_tail": {key: value}} of series b (None for one chain)."""
    if self._diag_draws is None:
      return None
    b = range(len(self))[b]
    if b not in self._diag:
      d = {k: v[b] for k, v in self._diag_draws.items()}
      self._diag[b] = {
          "split_rhat": {k: lib.split_rhat(v) for k, v in d.items()},
          "ess_bulk": {k: lib.effective_sample_size(v, "bulk") for k, v in d.items()},
          "ess_tail": {k: lib.effective_sample_size(v, "tail") for k, v in d.items()}}
    return self._diag[b]

  @property
  def diagnostics(self):
    """{"split_rhat" | "ess_bulk" | "ess_tail": [per-series {key: value}]} for ALL series (computed
    now, O(B) host work); None when a single chain was run."""
    if self._diag_draws is None:
      return None
    per = [self.diagnostics_of(b) for b in range(len(self))]
    return {name: [p[name] for p in per] for name in ("split_rhat", "ess_bulk", "ess_tail")}

  def __len__(self):
    return len(self._names)

  def _request(self, b: int) -> Dict:
    p = self._prep
    idx = p.index[p.model_rows]
    in_post = np.asarray((idx >= p.post_period[0]) & (idx <= p.post_period[1]))
    obs = p.values[b, p.model_rows, 0].copy()
    obs[p.num_pre:][~in_post[p.num_pre:]] = np.nan        # gap / tail: predictions only
    flags = (~np.asarray(idx < p.post_period[0])).astype(np.uint8) | (in_post.astype(np.uint8) << 1)
    return dict(scale=float(p.outcome_sd[b]) if p.standardize_data else 1.0,
                shift=float(p.outcome_mean[b]) if p.standardize_data else 0.0,
                observed=obs, flags=flags, ranks=self._ranks,
                quantiles=(self.alpha / 2.0, 1.0 - self.alpha / 2.0))

  def _build_summary(self) -> pd.DataFrame:
    """The reference's 15 summary columns (causalimpact_lib.py:934-1093) for every series at
    once: the same numpy reductions as `_summary_rows`, along axis 1 of [B, draws] arrays."""
    p, B = self._prep, len(self)
    rq = self._request(0)
    win = (rq["flags"] & 2) != 0
    n_win = int(win.sum())
    idx = p.index[p.model_rows]
    in_post = np.asarray((idx >= p.post_period[0]) & (idx <= p.post_period[1]))
    obs = p.values[:, p.model_rows, 0].copy()
    obs[:, p.num_pre:][:, ~in_post[p.num_pre:]] = np.nan
    obs_w = obs[:, win]                                                    # [B, T_w]
    scale = p.outcome_sd if p.standardize_data else np.ones(B)
    shift = p.outcome_mean if p.standardize_data else np.zeros(B)
    post_mean = (self._means.astype(np.float64) * scale[:, None] + shift[:, None])[:, win]
    n_obs = np.sum(~np.isnan(obs_w), axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
      obs_mean, obs_sum = np.nanmean(obs_w, axis=1), np.nansum(obs_w, axis=1)
    return summary_table(self._names, self.alpha, self._ranks, self._dsum, n_win=n_win, n_obs=n_obs,
                         obs_mean=obs_mean, obs_sum=obs_sum, avg_pred=post_mean.mean(axis=1),
                         cum_pred=post_mean.sum(axis=1))

  def __getitem__(self, b: int) -> lib.CausalImpactAnalysis:
    b = range(len(self))[b]
    if b not in self._cache:
      p = self._prep
      df = pd.DataFrame(p.values[b], index=p.index, columns=self._columns)
      ci_data = cid.CausalImpactData(df, p.pre_period, p.post_period,
                                     standardize_data=p.standardize_data)
      dsum = {k: v[b] for k, v in self._dsum.items()}
      rq = lib._device_summary_request(ci_data, self.alpha)   # pylint: disable=protected-access
      rq["ranks"] = self._ranks
      series, summary = lib._compute_impact_device(            # pylint: disable=protected-access
          self._means[b], dsum, rq, ci_data, self.alpha)
      self._cache[b] = lib.CausalImpactAnalysis(series, summary, None, self.diagnostics_of(b),
                                                *self._component_frames(b, ci_data))
    return self._cache[b]

  def _component_frames(self, b: int, ci_data, num_steps: Optional[int] = None):
    """(components, coefficients) of series b (its first `num_steps` steps: a panel's arrays are
    padded to the longest series), or (None, None) when they were not asked for."""
    if self._csum is None:
      return None, None
    csum = {k: (v[b] if k in _PER_COLUMN or num_steps is None
                else v[b][..., :num_steps]) for k, v in self._csum.items()}
    return lib._component_frames(                               # pylint: disable=protected-access
        csum, self._ranks, self._dsum["per_draw"].shape[-1], self.alpha,
        lib.posterior_processing.model_index(ci_data), ci_data.data.index,
        list(ci_data.feature_ts.columns) if ci_data.feature_ts is not None else None)

  def __iter__(self):
    return (self[b] for b in range(len(self)))


class PerSeriesBatchAnalysis(CausalImpactBatchAnalysis):
  """The same container over analyses that were fitted one series at a time (the routes the
  one-launch path does not have: float64 compute, raw-scale outcomes)."""

  def __init__(self, names, alpha, analyses):   # pylint: disable=super-init-not-called
    self._names, self.alpha = list(names), alpha
    self._cache = dict(enumerate(analyses))
    self._diag_draws = None
    self.summary = pd.concat([a.summary for a in analyses], keys=self._names, names=["series", None])

  def diagnostics_of(self, b: int):
    return self._cache[range(len(self))[b]].diagnostics

  @property
  def diagnostics(self):
    per = [self.diagnostics_of(b) for b in range(len(self))]
    if any(p is None for p in per):
      return None
    return {name: [p[name] for p in per] for name in ("split_rhat", "ess_bulk", "ess_tail")}

  def __getitem__(self, b: int) -> lib.CausalImpactAnalysis:
    return self._cache[range(len(self))[b]]


# The one-launch HMC path (csrc/ci_hmc.h with a series axis, ci_ll_session_create_batch) covers
# standardised float32 trend models of at most this many steps and design columns started at the
# Gibbs initial state; every other HMC batch is fitted series by series.
HMC_BATCH_MAX_T = 4096
HMC_BATCH_MAX_P = 128


def hmc_batch_route(*, float64: bool, standardize_data: bool, num_seasonal_blocks: int, T: int,
                    P: int, hmc_init: str) -> str:
  """Where `fit_causalimpact_batch(sampler="hmc")` fits a batch: "one_launch" (all series x chains
  in one kernel launch per device and HBM budget) or "per_series" (`fit_causalimpact` on every
  series in turn, with the series' key: seasonal blocks, T > 4096, P > 128, hmc_init="vi", float64,
  standardize_data=False -- the refusals of the single-series path stay where they are)."""
  if (float64 or not standardize_data or num_seasonal_blocks > 0 or T > HMC_BATCH_MAX_T
      or P > HMC_BATCH_MAX_P or hmc_init != "gibbs"):
    return "per_series"
  return "one_launch"


def fit_causalimpact_batch(data: Union[Sequence[pd.DataFrame], np.ndarray],
                           pre_period, post_period, alpha: float = 0.05, seed=None,
                           data_options: Optional[lib.DataOptions] = None,
                           model_options: Optional[lib.ModelOptions] = None,
                           inference_options: Optional[lib.InferenceOptions] = None,
                           index: Optional[pd.Index] = None,
                           names: Optional[Sequence[Any]] = None,
                           shared_streams: bool = False) -> CausalImpactBatchAnalysis:
  """`fit_causalimpact` for B series at once.

  data: a sequence of DataFrames with identical index and column layout (outcome first, or
  `DataOptions.outcome_column`), or an array [B, T, 1 + covariates] (outcome first) with
  `index` (default: 0..T-1).  Other arguments as `fit_causalimpact`.  Series that do NOT share
  the index and the periods (own lengths, own intervention dates) go to `fit_causalimpact_panel`.  Latent-state draws are not
  downloaded (B x chains x draws x T values); the per-series frames and the summary table are.

  Random streams: series b draws from streams keyed by (its position b in the batch, chain), so
  the Monte-Carlo errors of different series are independent (pooling effects over geos averages
  them out) and the result does not depend on how the batch is split over devices.  Series 0 of
  a batch equals `fit_causalimpact` on that series alone with the same seed.
  `shared_streams=True` keys the streams by chain only: EVERY series then reproduces its
  single-series fit draw for draw, at the price of perfectly correlated Monte-Carlo errors.
  "Equals" is bit for bit on every route: the kernel a series runs on is a function of its model
  and length alone (trend models, trend + one block of 2-7 seasons, and the general seasonal /
  more-than-52-covariate routes alike), never of the batch size or the device's CU count; the
  launch size only decides how many workgroups share one chain's work, which does not change the
  arithmetic (tests/test_gpu_gibbs.py, including a seasonal batch with more chains than CUs).
  `InferenceOptions.kernel_flags` (e.g. `_native.FLAG_SEQUENTIAL_SEASONAL`: 1.5-1.7x the throughput
  for batches of hundreds of short multi-block series) applies to the batch as to a single fit: give
  it to both when comparing them.

  `DataOptions.dtype=float64` and `standardize_data=False` batches are NOT one launch: they are
  fitted series by series on the single-series routes (float64 kernels / exact internal
  conditioning), i.e. B sequential fits on one device -- B times the cost of one fit, and
  `inference_options.devices` is not used to shard them.  Their streams are keyed per series in
  the same way (series b on the key of series id b) unless `shared_streams=True`.

  `InferenceOptions(sampler="hmc")`: standardised float32 batches of trend models with T <= 4096,
  at most 128 design columns and `hmc_init="gibbs"` (either `hmc_prior`) run in one launch per
  device: B x num_chains HMC chains (csrc/ci_hmc.h), then the latent paths, predictive
  trajectories and their summary on the device.  A shard whose trajectories would exceed
  `_hmc.HMC_BATCH_HBM_BYTES` is fitted in several launches; neither that split nor the one over
  devices changes a result.  Every other HMC batch (seasonal blocks, longer series,
  `hmc_init="vi"`, float64, `standardize_data=False`) is fitted series by series through
  `fit_causalimpact`, keyed as above (`hmc_batch_route`).  With `shared_streams=True` series b
  equals `fit_causalimpact(..., sampler="hmc")` on it alone on either route.
  """
  data_options = data_options or lib.DataOptions()
  model_options = model_options or lib.ModelOptions()
  inference_options = inference_options or lib.InferenceOptions()
  if not 0 < alpha < 1:
    raise ValueError("`alpha` must be between 0 and 1.")
  if inference_options.sampler not in ("gibbs", "hmc"):
    raise ValueError(f"sampler must be 'gibbs' or 'hmc', got {inference_options.sampler!r}")
  hmc = inference_options.sampler == "hmc"
  if isinstance(data, np.ndarray):
    values = np.asarray(data, np.float64)
    index = pd.RangeIndex(values.shape[1]) if index is None else pd.Index(index)
    columns = ["y"] + [f"x{j}" for j in range(values.shape[2] - 1)]
  else:
    frames = [pd.DataFrame(d) for d in data]
    if not frames:
      raise ValueError("`data` is empty")
    first = frames[0]
    oc = data_options.outcome_column if data_options.outcome_column is not None else first.columns[0]
    columns = [oc] + [c for c in first.columns if c != oc]
    for f in frames:
      if not f.index.equals(first.index) or list(f.columns) != list(first.columns):
        raise ValueError("all series of a batch must share the index and the columns")
    values = np.stack([f[columns].to_numpy(dtype=np.float64) for f in frames])
    index = first.index
  B = values.shape[0]
  names = list(range(B)) if names is None else list(names)
  float64 = cid._as_numpy_dtype(data_options.dtype) == np.float64  # pylint: disable=protected-access
  prep = None
  per_series = float64 or not data_options.standardize_data
  if hmc and not per_series:
    prep = prepare_batch(values, index, pre_period, post_period, data_options.standardize_data)
    route = hmc_batch_route(float64=float64, standardize_data=data_options.standardize_data,
                            num_seasonal_blocks=len(_model.expand_seasons(model_options.seasons,
                                                                          prep.y.shape[1])[0]),
                            T=prep.y.shape[1],
                            P=0 if prep.design is None else prep.design.shape[2],
                            hmc_init=inference_options.hmc_init)
    # the one-launch HMC path keeps no latent draws and has no component summary: asked for
    # components, an HMC batch takes the per-series route, where `fit_causalimpact` has the draws
    per_series = route == "per_series" or inference_options.components
  if per_series:
    # float64 compute (csrc/ci_gibbs64.h) and raw-scale outcomes (their per-series internal
    # conditioning, causalimpact_lib._internal_conditioning) exist on the single-series path: the
    # batch is fitted series by series there -- same container, same summary table, every series
    # keyed like the one-launch path (series b on the Philox key of series id b,
    # ci_series_stream_key, so the Monte-Carlo errors of different series are independent; with
    # shared_streams=True every series equals `fit_causalimpact` on it alone with this seed).
    # Not the one-launch path: B sequential fits on one device (see the docstring).  The HMC
    # batches the one-launch path does not take (hmc_batch_route) come here too.
    opts = dataclasses.replace(data_options, outcome_column=columns[0])
    analyses = []
    base_seed = lib._sanitize_seed(seed)   # pylint: disable=protected-access
    for b in range(B):
      seed_b = base_seed if shared_streams else _native.series_stream_key(base_seed, b)
      one = lib.fit_causalimpact(pd.DataFrame(values[b], index=index, columns=columns), pre_period,
                                 post_period, alpha=alpha, seed=seed_b, data_options=opts,
                                 model_options=model_options, inference_options=inference_options)
      analyses.append(dataclasses.replace(one, posterior_samples=None))   # (draws are not kept)
    return PerSeriesBatchAnalysis(names, alpha, analyses)
  if prep is None:
    prep = prepare_batch(values, index, pre_period, post_period, data_options.standardize_data)
  T = prep.y.shape[1]
  P = 0 if prep.design is None else prep.design.shape[2]
  num_seasons, season_change = _model.expand_seasons(model_options.seasons, T)
  # the sampler sees the outcome in DataOptions.dtype (data.py:121-128), priors included
  y_model = prep.y.astype(cid._as_numpy_dtype(data_options.dtype)).astype(np.float64)  # pylint: disable=protected-access
  with np.errstate(invalid="ignore"):
    pre_sd = np.nanstd(y_model[:, :prep.num_pre], axis=1, ddof=1)
  params = [_model.series_params(y_model[b], prep.mask[b],
                                 None if prep.design is None else prep.design[b],
                                 prior_level_sd=model_options.prior_level_sd,
                                 num_seasonal_blocks=len(num_seasons),
                                 has_slope=model_options.local_linear_trend,
                                 outcome_sd=float(pre_sd[b])) for b in range(B)]
  seed_pair = lib._sanitize_seed(seed)   # pylint: disable=protected-access
  C, S = inference_options.num_chains, inference_options.num_results
  ranks = lib._summary_ranks(C * S, (alpha / 2.0, 1.0 - alpha / 2.0))   # pylint: disable=protected-access
  idx = index[prep.model_rows]
  in_post = np.asarray((idx >= prep.post_period[0]) & (idx <= prep.post_period[1]))
  flags = (~np.asarray(idx < prep.post_period[0])).astype(np.uint8) | (in_post.astype(np.uint8) << 1)
  observed = values[:, prep.model_rows, 0].copy()
  observed[:, prep.num_pre:][:, ~in_post[prep.num_pre:]] = np.nan
  devs = list(inference_options.devices) if inference_options.devices else [0]
  shards = [s for s in np.array_split(np.arange(B), len(devs)) if len(s)]

  def run_hmc(dev, ids):
    # one launch per part of the shard that fits the HBM budget; series keep their global ids
    from causalimpact import _hmc  # pylint: disable=import-outside-toplevel
    step = _hmc.series_per_launch(T, P, C, S)
    outs, sums = [], []
    for lo in range(0, len(ids), step):
      part = ids[lo:lo + step]
      res = _hmc.fit_hmc_batch(
          y_model[part], prep.mask[part], None if prep.design is None else prep.design[part],
          [params[b] for b in part], has_slope=model_options.local_linear_trend, num_results=S,
          num_warmup=inference_options.num_warmup_steps, num_chains=C, seed=seed_pair, device=dev,
          series_offset=int(part[0]), shared_streams=shared_streams,
          prior=inference_options.hmc_prior,
          summary=dict(scale=prep.outcome_sd[part] if prep.standardize_data else 1.0,
                       shift=prep.outcome_mean[part] if prep.standardize_data else 0.0,
                       observed=observed[part], flags=flags, ranks=ranks))
      outs.append(res)
      sums.append(res["summary"])
    out = {k: np.concatenate([o[k] for o in outs], axis=0)
           for k in ("posterior_means", "observation_noise_scale", "level_scale")}
    return out, {k: np.concatenate([d[k] for d in sums], axis=0) for k in sums[0]}

  def run(dev, ids):
    if hmc:
      return run_hmc(dev, ids)
    pb = _native.make_problem(T=T, P=P, has_slope=model_options.local_linear_trend,
                              num_seasons=num_seasons, num_warmup=inference_options.num_warmup_steps,
                              num_results=S, num_chains=C, num_series=len(ids), seed=seed_pair,
                              device=dev, series_offset=int(ids[0]),
                              flags=int(getattr(inference_options, "kernel_flags", 0)) |
                              (_native.FLAG_SHARED_SERIES_STREAMS if shared_streams else 0))
    sess = _native.Session(pb, y_model[ids], prep.mask[ids],
                           None if prep.design is None else prep.design[ids], season_change,
                           _native.make_params([params[b] for b in ids]))
    try:
      sess.run()
      out = sess.fetch(["posterior_means", "observation_noise_scale", "level_scale"])
      dsum = sess.summarize(prep.outcome_sd[ids] if prep.standardize_data else 1.0,
                            prep.outcome_mean[ids] if prep.standardize_data else 0.0,
                            observed[ids], flags, ranks)
      if len(ids) == 1:
        dsum = {k: v[None] for k, v in dsum.items()}
      if inference_options.components:
        out["components"] = sess.summarize_components(
            prep.outcome_sd[ids] if prep.standardize_data else 1.0,
            prep.outcome_mean[ids] if prep.standardize_data else 0.0, ranks)
    finally:
      sess.close()
    return out, dsum

  if len(shards) == 1:
    # one device: no worker thread (a fresh host thread pays the runtime's per-thread set-up,
    # ~30 ms, more than the fit of 512 series takes)
    results = [run(devs[0], shards[0])]
  else:
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(shards)) as pool:
      results = list(pool.map(lambda a: run(*a), zip(devs, shards)))
  means = np.concatenate([r[0]["posterior_means"].mean(axis=1) for r in results], axis=0)   # [B, T]
  dsum = {k: np.concatenate([r[1][k] for r in results], axis=0) for k in results[0][1]}
  diag_draws = None
  if C > 1:
    keys = ("observation_noise_scale", "level_scale")
    diag_draws = {k: np.concatenate([r[0][k] for r in results], axis=0) for k in keys}   # [B, C, S]
  csum = None
  if inference_options.components:
    csum = {k: np.concatenate([r[0]["components"][k] for r in results], axis=0)
            for k in results[0][0]["components"]}
  return CausalImpactBatchAnalysis(prep, names, alpha, means, dsum, ranks, columns, diag_draws, csum)


# ------------------------------------------------------------------------------------------
# Panels: B series with the same columns, each with its own index, length and periods
# ------------------------------------------------------------------------------------------
# The ragged one-launch path (csrc/ci_kernels.h, the RAGGED build of the four-wavefront trend
# kernel; ci_session_create_ragged) covers standardised float32 Gibbs trend models of at most this
# many steps and design columns; all series of a launch run the same number of steps per thread.
PANEL_RAGGED_MAX_T = 4096
PANEL_RAGGED_MAX_P = 52


def steps_class(T: int) -> int:
  """Steps per thread of the register-resident trend kernels for a series of T steps: the
  smallest L in (1, 2, 4, 8, 16) with 256 L >= T; 0 beyond 4096 steps."""
  for L in (1, 2, 4, 8, 16):
    if 256 * L >= T:
      return L
  return 0


# The ragged seasonal one-launch path (csrc/ci_wide.h, the RAGGED build of the time-parallel kernel;
# ci_session_create_ragged_seasonal) covers standardised float32 Gibbs models of trend plus ONE block
# of 2..7 seasons with at most PANEL_RAGGED_MAX_P design columns and this many steps; all series of a
# launch share the chunk length of the draw's grid.
PANEL_SEASONAL_MAX_T = 65536
PANEL_SEASONAL_MAX_SEASONS = 7


def seasonal_steps_class(T: int) -> int:
  """Steps per chunk of the time-parallel seasonal kernel's grid of 512 chunks for a series of T
  steps (csrc/ci_wide.h: wide_quad_steps): 4 up to 2048 steps, then ceil(T / 512) rounded up to a
  multiple of 4."""
  lc = -(-int(T) // 512)
  return 4 if lc < 4 else (lc + 3) & ~3


def panel_route(*, float64: bool, standardize_data: bool, sampler: str, num_seasonal_blocks: int,
                P: int, lengths: Sequence[int],
                num_seasons: Optional[Sequence[int]] = None) -> Dict[str, Any]:
  """Where `fit_causalimpact_panel` fits a panel whose series b has lengths[b] model steps.

  {"route": ..., "groups": [(key, [series positions]), ...]}, groups in ascending key order, the
  positions of a group ascending:
    "ragged"        trend model, P <= 52, every length <= 4096, float32, standardised, Gibbs: series
                    grouped by steps-per-thread class (key = L), one ragged launch per class (and
                    device);
    "ragged_seasonal"  (only when `num_seasons`, the seasons of every block, is given) trend plus ONE
                    block of 2..7 seasons, P <= 52, every length <= 65536, float32, standardised,
                    Gibbs: series grouped by `seasonal_steps_class` (key = steps per chunk), one
                    ragged launch of the time-parallel kernel per class (and device);
    "equal_length"  any other float32 standardised Gibbs model (other seasonal blocks, P > 52, a
                    trend series longer than 4096): series grouped by equal length (key = T), one
                    ordinary session per distinct length -- the existing kernels, per-series mask /
                    flags;
    "per_series"    float64, standardize_data=False, sampler="hmc": `fit_causalimpact` on every
                    series in turn (one group per series, key = its position).
  A series' random streams are keyed by its POSITION IN THE PANEL on every route (the positions
  listed here are what the launches pass on), never by its place in a group."""
  lengths = [int(t) for t in lengths]
  if float64 or not standardize_data or sampler != "gibbs":
    return dict(route="per_series", groups=[(b, [b]) for b in range(len(lengths))])
  ragged = (num_seasonal_blocks == 0 and P <= PANEL_RAGGED_MAX_P and
            all(t <= PANEL_RAGGED_MAX_T for t in lengths))
  seasonal = (num_seasons is not None and num_seasonal_blocks == 1 and len(num_seasons) == 1 and
              2 <= int(num_seasons[0]) <= PANEL_SEASONAL_MAX_SEASONS and P <= PANEL_RAGGED_MAX_P and
              all(t <= PANEL_SEASONAL_MAX_T for t in lengths))
  key_of = steps_class if ragged else (seasonal_steps_class if seasonal else (lambda t: t))
  groups: Dict[int, List[int]] = {}
  for b, t in enumerate(lengths):
    groups.setdefault(key_of(t), []).append(b)
  name = "ragged" if ragged else ("ragged_seasonal" if seasonal else "equal_length")
  return dict(route=name, groups=sorted(groups.items()))


def panel_launches(route: Dict[str, Any], devices: Sequence[int], shared_streams: bool = False):
  """[(device, key, [series positions])]: the launches of a routed panel.  Every group is sharded
  over the devices as a batch is.  The ragged entry points take the positions as `series_ids`, so
  a shard is one launch whatever its positions are; an ordinary session keys series b of the launch
  by series_offset + b, so on the "equal_length" route a shard is cut into runs of consecutive
  positions (one launch each) -- unless the streams are shared, when no position enters a key."""
  devs = list(devices) if devices else [0]
  out = []
  for key, ids in route["groups"]:
    for dev, part in zip(devs, np.array_split(np.asarray(ids, dtype=np.int64), len(devs))):
      part = [int(b) for b in part]
      if not part:
        continue
      if route["route"] == "equal_length" and not shared_streams:
        run = [part[0]]
        for b in part[1:]:
          if b != run[-1] + 1:
            out.append((dev, key, run))
            run = []
          run.append(b)
        out.append((dev, key, run))
      else:
        out.append((dev, key, part))
  return out


@dataclasses.dataclass
class PreparedPanel:
  """What the sampler consumes for a panel: `PreparedBatch` with a length per series.  Arrays over
  time are padded to the longest series: y NaN, mask True, design 0, observed NaN, flags 0."""
  raw: List[np.ndarray]         # per series [T_all_b, 1+p] raw data
  indices: List[pd.Index]       # per series [T_all_b]
  periods: List[Tuple[Tuple[Any, Any], Tuple[Any, Any]]]   # parsed (pre_period, post_period)
  standardize_data: bool
  model_rows: List[np.ndarray]  # per series: positions (into its index) of its model steps
  lengths: np.ndarray           # [B] model steps T_b
  num_pre: np.ndarray           # [B] steps of the own pre-period
  y: np.ndarray                 # [B, T_max]
  mask: np.ndarray              # [B, T_max] bool
  design: Optional[np.ndarray]  # [B, T_max, P] or None
  outcome_mean: np.ndarray      # [B]
  outcome_sd: np.ndarray        # [B]
  observed: np.ndarray          # [B, T_max] data-scale outcome, NaN in gap / tail / padding
  flags: np.ndarray             # [B, T_max] uint8: bit 0 = t >= treatment start, bit 1 = in the window


def prepare_panel(frames_or_values, periods, standardize_data: bool = True,
                  indices_: Optional[Sequence[pd.Index]] = None, names=None) -> PreparedPanel:
  """Vectorised `CausalImpactData.__init__` for a panel: a sequence of DataFrames (outcome first)
  or of [T_b, 1 + p] arrays (with `indices_`, default 0..T_b-1), and one (pre_period, post_period)
  per series.  Per series: the rows before its own pre-period are dropped, gap and tail kept, the
  columns standardised by its own pre-period, y NaN from the end of that pre-period on.  The index
  of every series is compared with its own periods (that cannot be shared); the numeric work runs
  on the padded [B, T_max, 1 + p] block -- series with the same pre-period length are standardised
  together, with the very operations of `prepare_batch`.  The reference's refusals are raised
  with the series named."""
  items = list(frames_or_values)
  B = len(items)
  if B == 0:
    raise ValueError("`data` is empty")
  periods = list(periods)
  if len(periods) != B:
    raise ValueError(f"`periods` must hold one (pre_period, post_period) per series: {B} series, "
                     f"{len(periods)} periods")
  names = list(range(B)) if names is None else list(names)
  raw, idxs = [], []
  for b, item in enumerate(items):
    if isinstance(item, (pd.DataFrame, pd.Series)):
      frame = pd.DataFrame(item)
      raw.append(frame.to_numpy(dtype=np.float64))
      idxs.append(frame.index)
    else:
      v = np.asarray(item, dtype=np.float64)
      if v.ndim != 2:
        raise ValueError(f"series {names[b]!r}: values must be [num_timesteps, 1 + num_covariates]")
      raw.append(v)
      idxs.append(pd.RangeIndex(v.shape[0]) if indices_ is None else pd.Index(indices_[b]))
    if len(idxs[b]) != raw[b].shape[0]:
      raise ValueError(f"series {names[b]!r}: the index must have one entry per timestep")
  ncol = raw[0].shape[1]
  for b in range(B):
    if raw[b].shape[1] != ncol:
      raise ValueError(f"series {names[b]!r} has {raw[b].shape[1]} columns, series {names[0]!r} has "
                       f"{ncol}: all series of a panel must share the columns")
  # ---- per series: its periods against its index (positions only; no numeric work)
  parsed, rows_of, in_post_of, after_start_of = [], [], [], []
  n_pre = np.zeros(B, np.int64)
  for b in range(B):
    idx = idxs[b]
    try:
      pre, post = indices.parse_and_validate_date_data(
          data=pd.DataFrame({"y": np.zeros(len(idx))}, index=idx), pre_period=periods[b][0],
          post_period=periods[b][1])
    except ValueError as e:
      raise ValueError(f"series {names[b]!r}: {e}") from e
    parsed.append((pre, post))
    in_pre = np.asarray((idx >= pre[0]) & (idx <= pre[1]))
    rows = np.concatenate([np.flatnonzero(in_pre), np.flatnonzero(np.asarray(idx > pre[1]))])
    n_pre[b] = int(in_pre.sum())
    rows_of.append(rows)
    midx = idx[rows]
    in_post_of.append(np.asarray((midx >= post[0]) & (midx <= post[1])))
    after_start_of.append(~np.asarray(midx < post[0]))
  lengths = np.array([len(r) for r in rows_of], np.int64)
  T_max, T_all = int(lengths.max()), max(v.shape[0] for v in raw)
  # ---- the padded blocks
  values = np.full((B, T_all, ncol), np.nan)
  real = np.zeros((B, T_all), bool)
  rows_pad = np.zeros((B, T_max), np.int64)
  valid = np.arange(T_max)[None, :] < lengths[:, None]                   # [B, T_max]
  in_post = np.zeros((B, T_max), bool)
  after_start = np.zeros((B, T_max), bool)
  for b in range(B):
    values[b, :raw[b].shape[0]] = raw[b]
    real[b, :raw[b].shape[0]] = True
    rows_pad[b, :lengths[b]] = rows_of[b]
    in_post[b, :lengths[b]] = in_post_of[b]
    after_start[b, :lengths[b]] = after_start_of[b]
  # ---- the reference's refusals (data.py:33-62), over every row of the frame as there
  outcome = values[:, :, 0]
  with np.errstate(invalid="ignore"):
    seen = np.sum(~np.isnan(outcome), axis=1)
    const = (seen > 0) & (np.nanstd(np.where(seen[:, None] > 0, outcome, 0.0), axis=1) == 0)
  if const.any():
    raise ValueError(f"series {names[int(np.flatnonzero(const)[0])]!r}: Input response cannot be constant.")
  if (seen < 3).any():
    raise ValueError(f"series {names[int(np.flatnonzero(seen < 3)[0])]!r}: Input data must have at "
                     "least 3 observations.")
  if ncol > 1:
    bad = (np.isnan(values[:, :, 1:]).any(axis=2) & real).any(axis=1)
    if bad.any():
      raise ValueError(f"series {names[int(np.flatnonzero(bad)[0])]!r}: Input data cannot have any "
                       "missing values.")
  model = values[np.arange(B)[:, None], rows_pad]                          # [B, T_max, 1+p]
  model[~valid] = np.nan
  if standardize_data:
    scaled = np.empty_like(model)
    o_mu, o_sd = np.zeros(B), np.ones(B)
    for n in np.unique(n_pre):                 # (one pass for a panel with one pre-period length)
      sel = np.flatnonzero(n_pre == n)
      sc, mu, sd = standardize.standardize_batch(model[sel], int(n))
      scaled[sel], o_mu[sel], o_sd[sel] = sc, mu[:, 0], sd[:, 0]
  else:
    scaled = model
    o_mu, o_sd = np.zeros(B), np.ones(B)
  y = scaled[:, :, 0].copy()
  y[np.arange(T_max)[None, :] >= n_pre[:, None]] = np.nan
  design = None
  if ncol > 1:
    design = np.concatenate([scaled[:, :, 1:], np.ones((B, T_max, 1))], axis=2)
    design[~valid] = 0.0
  observed = model[:, :, 0].copy()
  observed[(np.arange(T_max)[None, :] >= n_pre[:, None]) & ~in_post] = np.nan   # gap / tail: predictions only
  flags = (after_start.astype(np.uint8) | (in_post.astype(np.uint8) << 1)) * valid.astype(np.uint8)
  return PreparedPanel(raw=raw, indices=idxs, periods=parsed, standardize_data=standardize_data,
                       model_rows=rows_of, lengths=lengths, num_pre=n_pre, y=y, mask=np.isnan(y),
                       design=design, outcome_mean=o_mu, outcome_sd=o_sd, observed=observed,
                       flags=flags)


def panel_window_stats(observed: np.ndarray, flags: np.ndarray, post_mean: np.ndarray,
                       lengths: Sequence[int]) -> Dict[str, np.ndarray]:
  """The window statistics `summary_table` needs when every series has its own post-period window:
  observed, flags, post_mean [B, T_max] (data scale; bit 1 of flags marks the window), lengths [B].
  Per series the reductions of `_summary_rows` over ITS window: n_win, n_obs, obs_mean, obs_sum,
  avg_pred, cum_pred, each [B].  Series that share length and window are reduced together with the
  expressions of `CausalImpactBatchAnalysis._build_summary`: a panel with one shared period gets
  that table, bit for bit."""
  B = len(lengths)
  out = {k: np.zeros(B) for k in ("obs_mean", "obs_sum", "avg_pred", "cum_pred")}
  out["n_win"], out["n_obs"] = np.zeros(B, np.int64), np.zeros(B, np.int64)
  groups: Dict[Any, List[int]] = {}
  for b in range(B):
    groups.setdefault((int(lengths[b]), (flags[b, :lengths[b]] & 2).tobytes()), []).append(b)
  with np.errstate(invalid="ignore", divide="ignore"):
    for (Tg, _), sel in groups.items():
      win = (flags[sel[0], :Tg] & 2) != 0
      obs_w = np.ascontiguousarray(observed[sel][:, :Tg])[:, win]            # [Bg, T_w]
      pm_w = np.ascontiguousarray(post_mean[sel][:, :Tg])[:, win]
      out["n_win"][sel], out["n_obs"][sel] = int(win.sum()), np.sum(~np.isnan(obs_w), axis=1)
      out["obs_mean"][sel], out["obs_sum"][sel] = np.nanmean(obs_w, axis=1), np.nansum(obs_w, axis=1)
      out["avg_pred"][sel], out["cum_pred"][sel] = pm_w.mean(axis=1), pm_w.sum(axis=1)
  return out


class CausalImpactPanelAnalysis(CausalImpactBatchAnalysis):
  """`CausalImpactBatchAnalysis` for a panel: every series has its own index, length and periods,
  hence its own post-period window in the summary table.  `posterior_means` [B, T_max] and the
  device summary's arrays over time are padded to the longest series; series b owns [0, T_b)."""

  def _request(self, b: int) -> Dict:
    p, Tb = self._prep, int(self._prep.lengths[b])
    return dict(scale=float(p.outcome_sd[b]), shift=float(p.outcome_mean[b]),
                observed=p.observed[b, :Tb], flags=p.flags[b, :Tb], ranks=self._ranks,
                quantiles=(self.alpha / 2.0, 1.0 - self.alpha / 2.0))

  def _build_summary(self) -> pd.DataFrame:
    p = self._prep
    post_mean = (self._means.astype(np.float64) * p.outcome_sd[:, None] + p.outcome_mean[:, None])
    stats = panel_window_stats(p.observed, p.flags, post_mean, p.lengths)
    return summary_table(self._names, self.alpha, self._ranks, self._dsum, **stats)

  def __getitem__(self, b: int) -> lib.CausalImpactAnalysis:
    b = range(len(self))[b]
    if b not in self._cache:
      p = self._prep
      Tb = int(p.lengths[b])
      (pre, post) = p.periods[b]
      df = pd.DataFrame(p.raw[b], index=p.indices[b], columns=self._columns)
      ci_data = cid.CausalImpactData(df, pre, post, standardize_data=p.standardize_data)
      dsum = {k: (v[b][..., :Tb] if k in ("value_order", "cum_order") else v[b])
              for k, v in self._dsum.items()}
      rq = lib._device_summary_request(ci_data, self.alpha)   # pylint: disable=protected-access
      rq["ranks"] = self._ranks
      series, summary = lib._compute_impact_device(            # pylint: disable=protected-access
          self._means[b, :Tb], dsum, rq, ci_data, self.alpha)
      self._cache[b] = lib.CausalImpactAnalysis(series, summary, None, self.diagnostics_of(b),
                                                *self._component_frames(b, ci_data, Tb))
    return self._cache[b]


def fit_causalimpact_panel(data: Sequence[pd.DataFrame], periods, alpha: float = 0.05, seed=None,
                           data_options: Optional[lib.DataOptions] = None,
                           model_options: Optional[lib.ModelOptions] = None,
                           inference_options: Optional[lib.InferenceOptions] = None,
                           names: Optional[Sequence[Any]] = None,
                           shared_streams: bool = False) -> CausalImpactBatchAnalysis:
  """`fit_causalimpact` for a PANEL: B series with the same columns (outcome first, or
  `DataOptions.outcome_column`; the same covariates), each with its own index, its own length and
  its own (pre_period, post_period) -- staggered roll-outs, units that enter the data on different
  days, placebo studies that cut one history at many dates.

  data: a sequence of DataFrames; periods: one (pre_period, post_period) per series.  The result
  has the interface of `fit_causalimpact_batch`'s: `summary` indexed by (series,
  average|cumulative), `res[b]` the `CausalImpactAnalysis` of series b on its own index,
  `diagnostics_of`, `len`, iteration.

  Routes (`panel_route`): standardised float32 Gibbs trend models with at most 52 design columns
  and 4096 steps are grouped by steps-per-thread class (<= 256, 512, 1024, 2048, 4096 steps) and
  each class runs in ONE launch per device of the ragged build of the four-wavefront kernel, every
  series on its own length.  Trend plus ONE block of 2..7 seasons (`Seasons(num_seasons=7)` on daily
  data), at most 52 design columns and 65536 steps: grouped by `seasonal_steps_class` (one class up
  to 2048 steps), ONE launch per class and device of the ragged build of the time-parallel kernel.
  Other float32 standardised Gibbs models (other seasonal blocks, more columns, longer trend
  series) are grouped by equal length, one ordinary session per length.  float64,
  `standardize_data=False` and `sampler="hmc"` panels are fitted series by series.

  Random streams as in `fit_causalimpact_batch`: series b draws from the streams of series id b,
  its position in the PANEL, whatever group or device it lands in; `shared_streams=True` keys by
  chain only, and series b then equals `fit_causalimpact` on its frame with its periods and this
  seed (bit for bit in every array the session returns over its own steps); without it series 0
  does, and series b equals the single fit seeded with `_native.series_stream_key(seed, b)`."""
  data_options = data_options or lib.DataOptions()
  model_options = model_options or lib.ModelOptions()
  inference_options = inference_options or lib.InferenceOptions()
  if not 0 < alpha < 1:
    raise ValueError("`alpha` must be between 0 and 1.")
  if inference_options.sampler not in ("gibbs", "hmc"):
    raise ValueError(f"sampler must be 'gibbs' or 'hmc', got {inference_options.sampler!r}")
  frames = [pd.DataFrame(d) for d in data]
  if not frames:
    raise ValueError("`data` is empty")
  B = len(frames)
  periods = list(periods)
  if len(periods) != B:
    raise ValueError(f"`periods` must hold one (pre_period, post_period) per series: {B} series, "
                     f"{len(periods)} periods")
  names = list(range(B)) if names is None else list(names)
  first = frames[0]
  oc = data_options.outcome_column if data_options.outcome_column is not None else first.columns[0]
  columns = [oc] + [c for c in first.columns if c != oc]
  for b, f in enumerate(frames):
    if list(f.columns) != list(first.columns):
      raise ValueError(f"series {names[b]!r}: all series of a panel must share the columns")
  float64 = cid._as_numpy_dtype(data_options.dtype) == np.float64  # pylint: disable=protected-access
  seed_pair = lib._sanitize_seed(seed)   # pylint: disable=protected-access
  num_blocks = len(model_options.seasons)
  # (which panels go series by series does not depend on the lengths: the frames' bound them here)
  if panel_route(float64=float64, standardize_data=data_options.standardize_data,
                 sampler=inference_options.sampler, num_seasonal_blocks=num_blocks,
                 P=len(columns), lengths=[len(f) for f in frames])["route"] == "per_series":
    opts = dataclasses.replace(data_options, outcome_column=oc)
    analyses = []
    for b, f in enumerate(frames):
      seed_b = seed_pair if shared_streams else _native.series_stream_key(seed_pair, b)
      one = lib.fit_causalimpact(f, periods[b][0], periods[b][1], alpha=alpha, seed=seed_b,
                                 data_options=opts, model_options=model_options,
                                 inference_options=inference_options)
      analyses.append(dataclasses.replace(one, posterior_samples=None))   # (draws are not kept)
    return PerSeriesBatchAnalysis(names, alpha, analyses)

  prep = prepare_panel([f[columns] for f in frames], periods, data_options.standardize_data,
                       names=names)
  T_max = prep.y.shape[1]
  P = 0 if prep.design is None else prep.design.shape[2]
  route = panel_route(float64=float64, standardize_data=True, sampler="gibbs",
                      num_seasonal_blocks=num_blocks, P=P, lengths=prep.lengths,
                      num_seasons=_model.expand_seasons(model_options.seasons, 1)[0])
  # the sampler sees the outcome in DataOptions.dtype (data.py:121-128), priors included
  y_model = prep.y.astype(cid._as_numpy_dtype(data_options.dtype)).astype(np.float64)  # pylint: disable=protected-access
  params = []
  with np.errstate(invalid="ignore"):
    for b in range(B):
      Tb, nb = int(prep.lengths[b]), int(prep.num_pre[b])
      params.append(_model.series_params(
          y_model[b, :Tb], prep.mask[b, :Tb], None if prep.design is None else prep.design[b, :Tb],
          prior_level_sd=model_options.prior_level_sd, num_seasonal_blocks=num_blocks,
          has_slope=model_options.local_linear_trend,
          outcome_sd=float(np.nanstd(y_model[b, :nb], ddof=1))))
  C, S = inference_options.num_chains, inference_options.num_results
  ranks = lib._summary_ranks(C * S, (alpha / 2.0, 1.0 - alpha / 2.0))   # pylint: disable=protected-access
  kflags = (int(getattr(inference_options, "kernel_flags", 0)) |
            (_native.FLAG_SHARED_SERIES_STREAMS if shared_streams else 0))
  want = ["posterior_means", "observation_noise_scale", "level_scale"]

  def run(dev, key, ids):
    """One launch: the series `ids` (panel positions) on device `dev`; arrays back at stride T_max."""
    ids = np.asarray(ids, dtype=np.int64)
    T = int(prep.lengths[ids].max())                 # the stride of this launch
    design = None if prep.design is None else prep.design[ids, :T]
    common = dict(T=T, P=P, has_slope=model_options.local_linear_trend,
                  num_warmup=inference_options.num_warmup_steps, num_results=S, num_chains=C,
                  num_series=len(ids), seed=seed_pair, device=dev, flags=kflags)
    par = _native.make_params([params[b] for b in ids])
    observed, flags = prep.observed[ids, :T], prep.flags[ids, :T]
    if route["route"] == "ragged":
      sess = _native.Session.ragged(_native.make_problem(**common), prep.lengths[ids],
                                    y_model[ids, :T], prep.mask[ids, :T], design, par, series_ids=ids)
    elif route["route"] == "ragged_seasonal":
      # the stride: the longest series rounded up to a multiple of 4 (every row 16-byte aligned);
      # the padding as in PreparedPanel -- y NaN, mask True, design 0, observed NaN, flags 0 -- and
      # one table of positional change flags for the launch (every series starts at its own step 0)
      TS = (T + 3) & ~3
      pad = lambda a, fill: np.concatenate(   # pylint: disable=unnecessary-lambda-assignment
          [a[ids, :T], np.full((len(ids), TS - T) + a.shape[2:], fill, a.dtype)], axis=1)
      num_seasons, season_change = _model.expand_seasons(model_options.seasons, TS)
      common["T"] = TS
      sess = _native.Session.ragged(_native.make_problem(num_seasons=num_seasons, **common),
                                    prep.lengths[ids], pad(y_model, np.nan), pad(prep.mask, True),
                                    None if design is None else pad(prep.design, 0.0), par,
                                    series_ids=ids, season_change=season_change)
      observed, flags = pad(prep.observed, np.nan), pad(prep.flags, 0)
    else:
      num_seasons, season_change = _model.expand_seasons(model_options.seasons, T)
      sess = _native.Session(_native.make_problem(num_seasons=num_seasons, series_offset=int(ids[0]),
                                                  **common),
                             y_model[ids, :T], prep.mask[ids, :T], design, season_change, par)
    try:
      sess.run()
      out = sess.fetch(want)
      dsum = sess.summarize(prep.outcome_sd[ids], prep.outcome_mean[ids], observed, flags, ranks)
      if len(ids) == 1:
        dsum = {k: v[None] for k, v in dsum.items()}
      csum = None
      if inference_options.components:
        csum = sess.summarize_components(prep.outcome_sd[ids], prep.outcome_mean[ids], ranks)
    finally:
      sess.close()
    if route["route"] == "ragged_seasonal":      # (back at the stride of the longest series)
      out = {k: (v[..., :T] if k == "posterior_means" else v) for k, v in out.items()}
      dsum = {k: (v[..., :T] if k in ("value_order", "cum_order") else v) for k, v in dsum.items()}
      if csum is not None:
        csum = {k: (v if k in _PER_COLUMN else v[..., :T]) for k, v in csum.items()}
    return ids, T, out, dsum, csum

  launches = panel_launches(route, inference_options.devices, shared_streams)
  by_dev: Dict[int, list] = {}
  for dev, key, ids in launches:
    by_dev.setdefault(dev, []).append((dev, key, ids))
  if len(by_dev) == 1:
    results = [run(*a) for a in launches]
  else:
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(by_dev)) as pool:
      per_dev = list(pool.map(lambda work: [run(*a) for a in work], by_dev.values()))
    results = [r for part in per_dev for r in part]
  R, N = len(ranks), C * S
  means = np.zeros((B, T_max), np.float32)
  dsum = dict(value_order=np.full((B, R, T_max), np.nan), cum_order=np.full((B, R, T_max), np.nan),
              per_draw=np.zeros((B, 2, N)), per_draw_order=np.zeros((B, 2, R)))
  diag_draws = None
  if C > 1:
    diag_draws = {k: np.zeros((B, C, S), np.float32) for k in ("observation_noise_scale", "level_scale")}
  csum = None
  for ids, T, out, ds, cs in results:
    if cs is not None:
      if csum is None:      # over time padded to the longest series with NaN, like the order statistics
        csum = {k: (np.zeros((B,) + v.shape[1:]) if k in _PER_COLUMN
                    else np.full((B,) + v.shape[1:-1] + (T_max,), np.nan)) for k, v in cs.items()}
      for k, v in cs.items():
        if k in _PER_COLUMN:
          csum[k][ids] = v
        else:
          csum[k][ids, ..., :T] = v
    means[ids, :T] = out["posterior_means"].mean(axis=1)
    dsum["value_order"][ids, :, :T] = ds["value_order"]
    dsum["cum_order"][ids, :, :T] = ds["cum_order"]
    dsum["per_draw"][ids] = ds["per_draw"]
    dsum["per_draw_order"][ids] = ds["per_draw_order"]
    if diag_draws is not None:
      for k in diag_draws:
        diag_draws[k][ids] = out[k]
  return CausalImpactPanelAnalysis(prep, names, alpha, means, dsum, ranks, columns, diag_draws, csum)
