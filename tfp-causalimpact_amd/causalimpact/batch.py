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

`fit_causalimpact_batch(..., aggregates={name: members})` also returns the POOLED effect of groups of
series (all geos, a region) with its credible bands: the weighted sum of the members' predictive
trajectories draw by draw, formed on the device that holds them (csrc/ci_pool.h) and chained from
launch to launch in series order, then summarised like any single series.

`fit_causalimpact_panel` is the same for series with their own index, length and periods;
`fit_causalimpact_panel(..., event_aggregates={name: members})` pools groups of them in EVENT TIME,
every series aligned on its own treatment start (the same header and chain, over windows).

Both fit functions are one pipeline over different preparations (`prepare_batch`, one shared
calendar; `prepare_panel`, padded to the longest series):
  * `_options` / `_frames_outcome_first`: defaults, argument checks, outcome-first columns;
  * `_fit_per_series`: the routes without a one-launch kernel (float64, raw scale, most HMC);
  * `panel_route` + `panel_launches`: which series share a launch on which device -- a batch is
    the panel of ONE group of equal lengths, cut into consecutive positions per device;
  * `_run_launch` (Gibbs: ordinary, ragged or ragged seasonal session) or `_run_hmc_launch`: one
    session from creation to close, arrays back with the series axis at the launch's stride -- what
    it fetches and the `causalimpact_lib.SummaryRecord` that `causalimpact_lib.take_summaries` fills
    from the open session (one kind per summary; `_KINDS` says how each is laid out);
  * `aggregate_groups`, `_PoolChain` (`HostPool` on the per-series routes), `_frame_analyses`: the
    aggregates of both -- the group table, the running sums handed from launch to launch, the frames
    of every group.  A calendar aggregate is an event-time aggregate whose members all start at step
    0 with the width T, so one chain and one host pool serve both, given the axes or not;
  * `PlaceboPoolPlan`, `_PlaceboChain` (`HostPlaceboPool` on the per-series routes),
    `_take_aggregate_placebo`: the placebo forecasts of the pooled effects (`placebo=` with
    aggregates) -- per entry of the group table the member's origins, a second chain next to
    `_PoolChain` for the sums [G, O, 2, N] of csrc/ci_placebo.h, the frames of every group; with a
    `SimulatedPool` (`Placebo(simulate=True, pool=True)`) the same chain for the sums [G, O, N] of the
    members' simulated totals;
  * `pool_weighted` + `_aggregate_analyses` (a batch) and `event_axes` / `event_plan`,
    `pool_event_weighted` + `_event_aggregate_analyses` (a panel): what differs -- every group's axis
    around its members' own treatment starts, the pooled outcome and posterior mean, the rows of
    `_frame_analyses`;
  * `_assemble`: the launches of a device in turn, the devices side by side
    (`causalimpact_lib.map_by_device`), then the [B, ..., T_max] blocks of the containers.
"""
from __future__ import annotations

import concurrent.futures
import dataclasses
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

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
  observed: np.ndarray        # [B, T] data-scale outcome, NaN in gap / tail (predictions only)
  flags: np.ndarray           # [T] uint8: bit 0 = t >= treatment start, bit 1 = in the window
  # `outcome_link` (`_under_link`): the `_native.LINK_*`, and the prepared batch of the model's copy
  # (log y); `values` and `observed` here are then the RAW outcome's, everything the sampler reads the model's
  link: int = 0
  model: Optional["PreparedBatch"] = None


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
  idx = index[rows]
  in_post = np.asarray((idx >= post[0]) & (idx <= post[1]))
  flags = (~np.asarray(idx < post[0])).astype(np.uint8) | (in_post.astype(np.uint8) << 1)
  observed = values[:, rows, 0].copy()
  observed[:, n_pre:][:, ~in_post[n_pre:]] = np.nan        # gap / tail: predictions only
  return PreparedBatch(values=values, index=index, pre_period=pre, post_period=post,
                       standardize_data=standardize_data, model_rows=rows, num_pre=n_pre, y=y,
                       mask=mask, design=design, outcome_mean=o_mu, outcome_sd=o_sd,
                       observed=observed, flags=flags)


def _under_link(model_prep, raw_prep, link: int):
  """The prepared batch or panel of a fit under `outcome_link`: what the sampler reads (y, mask, design,
  the outcome's mean and sd) comes from `model_prep`, prepared from the model's copy (log y, log1p y);
  what the data-scale frames read -- the raw values and `observed` -- from `raw_prep`, prepared from the
  input as it came.  `model` keeps `model_prep` for what describes the model (components, prediction
  errors)."""
  own = dict(raw=raw_prep.raw) if isinstance(model_prep, PreparedPanel) else dict(values=raw_prep.values)
  return dataclasses.replace(model_prep, observed=raw_prep.observed, link=link, model=model_prep, **own)


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


# ------------------------------------------------------------------------------------------
# Effect windows: the summary over sub-windows of the post-period
# ------------------------------------------------------------------------------------------
def calendar_windows(index: pd.DatetimeIndex, post_period, freq) -> Dict[str, Tuple[Any, Any]]:
  """`effect_windows` of a fit on a DatetimeIndex: one window per pandas period of `freq` ("W", "M",
  ...) that holds a row of the post-period, clipped to the post-period and named by the period's
  label.  post_period as the fit takes it (labels, aligned to the index)."""
  index = pd.DatetimeIndex(index)
  start, end = indices._align(                                  # pylint: disable=protected-access
      tuple(indices._to_index_value(v, index) for v in post_period), index)   # pylint: disable=protected-access
  out = {}
  for period in pd.period_range(start, end, freq=freq):
    rows = index[(index >= max(period.start_time, start)) & (index <= min(period.end_time, end))]
    if len(rows):
      out[str(period)] = (rows[0], rows[-1])
  return out


def event_windows(width: int, num: int) -> Dict[str, Tuple[int, int]]:
  """`effect_windows` of a panel: `num` consecutive windows of `width` rows in event time, named
  "0..6", "7..13", ... (both ends inclusive)."""
  width, num = int(width), int(num)
  if width < 1 or num < 1:
    raise ValueError(f"`width` and `num` must be >= 1, got {width} and {num}")
  return {f"{k * width}..{(k + 1) * width - 1}": (k * width, (k + 1) * width - 1) for k in range(num)}


@dataclasses.dataclass
class WindowPlan:
  """The resolved `effect_windows` of a batch or panel: the window names and, per series and
  window, the model steps first .. first + count - 1 (count 0: the series does not cover it)."""
  names: List[Any]
  first: np.ndarray           # [B, W] int32
  count: np.ndarray           # [B, W] int32
  # batches: the `lib.EffectWindow`s every series shares; panels: the (tau_first, tau_last) pairs
  windows: List[Any]


def batch_windows(effect_windows, prep: PreparedBatch) -> WindowPlan:
  """The `WindowPlan` of a prepared batch: labels on the shared index, as `fit_causalimpact` reads
  them (`lib.resolve_windows`), the same steps for every series."""
  wins = lib.resolve_windows(effect_windows, prep.index, prep.index[prep.model_rows], prep.post_period)
  B = prep.y.shape[0]
  return WindowPlan([w.name for w in wins],
                    np.tile(np.array([w.first for w in wins], np.int32), (B, 1)),
                    np.tile(np.array([w.count for w in wins], np.int32), (B, 1)), wins)


def _tau_windows(effect_windows):
  """[(name, tau_first, tau_last)] of a panel's `effect_windows`; ValueError with the window named."""
  out = []
  for name, bounds in lib._window_items(effect_windows):       # pylint: disable=protected-access
    if not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in bounds):
      raise ValueError(f"effect window {name!r}: the bounds of a panel's window are integers in event "
                       f"time, got {tuple(bounds)!r}")
    lo, hi = int(bounds[0]), int(bounds[1])
    if not 0 <= lo <= hi:
      raise ValueError(f"effect window {name!r}: need 0 <= tau_first <= tau_last, got ({lo}, {hi})")
    out.append((name, lo, hi))
  return out


def panel_windows(effect_windows, prep: PreparedPanel) -> WindowPlan:
  """The `WindowPlan` of a prepared panel: windows (tau_first, tau_last) in event time, the model
  rows since a series' own treatment start (`event_axes`).  Series b covers a window that ends inside
  its post-period window; it then owns the steps start_b + tau_first .. start_b + tau_last, else
  count 0.  ValueError naming the window that no series covers."""
  taus = _tau_windows(effect_windows)
  B = len(prep.lengths)
  first, count = np.zeros((B, len(taus)), np.int32), np.zeros((B, len(taus)), np.int32)
  for b in range(B):
    after = np.flatnonzero(prep.flags[b, :prep.lengths[b]] & 1)
    width = int(np.sum((prep.flags[b] & 2) != 0))
    for w, (_, lo, hi) in enumerate(taus):
      if after.size and hi < width:
        first[b, w], count[b, w] = after[0] + lo, hi - lo + 1
  for w, (name, lo, hi) in enumerate(taus):
    if not count[:, w].any():
      raise ValueError(f"effect window {name!r}: no series has a post-period of {hi + 1} rows to cover "
                       f"({lo}, {hi})")
  return WindowPlan([t[0] for t in taus], first, count, [(lo, hi) for _, lo, hi in taus])


def window_table(names, alpha, ranks, plan: WindowPlan, wsum: Dict[str, np.ndarray],
                 observed: np.ndarray, post_mean: np.ndarray, classes=None) -> pd.DataFrame:
  """`window_summary` of B series: `summary_table` fed with every (series, window)'s own statistics
  -- n_win, n_obs, obs_mean, obs_sum from observed [B, T], avg_pred and cum_pred from post_mean [B, T]
  (data scale), and the window totals wsum ("per_draw" [B, W, 2, N], optionally "per_draw_order"
  [B, W, 2, R]).  Indexed by (series, window, average|cumulative); NaN rows where count is 0.
  classes: [(steps, positions)], the series whose `summary` rows are reduced together over arrays of
  `steps` columns (default: all B over T; a panel: `panel_window_stats`' groups).  Within a class the
  series that share a window's steps are reduced together with the very expressions of
  `_build_summary` -- numpy's summation order depends on the shape of what it reduces -- so that a
  window equal to the post-period gets the `summary` rows bit for bit."""
  B, W = plan.first.shape
  if classes is None:
    classes = [(observed.shape[1], list(range(B)))]
  stats = {k: np.zeros((B, W)) for k in ("obs_mean", "obs_sum", "avg_pred", "cum_pred")}
  stats["n_obs"] = np.zeros((B, W), np.int64)
  with np.errstate(invalid="ignore", divide="ignore"):
    for Tg, members in classes:
      for w in range(W):
        groups: Dict[Any, List[int]] = {}
        for b in members:
          if plan.count[b, w] > 0:
            groups.setdefault((int(plan.first[b, w]), int(plan.count[b, w])), []).append(b)
        for (f, c), sel in groups.items():
          win = np.zeros(Tg, bool)
          win[f:f + c] = True
          obs_w = np.ascontiguousarray(observed[sel][:, :Tg])[:, win]
          pm_w = np.ascontiguousarray(post_mean[sel][:, :Tg])[:, win]
          stats["n_obs"][sel, w] = np.sum(~np.isnan(obs_w), axis=1)
          stats["obs_mean"][sel, w], stats["obs_sum"][sel, w] = np.nanmean(obs_w, axis=1), np.nansum(obs_w, axis=1)
          stats["avg_pred"][sel, w], stats["cum_pred"][sel, w] = pm_w.mean(axis=1), pm_w.sum(axis=1)
  covered = np.flatnonzero(plan.count.reshape(-1) > 0)
  pick = (lambda a: a) if covered.size == B * W else (lambda a: a[covered])   # (a batch: views, no copy)
  flat = {k: pick(v.reshape((B * W,) + v.shape[2:])) for k, v in wsum.items()}
  table = summary_table(covered, alpha, ranks, flat, n_win=pick(plan.count.reshape(-1)).astype(np.int64),
                        **{k: pick(v.reshape(-1)) for k, v in stats.items()})
  rows = (2 * covered[:, None] + np.arange(2)[None, :]).reshape(-1)
  full = np.full((2 * B * W, table.shape[1]), np.nan)
  full[rows] = table.to_numpy(dtype=np.float64)
  index = pd.MultiIndex.from_product([list(names), list(plan.names), ["average", "cumulative"]],
                                     names=["series", "window", None])
  return pd.DataFrame(full, index=index, columns=table.columns)


# What a launch returns has the series axis first and, but for the names a kind lists as whole, time
# last: the kinds of `lib.SummaryRecord` and what a launch fetches -- posterior_means over time and
# the draws of the scalars the diagnostics rank [B, chains, draws], 0 beyond a series' length.
_DRAW_SCALARS = ("observation_noise_scale", "level_scale")
_KINDS = dict(lib.SUMMARY_KINDS, fetched=lib.SummaryKind(_DRAW_SCALARS, 0))


def _cut(arrays: Dict[str, np.ndarray], num_steps: int, kind: str) -> Dict[str, np.ndarray]:
  """`arrays` of `kind` with the time (last) axis cut to `num_steps`."""
  whole = _KINDS[kind].whole + _KINDS[kind].also
  return {k: (v if k in whole else v[..., :num_steps]) for k, v in arrays.items()}


class CausalImpactBatchAnalysis:
  """Results for B series.  `summary`: DataFrame indexed by (series, average|cumulative) with the
  reference's 15 summary columns; `analysis[b]` / iteration: per-series CausalImpactAnalysis
  (the `series` frame is assembled on first access); `diagnostics`: split-R-hat / ESS per series
  when more than one chain was run."""

  def __init__(self, prepared, names, alpha, posterior_means, device_summary, ranks, columns,
               diagnostic_draws, record: Optional[lib.SummaryRecord] = None, state_dim=0,
               placebo_plan=None):
    self._prep, self._names, self.alpha = prepared, list(names), alpha
    record = record if record is not None else lib.SummaryRecord()
    # `placebo=`: placebo_plan dict(origins [B, O] (-1: unused), horizon [B], n_post [B]) with the
    # record's placebo summary {name: [B, O]} as "summary", or None
    self._placebo = None if placebo_plan is None else dict(placebo_plan, summary=record.placebo)
    self._placebo_quality: Optional[pd.DataFrame] = None
    self._placebo_profile: Optional[pd.DataFrame] = None
    # {name: [B, ...]} of ci_session_summarize_components (InferenceOptions.components), or None
    self._csum = record.components
    # {name: [B, ...]} of ci_session_summarize_predictions (InferenceOptions.prediction_errors), or
    # None, and the state dimension of the model (the first step `fit_quality` scores)
    self._psum, self._state_dim = record.predictions, state_dim
    self._quality: Optional[pd.DataFrame] = None
    self._means, self._dsum, self._ranks, self._columns = posterior_means, device_summary, ranks, columns
    # {key: [B, chains, draws]} of the scalars the diagnostics rank, or None for one chain.  The
    # diagnostics themselves (three rank / FFT passes per key per series) are computed on access:
    # for thousands of series they would otherwise cost more host time than the device fit.
    self._diag_draws = diagnostic_draws
    self._diag: Dict[int, Dict] = {}
    self._cache: Dict[int, lib.CausalImpactAnalysis] = {}
    self.summary = self._build_summary()
    # `fit_causalimpact_batch(aggregates=...)`: {aggregate name: CausalImpactAnalysis of the pooled
    # outcome} and the 15-column table indexed by (aggregate, average|cumulative); None otherwise
    self.aggregates: Optional[Dict[Any, lib.CausalImpactAnalysis]] = None
    self.aggregate_summary: Optional[pd.DataFrame] = None
    # `effect_windows=`: the 15 summary columns of every sub-window of the post-period, indexed by
    # (series, window, average|cumulative) -- `analysis[b].window_summary` is the slice of series b --
    # and, with aggregates, the same for every pooled group (aggregate, window, average|cumulative)
    self.window_summary: Optional[pd.DataFrame] = None
    self.aggregate_window_summary: Optional[pd.DataFrame] = None
    # `joint_bands=True` (`set_joint`): `joint_summary`, the `lib.JOINT_SUMMARY_COLUMNS` indexed by
    # (series, pointwise|cumulative), and with `effect_windows` `window_joint_summary`, indexed by
    # (series, window, pointwise|cumulative), NaN where a series does not cover a window;
    # `analysis[b]` carries its own slices and its `joint_bands` frame
    self._joint: Optional[Dict[str, Any]] = None
    self.joint_summary: Optional[pd.DataFrame] = None
    self.window_joint_summary: Optional[pd.DataFrame] = None
    # `joint_bands=True` with aggregates: the same two tables of the pooled groups, indexed by
    # (aggregate, pointwise|cumulative) and (aggregate, window, pointwise|cumulative); every
    # `aggregates[name]` carries its own slices and its `joint_bands` frame
    self.aggregate_joint_summary: Optional[pd.DataFrame] = None
    self.aggregate_window_joint_summary: Optional[pd.DataFrame] = None
    # `placebo=` with aggregates: one row per aggregate with the `lib.PLACEBO_QUALITY_ENTRIES` of its
    # pooled placebo forecasts; every `aggregates[name]` carries its `placebo` and `placebo_quality`
    self.aggregate_placebo_quality: Optional[pd.DataFrame] = None
    # `Placebo(horizons=...)` with aggregates: every aggregate's `placebo_profile`, indexed by (aggregate, horizon)
    self.aggregate_placebo_profile: Optional[pd.DataFrame] = None

  def _model_labels(self, b: int) -> pd.Index:
    """The labels of the model steps of series b."""
    return self._prep.index[self._prep.model_rows]

  def _data_means(self) -> np.ndarray:
    """The posterior means [B, T] on the data scale: the sampler's through every outcome's (sd, mean),
    or under `outcome_link` the means of the linked draws as they are (`value_mean`)."""
    p = self._prep
    if getattr(p, "link", 0):
      return np.asarray(self._means, np.float64)
    return self._means.astype(np.float64) * p.outcome_sd[:, None] + p.outcome_mean[:, None]

  def set_joint(self, wsum: Dict[str, np.ndarray], path_ranks, window_names=None):
    """Takes the path arrays of the record's `windows` kind ({path_*: [B, 1 + W, 2, ...]}, window 0
    every series' post-period) and builds `joint_summary` and `window_joint_summary`."""
    self._joint = dict(psum={k: v for k, v in wsum.items() if k.startswith("path_")},
                       ranks=list(path_ranks), names=list(window_names) if window_names else None)
    num_draws = self._dsum["per_draw"].shape[-1]
    critical = lib._joint_critical(self._joint["psum"], path_ranks, num_draws, self.alpha)   # pylint: disable=protected-access
    rows = []                                                   # [series][window]: the two rows
    for b in range(len(self)):
      Tb, labels = self._series_view(b)[3], self._model_labels(b)
      psum = _cut({k: v[b] for k, v in self._joint["psum"].items()}, Tb, "windows")
      rows.append([lib._joint_rows(psum, w, critical[b], num_draws, self._prep.observed[b, :Tb],   # pylint: disable=protected-access
                                   lambda step, labels=labels: labels[step])
                   for w in range(critical.shape[1])])
    paths = list(lib.JOINT_PATHS)
    self.joint_summary = lib.joint_table_frame(
        [r for per in rows for r in per[0]],
        pd.MultiIndex.from_product([self._names, paths], names=["series", None]))
    if window_names:
      self.window_joint_summary = lib.joint_table_frame(
          [r for per in rows for two in per[1:] for r in two],
          pd.MultiIndex.from_product([self._names, list(window_names), paths], names=["series", "window", None]))

  def _joint_frames(self, b: int, ci_data, num_steps: int):
    """(joint_bands, joint_summary, window_joint_summary) of series b, or Nones."""
    if self._joint is None:
      return None, None, None
    psum = _cut({k: v[b] for k, v in self._joint["psum"].items()}, num_steps, "windows")
    rq = lib._device_summary_request(ci_data, self.alpha)       # pylint: disable=protected-access
    return lib._joint_frames(                                   # pylint: disable=protected-access
        psum, self._joint["ranks"], self._dsum["per_draw"].shape[-1], self.alpha, rq["observed"],
        lib.posterior_processing.model_index(ci_data), ci_data.data.index, self._joint["names"])

  def _window_slice(self, b: int) -> Optional[pd.DataFrame]:
    """The rows of series b of `window_summary`, indexed by (window, average|cumulative)."""
    if self.window_summary is None:
      return None
    per = len(self.window_summary) // len(self)
    return self.window_summary.iloc[b * per:(b + 1) * per].droplevel("series")

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

  def _build_summary(self) -> pd.DataFrame:
    """The reference's 15 summary columns (causalimpact_lib.py:934-1093) for every series at
    once: the same numpy reductions as `_summary_rows`, along axis 1 of [B, draws] arrays."""
    p = self._prep
    win = (p.flags & 2) != 0
    obs_w = p.observed[:, win]                                             # [B, T_w]
    post_mean = self._data_means()[:, win]
    n_obs = np.sum(~np.isnan(obs_w), axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
      obs_mean, obs_sum = np.nanmean(obs_w, axis=1), np.nansum(obs_w, axis=1)
    return summary_table(self._names, self.alpha, self._ranks, self._dsum, n_win=int(win.sum()),
                         n_obs=n_obs, obs_mean=obs_mean, obs_sum=obs_sum,
                         avg_pred=post_mean.mean(axis=1), cum_pred=post_mean.sum(axis=1))

  def _series_view(self, b: int):
    """(frame, pre_period, post_period, model steps) of series b."""
    p = self._prep
    return (pd.DataFrame(p.values[b], index=p.index, columns=self._columns), p.pre_period,
            p.post_period, len(p.model_rows))

  def _model_frame(self, b: int) -> pd.DataFrame:
    """(`outcome_link`) the frame of series b as its model read it."""
    p = self._prep.model
    return pd.DataFrame(p.values[b], index=p.index, columns=self._columns)

  def __getitem__(self, b: int) -> lib.CausalImpactAnalysis:
    b = range(len(self))[b]
    if b not in self._cache:
      # (arrays over time are padded to the longest series of a panel: series b owns [0, Tb))
      df, pre, post, Tb = self._series_view(b)
      # (`outcome_link`: ci_data of the model's copy; the effect's frames read the raw outcome and
      #  means that are on the data scale already)
      linked = bool(getattr(self._prep, "link", 0))
      ci_data = cid.CausalImpactData(self._model_frame(b) if linked else df, pre, post,
                                     standardize_data=self._prep.standardize_data)
      effect_data = lib._data_scale_view(ci_data, df) if linked else ci_data   # pylint: disable=protected-access
      dsum = _cut({k: v[b] for k, v in self._dsum.items()}, Tb, "effect")
      rq = lib._device_summary_request(effect_data, self.alpha)   # pylint: disable=protected-access
      series, summary = lib._compute_impact_device(            # pylint: disable=protected-access
          self._means[b, :Tb], dsum, rq["observed"], rq["flags"], self._ranks, effect_data, self.alpha)
      self._cache[b] = lib.CausalImpactAnalysis(series, summary, None, self.diagnostics_of(b),
                                                *self._component_frames(b, ci_data, Tb),
                                                *self._prediction_frames(b, ci_data, Tb),
                                                self._window_slice(b),
                                                *self._placebo_frames(b, ci_data, Tb, summary),
                                                *self._joint_frames(b, effect_data, Tb),
                                                *self._placebo_horizon_frames(b, ci_data, Tb, summary))
    return self._cache[b]

  def _placebo_horizon_frames(self, b: int, ci_data, num_steps: int, summary: pd.DataFrame):
    """(placebo_by_horizon, placebo_profile) of series b, or (None, None) without `Placebo(horizons=...)`."""
    pl = self._placebo
    if pl is None or pl.get("horizons") is None:
      return None, None
    return lib._placebo_horizon_frames(                         # pylint: disable=protected-access
        {k: v[b] for k, v in pl["summary"].items()}, pl["origins"][b], pl["horizons"][b], self.alpha,
        self._prep.observed[b, :num_steps], lib.posterior_processing.model_index(ci_data),
        int(pl["n_post"][b]), summary.loc["cumulative", "rel_effect"])

  @property
  def placebo_profile(self) -> Optional[pd.DataFrame]:
    """`CausalImpactAnalysis.placebo_profile` of every series as one table indexed by (series, horizon)
    (None without `Placebo(horizons=...)`): every series over the union of the horizons, NaN rows for
    the horizons a series lacks (a panel's series keeps the listed horizons <= its own H)."""
    pl = self._placebo
    if pl is None or pl.get("horizons") is None:
      return None
    if self._placebo_profile is None:
      rel = self.summary["rel_effect"].to_numpy()[1::2]          # (the cumulative rows)
      tables = []
      for b in range(len(self)):
        per = []
        if np.any(pl["origins"][b] >= 0):
          per = lib._placebo_horizon_columns(                   # pylint: disable=protected-access
              {k: v[b] for k, v in pl["summary"].items()}, pl["origins"][b], pl["horizons"][b], self.alpha,
              self._prep.observed[b, :self._series_view(b)[3]])
        rows = [lib._placebo_profile_row(cols, h, self.alpha, int(pl["n_post"][b]), rel[b]) for h, cols in per]   # pylint: disable=protected-access
        tables.append(pd.DataFrame(rows, index=pd.Index([h for h, _ in per], dtype=np.int64, name="horizon"),
                                   columns=list(lib.PLACEBO_PROFILE_COLUMNS)))
      self._placebo_profile = _stack_profiles(tables, self._names)
    return self._placebo_profile

  def _placebo_frames(self, b: int, ci_data, num_steps: int, summary: pd.DataFrame):
    """(placebo, placebo_quality) of series b, or (None, None) when they were not asked for."""
    if self._placebo is None:
      return None, None
    pl = self._placebo
    return lib._placebo_frames(                                 # pylint: disable=protected-access
        {k: v[b] for k, v in pl["summary"].items()}, pl["origins"][b], int(pl["horizon"][b]), self.alpha,
        self._prep.observed[b, :num_steps], lib.posterior_processing.model_index(ci_data),
        int(pl["n_post"][b]), summary.loc["cumulative", "rel_effect"])

  @property
  def placebo_quality(self) -> Optional[pd.DataFrame]:
    """One row per series with the entries of `CausalImpactAnalysis.placebo_quality` (None without
    `placebo=`): which cumulative bands of the batch to trust at the post-period's horizon.  A
    series of a panel whose pre-period has no room for an origin has n_origins 0 and NaN."""
    if self._placebo is None:
      return None
    if self._placebo_quality is None:
      pl, rows = self._placebo, []
      rel = self.summary["rel_effect"].to_numpy()[1::2]          # (the cumulative rows)
      for b in range(len(self)):
        H, cols = int(pl["horizon"][b]), None
        if np.any(pl["origins"][b] >= 0):
          cols = lib._placebo_columns(                          # pylint: disable=protected-access
              {k: v[b] for k, v in pl["summary"].items()}, pl["origins"][b], H, self.alpha,
              self._prep.observed[b, :self._series_view(b)[3]])
        rows.append(lib._placebo_quality(cols, H, self.alpha, int(pl["n_post"][b]), rel[b]))   # pylint: disable=protected-access
      self._placebo_quality = pd.DataFrame(rows, index=pd.Index(self._names, name="series"))
    return self._placebo_quality

  def _prediction_inputs(self, b: int, num_steps: int):
    """(summary, observed, conditioned) of series b over its `num_steps` steps."""
    p = getattr(self._prep, "model", None) or self._prep      # (`outcome_link`: the model's own outcome)
    psum = _cut({k: v[b] for k, v in self._psum.items()}, num_steps, "predictions")
    return psum, p.observed[b, :num_steps], ~p.mask[b, :num_steps]

  def _prediction_frames(self, b: int, ci_data, num_steps: int):
    """(prediction_errors, fit_quality) of series b, or (None, None) when they were not asked for."""
    if self._psum is None:
      return None, None
    psum, observed, conditioned = self._prediction_inputs(b, num_steps)
    return lib._prediction_frames(                              # pylint: disable=protected-access
        psum, self._ranks, self.alpha, observed, conditioned, self._state_dim,
        lib.posterior_processing.model_index(ci_data), ci_data.data.index)

  @property
  def fit_quality(self) -> Optional[pd.DataFrame]:
    """One row per series with the entries of `CausalImpactAnalysis.fit_quality` (None unless
    InferenceOptions.prediction_errors): which fits of the batch to trust."""
    if self._psum is None:
      return None
    if self._quality is None:
      rows = []
      for b in range(len(self)):
        psum, observed, conditioned = self._prediction_inputs(b, self._series_view(b)[3])
        cols = lib._prediction_columns(psum, self._ranks, self.alpha, observed, conditioned)   # pylint: disable=protected-access
        rows.append(lib._fit_quality(cols, psum["loglik"], self.alpha, observed, self._state_dim))   # pylint: disable=protected-access
      self._quality = pd.DataFrame(rows, index=pd.Index(self._names, name="series"))
    return self._quality

  def _component_frames(self, b: int, ci_data, num_steps: int):
    """(components, coefficients) of series b over its `num_steps` steps, or (None, None) when they
    were not asked for."""
    if self._csum is None:
      return None, None
    csum = _cut({k: v[b] for k, v in self._csum.items()}, num_steps, "components")
    return lib._component_frames(                               # pylint: disable=protected-access
        csum, self._ranks, self._dsum["per_draw"].shape[-1], self.alpha,
        lib.posterior_processing.model_index(ci_data), ci_data.data.index,
        list(ci_data.feature_ts.columns) if ci_data.feature_ts is not None else None)

  def __iter__(self):
    return (self[b] for b in range(len(self)))


def _stack_profiles(tables: Sequence[pd.DataFrame], names, level: str = "series") -> pd.DataFrame:
  """The per-series `placebo_profile` tables as one, indexed by (series, horizon): every series over
  the sorted union of the horizons, NaN rows where it lacks one.  level: the name of the first index
  level ("aggregate" for the pooled effects' profiles)."""
  horizons = pd.Index(sorted({int(h) for t in tables for h in t.index}), dtype=np.int64, name="horizon")
  columns = list(lib.PLACEBO_PROFILE_COLUMNS)
  values = [t.reindex(horizons)[columns].to_numpy(np.float64) for t in tables]
  index = pd.MultiIndex.from_product([list(names), horizons], names=[level, "horizon"])
  return pd.DataFrame(np.concatenate(values) if values else np.zeros((0, len(columns))), index=index, columns=columns)


class PerSeriesBatchAnalysis(CausalImpactBatchAnalysis):
  """The same container over analyses that were fitted one series at a time (the routes the
  one-launch path does not have: float64 compute, raw-scale outcomes)."""

  def __init__(self, names, alpha, analyses):   # pylint: disable=super-init-not-called
    self._names, self.alpha = list(names), alpha
    self._cache = dict(enumerate(analyses))
    self._diag_draws = None
    self.summary = pd.concat([a.summary for a in analyses], keys=self._names, names=["series", None])
    self.aggregates = None
    self.aggregate_summary = None
    self.window_summary = None
    self.aggregate_window_summary = None
    self._joint = None
    self.joint_summary = None
    self.window_joint_summary = None
    self.aggregate_joint_summary = None
    self.aggregate_window_joint_summary = None
    self.aggregate_placebo_quality = None
    self.aggregate_placebo_profile = None
    if all(a.joint_summary is not None for a in analyses):
      self.joint_summary = pd.concat([a.joint_summary for a in analyses], keys=self._names,
                                     names=["series", None])

  @property
  def fit_quality(self) -> Optional[pd.DataFrame]:
    if any(a.fit_quality is None for a in self._cache.values()):
      return None
    return pd.DataFrame([self._cache[b].fit_quality for b in range(len(self))],
                        index=pd.Index(self._names, name="series"))

  @property
  def placebo_quality(self) -> Optional[pd.DataFrame]:
    if any(a.placebo_quality is None for a in self._cache.values()):
      return None
    return pd.DataFrame([self._cache[b].placebo_quality for b in range(len(self))],
                        index=pd.Index(self._names, name="series"))

  @property
  def placebo_profile(self) -> Optional[pd.DataFrame]:
    if any(a.placebo_profile is None for a in self._cache.values()):
      return None
    return _stack_profiles([self._cache[b].placebo_profile for b in range(len(self))], self._names)

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
                    P: int, hmc_init: str, outcome_link: bool = False) -> str:
  """Where `fit_causalimpact_batch(sampler="hmc")` fits a batch: "one_launch" (all series x chains
  in one kernel launch per device and HBM budget) or "per_series" (`fit_causalimpact` on every
  series in turn, with the series' key: seasonal blocks, T > 4096, P > 128, hmc_init="vi", float64,
  standardize_data=False -- the refusals of the single-series path stay where they are; and
  outcome_link, which the one-launch session's summaries do not take)."""
  if (float64 or not standardize_data or num_seasonal_blocks > 0 or T > HMC_BATCH_MAX_T
      or P > HMC_BATCH_MAX_P or hmc_init != "gibbs" or outcome_link):
    return "per_series"
  return "one_launch"


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
  # `outcome_link` (`_under_link`): as in `PreparedBatch`; `raw` and `observed` are the RAW outcome's
  link: int = 0
  model: Optional["PreparedPanel"] = None


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

  def _build_summary(self) -> pd.DataFrame:
    p = self._prep
    stats = panel_window_stats(p.observed, p.flags, self._data_means(), p.lengths)
    return summary_table(self._names, self.alpha, self._ranks, self._dsum, **stats)

  def _series_view(self, b: int):
    p = self._prep
    return (pd.DataFrame(p.raw[b], index=p.indices[b], columns=self._columns), *p.periods[b],
            int(p.lengths[b]))

  def _model_frame(self, b: int) -> pd.DataFrame:
    p = self._prep.model
    return pd.DataFrame(p.raw[b], index=p.indices[b], columns=self._columns)

  def _model_labels(self, b: int) -> pd.Index:
    return self._prep.indices[b][self._prep.model_rows[b]]


# ------------------------------------------------------------------------------------------
# Aggregates: the pooled effect of groups of series of a batch
# ------------------------------------------------------------------------------------------
def aggregate_groups(aggregates, names: Sequence[Any]):
  """The group table of `fit_causalimpact_batch(aggregates=...)`: (aggregate names, (offsets,
  members, weights)), the groups in CSR form over the POSITIONS of the series in the batch
  (`_native.groups_csr`: members ascending, those of zero weight left out).

  aggregates: a mapping {aggregate name: members}; members are a sequence of series names (weight 1),
  a mapping {series name: weight}, or the string "all" (every series, weight 1).  ValueError for a
  series name the batch does not have, a member listed twice, a weight that is not finite and a
  group without a member of non-zero weight."""
  if not hasattr(aggregates, "items"):
    raise ValueError("`aggregates` must be a mapping {aggregate name: members}")
  if len(aggregates) == 0:
    raise ValueError("`aggregates` is empty")
  names = list(names)
  position = {}
  for b, name in enumerate(names):
    if name in position:
      raise ValueError(f"aggregates need unique series names: {name!r} names series {position[name]} and {b}")
    position[name] = b
  groups = []
  for agg, spec in aggregates.items():
    if isinstance(spec, str):
      if spec != "all":
        raise ValueError(f"aggregate {agg!r}: members are a sequence or a mapping of series names, or "
                         f"the string 'all'; got {spec!r}")
      items = [(name, 1.0) for name in names]
    elif hasattr(spec, "items"):
      items = list(spec.items())
    else:
      items = [(name, 1.0) for name in spec]
    group = {}
    for name, w in items:
      if name not in position:
        raise ValueError(f"aggregate {agg!r}: unknown series {name!r}")
      if position[name] in group:
        raise ValueError(f"aggregate {agg!r}: series {name!r} is listed twice")
      w = float(w)
      if not np.isfinite(w):
        raise ValueError(f"aggregate {agg!r}: the weight of series {name!r} is not finite")
      group[position[name]] = w
    if not any(w != 0.0 for w in group.values()):
      raise ValueError(f"aggregate {agg!r} is empty: it has no member of non-zero weight")
    groups.append(group)
  return list(aggregates.keys()), _native.groups_csr(groups, len(names))


def _check_aggregates(aggregates, names, shared_streams: bool, argument: str = "aggregates"):
  """`aggregate_groups` for the argument `aggregates` or `event_aggregates`, after the refusal of
  common random numbers."""
  if shared_streams:
    raise ValueError(
        f"`{argument}` cannot be combined with shared_streams=True: with common random numbers the "
        "Monte-Carlo errors of all series are perfectly correlated, and pairing draw n of every "
        "series is then not a draw from the joint posterior of independent series -- the pooled "
        "bands would be wrong.  Fit with the default per-series streams.")
  return aggregate_groups(aggregates, names)


def pool_weighted(rows: np.ndarray, csr, init: Optional[np.ndarray] = None) -> np.ndarray:
  """out[g] = init[g] + the sum over the members b of group g, ascending, of w[g, b] * rows[b], in
  float64 with one rounding per operation (NaN wherever a member is NaN): rows [B, ...] -> [G, ...].
  The accumulation of `csrc/ci_pool.h` for values already on the data scale: the pooled outcome, the
  pooled posterior mean, and the running sums of the routes that fit series by series."""
  offsets, members, weights = csr
  rows = np.asarray(rows, np.float64)
  G = len(offsets) - 1
  out = np.zeros((G,) + rows.shape[1:]) if init is None else np.array(init, np.float64)
  for g in range(G):
    for k in range(offsets[g], offsets[g + 1]):
      out[g] = out[g] + weights[k] * rows[members[k]]
  return out


class HostPool:
  """The running sums of csrc/ci_pool.h in numpy, for batches and panels that are fitted series by
  series: the series are added in order, `add(b, ...)` for b = 0, 1, ..., each from its fit's
  trajectories [N, T] (any float type) with value = trajectory * scale + shift in float64, two
  roundings, and pooled[g] = pooled[g] + w[g, b] * value for every group that has b, two roundings.
  Without `axes` (calendar time) `pooled` is [G, N, T] float64.  With the `EventAxis` of every group
  (event time) the window value[:, first_b : first_b + width_g] is added to pooled[g][:, :width_g];
  `pooled` is [G, N, stride] float64, stride the widest group, 0.0 beyond a group's width.  `means`:
  every series' posterior mean over its own steps on the data scale."""

  def __init__(self, csr, axes: Optional[Sequence[EventAxis]] = None):
    self.csr = csr
    self.axes = None if axes is None else list(axes)
    self.stride = None if axes is None else max(axis.width for axis in self.axes)
    self.pooled: Optional[np.ndarray] = None
    self.means: List[np.ndarray] = []

  def add(self, b: int, posterior_means, trajectories, scale, shift):
    offsets, members, weights = self.csr
    scale, shift = np.float64(scale), np.float64(shift)
    value = np.asarray(trajectories).astype(np.float64) * scale + shift
    self.means.append(np.asarray(posterior_means).astype(np.float64) * scale + shift)
    if self.pooled is None:
      self.pooled = np.zeros((len(offsets) - 1,) + value.shape[:-1] + (self.stride or value.shape[-1],))
    for g in range(len(offsets) - 1):
      k = offsets[g] + int(np.searchsorted(members[offsets[g]:offsets[g + 1]], b))
      if k < offsets[g + 1] and members[k] == b:
        f, W = 0, value.shape[-1]
        if self.axes is not None:
          f, W = int(self.axes[g].first[k - offsets[g]]), self.axes[g].width
        self.pooled[g, ..., :W] = self.pooled[g, ..., :W] + weights[k] * value[..., f:f + W]


class _PoolChain:
  """The running sums of a fit's aggregates over its launches: [G, N, T] for a batch (calendar time),
  [G, N, stride] with the `EventAxis` of every group for a panel (event time; `stride` the widest
  group).  The launches are chained in list order: launch k waits for the accumulator of launch
  k - 1, passes it on as `init` and hands its own result to launch k + 1.  The fits still run side by
  side; only these steps serialise.

  A batch lists its launches in ascending positions, so the sum runs over the series in order
  however the batch is cut into launches and devices.  A class of a panel holds whatever positions
  fall in it, so the launches do not cut the positions into consecutive runs; they are chained in the
  order `panel_launches` lists them -- class key ascending, ascending positions within a class, which
  its split over devices keeps -- and a session adds its members in ascending position.  A group is
  therefore summed in (class key, position) order: a function of the model and the series alone, the
  same on any number of devices, and not plain position order when its members fall in different
  classes.

  Every launch waits for an earlier one of the list and every device runs its launches in list order
  (`causalimpact_lib.map_by_device`), so no wait is circular.  Futures carry the accumulators: the
  exception of a launch reaches the launch that waits for it.  A launch that fails also fails every
  launch behind it in the chain that is not done: a device stops at its first failure, so the
  launches it had left never run, and whoever waits for one of them on another device must not wait
  for ever."""

  def __init__(self, launches, csr, axes: Optional[Sequence[EventAxis]] = None):
    self.csr = csr
    self.axes = None if axes is None else list(axes)
    self.stride = None if axes is None else max(axis.width for axis in self.axes)
    self._index = {int(launch[2][0]): k for k, launch in enumerate(launches)}
    self._futures = [concurrent.futures.Future() for _ in launches]

  def groups_of(self, ids: Sequence[int]):
    """The groups cut to the positions `ids` of one launch, whatever they are, as the session's pool
    method takes them: per group {place within the launch: weight}, or with axes ({place: (weight,
    first)}, width); the mapping is empty for a group without a member there."""
    offsets, members, weights = self.csr
    place = {int(b): i for i, b in enumerate(ids)}
    out = []
    for g in range(len(offsets) - 1):
      m, w = members[offsets[g]:offsets[g + 1]], weights[offsets[g]:offsets[g + 1]]
      if self.axes is None:
        out.append({place[int(b)]: float(x) for b, x in zip(m, w) if int(b) in place})
      else:
        out.append(({place[int(b)]: (float(x), int(f)) for b, x, f in zip(m, w, self.axes[g].first)
                     if int(b) in place}, self.axes[g].width))
    return out

  def session_pool(self, sess, scale, shift):
    """pool(groups, init) of the open session `sess` for `step`: its `pool_trajectories`, or with axes
    its `pool_event_trajectories` with out_stride = `stride` (first + width stays within every
    member's own length, hence within the stride of any kind of session)."""
    if self.axes is None:
      return lambda groups, init: sess.pool_trajectories(scale, shift, groups, init)
    return lambda groups, init: sess.pool_event_trajectories(scale, shift, groups, init, self.stride)

  def step(self, launch, pool):
    """The pool step of `launch`, its session still open: pool(groups, init) as `session_pool` makes
    it.  Only the groups with a member in the launch go to the device; the others pass their
    accumulator through untouched."""
    k = self._index[int(launch[2][0])]
    try:
      acc = self._futures[k - 1].result() if k else None
      groups = self.groups_of(launch[2])
      active = [g for g, group in enumerate(groups) if (group if self.axes is None else group[0])]
      if active:
        part = pool([groups[g] for g in active], None if acc is None else acc[active])
        if len(active) == len(groups):
          acc = part
        else:
          acc = np.zeros((len(groups),) + part.shape[1:]) if acc is None else acc.copy()
          acc[active] = part
      if self._futures[k].done():            # failed meanwhile by a launch in front that ended in an error
        self._futures[k].result()
      self._futures[k].set_result(acc)
    except BaseException as e:
      self.fail(launch, e)
      raise

  def fail(self, launch, error: BaseException):
    """A launch that ends in `error` before its pool step is done: whoever waits for it, or for a
    launch behind it (none of those can complete a sum that lacks this part), gets the error."""
    for future in self._futures[self._index[int(launch[2][0])]:]:
      try:
        future.set_exception(error)
      except concurrent.futures.InvalidStateError:     # done already
        pass

  def guarded(self, run):
    """`run(launch)` with its failure handed down the chain."""
    def call(launch):
      try:
        return run(launch)
      except BaseException as e:
        self.fail(launch, e)
        raise
    return call

  def result(self) -> np.ndarray:
    return self._futures[-1].result()


def scaler_stats(outcome_pre: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
  """(mean [B], sd [B]) of every series' pre-period outcome [B, n_pre] as `standardize.Scaler` fits
  them on that series alone (`CausalImpactData.outcome_scaler`): the statistics a series' own
  `series` frame puts its posterior mean on the data scale with.  (`standardize_batch` reduces the
  whole block along a strided axis and may differ from them in the last bit.)"""
  rows = [np.ascontiguousarray(r) for r in np.asarray(outcome_pre, np.float64)]
  with np.errstate(invalid="ignore"):
    return (np.array([np.nanmean(r, axis=0) for r in rows]),
            np.array([np.nanstd(r, axis=0, ddof=1) for r in rows]))


def _aggregate_paths(rows, alpha: float, device: int, windows):
  """The path arrays of every group's pooled draws in ONE device call (`_native.summarize_draw_paths`,
  ci_summarize_draw_paths_f64: scale 1, shift 0), as a record keeps them: ({path_*: [G, 1 + W, 2, ...]},
  the ranks of the excursions' order statistics, the number of draws).  rows, windows: those of
  `_frame_analyses`.  Window 0 of a group is its post-period (`lib.joint_windows` of its flags), then
  the effect windows in the order of their names, count 0 for one the group's axis does not cover.
  Groups of a panel have axes of their own: the draws are padded with 0.0, the observations with NaN,
  to the widest, and no window reaches the padding."""
  names = [] if windows is None else list(windows[0])
  G, N = len(rows), rows[0][5].shape[0]
  T = max(row[5].shape[1] for row in rows)
  draws, observed = np.zeros((G, N, T)), np.full((G, T), np.nan)
  first, count = np.zeros((G, 1 + len(names)), np.int32), np.zeros((G, 1 + len(names)), np.int32)
  for g, (_, _, obs, flags, _, pooled) in enumerate(rows):
    width = pooled.shape[1]
    draws[g, :, :width], observed[g, :width] = pooled, obs
    covered = {} if windows is None else {w.name: w for w in windows[1][g]}
    more = None
    if names:
      more = lib.Windows(np.array([covered[n].first if n in covered else 0 for n in names], np.int32),
                         np.array([covered[n].count if n in covered else 0 for n in names], np.int32))
    first[g], count[g] = lib.joint_windows(np.asarray(flags), more)
  path_ranks = lib._path_ranks(N, alpha)                        # pylint: disable=protected-access
  got = _native.summarize_draw_paths(draws, 1.0, 0.0, observed, first, count, path_ranks,
                                     want=lib._PATH_RECORD, device=device)   # pylint: disable=protected-access
  return lib._paths_record(got), path_ranks, N                  # pylint: disable=protected-access


def _frame_analyses(rows, alpha: float, ranks, device: int = 0, windows=None, joint_bands: bool = False):
  """(`aggregates`, `aggregate_summary`, `aggregate_window_summary`, `aggregate_joint_summary`,
  `aggregate_window_joint_summary`) from one row per group: (name, the `CausalImpactData` of the
  pooled outcome -- on the data scale already: standardize_data=False -- the pooled observed outcome
  and the window flags over the model steps, the pooled posterior mean, the pooled draws [N, steps]
  float64).  The order statistics and per-draw totals of the pooled draws come from
  `_native.summarize_draws` (ci_summarize_draws_f64: scale 1, shift 0), and the reference's frames are
  built by `_compute_impact_device`.  windows (`effect_windows`): (window names, per group the
  `lib.EffectWindow`s its axis covers); their totals come from `_native.window_totals_host` on the
  same pooled draws (scale 1, shift 0), and the table has NaN rows for a window a group does not
  cover.  The third result is None without them.  joint_bands: every group's `joint_bands`,
  `joint_summary` and `window_joint_summary` (`lib._joint_frames` on the arrays of `_aggregate_paths`,
  over the index of its `CausalImpactData`) and the last two results, the groups' tables stacked; None
  without it, the last also without windows."""
  analyses = {}
  paths = _aggregate_paths(rows, alpha, device, windows) if joint_bands else None
  for g, (name, ci_data, observed, flags, mean, draws) in enumerate(rows):
    dsum = _native.summarize_draws(draws, 1.0, 0.0, observed, flags, ranks, device=device)
    wins, totals = (() if windows is None else windows[1][g]), None
    if wins:
      totals = _native.window_totals_host(
          draws[None], 1.0, 0.0, observed, [w.first for w in wins], [w.count for w in wins])[0]
    series, summary, window_summary = lib._compute_impact_device(   # pylint: disable=protected-access
        mean, dsum, observed, flags, ranks, ci_data, alpha, windows=wins, window_totals=totals)
    joint = (None, None, None)
    if paths is not None:
      psum = _cut({k: v[g] for k, v in paths[0].items()}, draws.shape[1], "windows")
      joint = lib._joint_frames(                                # pylint: disable=protected-access
          psum, paths[1], paths[2], alpha, np.asarray(observed, np.float64),
          lib.posterior_processing.model_index(ci_data), ci_data.data.index,
          None if windows is None else list(windows[0]))
    analyses[name] = lib.CausalImpactAnalysis(series, summary, None, window_summary=window_summary,
                                              joint_bands=joint[0], joint_summary=joint[1],
                                              window_joint_summary=joint[2])
  table = pd.concat([a.summary for a in analyses.values()], keys=list(analyses),
                    names=["aggregate", None])
  window_table_ = None
  if windows is not None:
    full = pd.MultiIndex.from_product([list(windows[0]), ["average", "cumulative"]], names=["window", None])
    blank = pd.DataFrame(np.nan, index=full, columns=table.columns)
    window_table_ = pd.concat(
        [blank if a.window_summary is None else a.window_summary.reindex(full) for a in analyses.values()],
        keys=list(analyses), names=["aggregate", "window", None])
  joint_table, window_joint_table = None, None
  if paths is not None:
    joint_table = pd.concat([a.joint_summary for a in analyses.values()], keys=list(analyses),
                            names=["aggregate", None])
    if windows is not None:
      window_joint_table = pd.concat([a.window_joint_summary for a in analyses.values()],
                                     keys=list(analyses), names=["aggregate", "window", None])
  return analyses, table, window_table_, joint_table, window_joint_table


def _take_aggregates(res, got):
  """Hands the five results of `_frame_analyses` to the batch or panel result `res`."""
  (res.aggregates, res.aggregate_summary, res.aggregate_window_summary, res.aggregate_joint_summary,
   res.aggregate_window_joint_summary) = got


def _aggregate_analyses(agg_names, csr, pooled: np.ndarray, means: np.ndarray, prep: PreparedBatch,
                        outcome_name, alpha: float, ranks, device: int = 0,
                        windows: Optional[WindowPlan] = None, joint_bands: bool = False):
  """The results of `_frame_analyses` for a batch from the pooled draws [G, N, T] (float64, data
  scale) and the series' posterior means [B, T] on the data scale.  Per group: the observed outcome
  and the posterior mean are pooled with the same weights (`pool_weighted`; the outcome is NaN
  wherever a member is), the flags are the batch's, and the frames are built by `_frame_analyses` over
  a `CausalImpactData` of the pooled outcome."""
  outcome = pool_weighted(prep.values[:, :, 0], csr)            # [G, T_all]: the raw pooled outcome
  observed = pool_weighted(prep.observed, csr)                  # [G, T]: NaN in gap / tail
  mean = pool_weighted(means, csr)                              # [G, T]
  rows = []
  for g, name in enumerate(agg_names):
    try:
      ci_data = cid.CausalImpactData(pd.DataFrame({outcome_name: outcome[g]}, index=prep.index),
                                     prep.pre_period, prep.post_period, standardize_data=False)
    except ValueError as e:
      raise ValueError(f"aggregate {name!r}: {e}") from e
    rows.append((name, ci_data, observed[g], prep.flags, mean[g], pooled[g]))
  # (the groups share the batch's calendar, hence its windows)
  return _frame_analyses(rows, alpha, ranks, device,
                         None if windows is None else (windows.names, [windows.windows] * len(rows)),
                         joint_bands)


# ------------------------------------------------------------------------------------------
# Event-time aggregates: the pooled effect of groups of series of a panel
# ------------------------------------------------------------------------------------------
# The series of a panel have their own calendars; what they share is EVENT TIME, the number of rows
# since each one's own treatment start.  What differs from a batch is here: the axis of every group
# and the sums over shifted windows of the members' steps; `HostPool` and `_PoolChain` take the axes.
@dataclasses.dataclass
class EventAxis:
  """The event-time axis of one group: tau = -L .. H - 1, column c of the group is step
  first[k] + c of its k-th member (members as the group table lists them: ascending positions,
  those of zero weight left out)."""
  L: int              # steps before the treatment start that every member has
  gap: int            # the longest gap between a member's pre-period and its treatment start
  Hwin: int           # the shortest post-period window
  H: int              # steps from the treatment start on that every member has
  first: np.ndarray   # int32, per member: its step at column 0 (tau = -L)

  @property
  def width(self) -> int:
    return self.L + self.H

  @property
  def index(self) -> pd.Index:
    return pd.Index(np.arange(-self.L, self.H, dtype=np.int64), name="event_time")

  @property
  def flags(self) -> np.ndarray:
    """The window flags of the pooled series: bit 0 = tau >= 0, bit 1 = 0 <= tau < Hwin."""
    tau = np.arange(-self.L, self.H)
    return (tau >= 0).astype(np.uint8) | (((tau >= 0) & (tau < self.Hwin)).astype(np.uint8) << 1)


def event_axes(prep: PreparedPanel, csr) -> List[EventAxis]:
  """The event-time axis of every group of the table `csr` (`aggregate_groups`), from the prepared
  panel alone.  Series b of T_b model steps starts its treatment at e_b, its first step with bit 0
  of `flags` set (its pre-period plus gap_b = e_b - num_pre[b] steps), and has a window of win_b
  steps (bit 1), contiguous from e_b.  Over the members of a group (zero weights are not members):
  L = min e_b, gap = max gap_b, Hwin = min win_b, H = min (T_b - e_b); member b contributes its
  steps first_b .. first_b + L + H - 1 with first_b = e_b - L, all inside [0, T_b).  Event time
  counts the ROWS of a series, not calendar units."""
  offsets, members, _ = csr
  B = len(prep.lengths)
  start = np.zeros(B, np.int64)
  for b in range(B):
    after = np.flatnonzero(prep.flags[b, :prep.lengths[b]] & 1)
    if after.size == 0:
      raise ValueError(f"series at position {b} has no step from its treatment start on")
    start[b] = after[0]
  gaps = start - np.asarray(prep.num_pre, np.int64)
  windows = np.sum((prep.flags & 2) != 0, axis=1)
  tails = np.asarray(prep.lengths, np.int64) - start
  axes = []
  for g in range(len(offsets) - 1):
    m = np.asarray(members[offsets[g]:offsets[g + 1]], np.int64)
    L = int(start[m].min())
    axes.append(EventAxis(L=L, gap=int(gaps[m].max()), Hwin=int(windows[m].min()),
                          H=int(tails[m].min()), first=(start[m] - L).astype(np.int32)))
  return axes


def pool_event_weighted(rows: Sequence[np.ndarray], csr, axes: Sequence[EventAxis]) -> List[np.ndarray]:
  """`pool_weighted` over shifted windows: per group g the [width_g] sum over its members b,
  ascending, of w[g, b] * rows[b][first_b : first_b + width_g], in float64 with one rounding per
  operation (NaN wherever a member is NaN).  rows: per series an array over its model steps."""
  offsets, members, weights = csr
  out = []
  for g, axis in enumerate(axes):
    acc = np.zeros(axis.width)
    for k, f in zip(range(offsets[g], offsets[g + 1]), axis.first):
      acc = acc + weights[k] * np.asarray(rows[members[k]], np.float64)[f:f + axis.width]
    out.append(acc)
  return out


@dataclasses.dataclass
class EventPlan:
  """What `fit_causalimpact_panel(event_aggregates=...)` knows before any fit: the group table, the
  axes, and per group the pooled observed outcome [width] (NaN wherever a member is: gap, tail,
  missing value) and the `CausalImpactData` of the pooled raw outcome on its `event_time` index."""
  names: List[Any]
  csr: Tuple[np.ndarray, np.ndarray, np.ndarray]
  axes: List[EventAxis]
  observed: List[np.ndarray]
  data: List[cid.CausalImpactData]

  @property
  def stride(self) -> int:
    """The row length of the accumulators [G, N, stride]: the widest group."""
    return max(axis.width for axis in self.axes)


def event_plan(agg_names, csr, prep: PreparedPanel, outcome_name) -> EventPlan:
  """The `EventPlan` of a prepared panel.  ValueError, with the aggregate named, when the common
  axis of a group leaves fewer than 3 pre-period steps (L - gap), and for whatever else
  `CausalImpactData` refuses about the pooled outcome."""
  axes = event_axes(prep, csr)
  model_outcome = [prep.raw[b][prep.model_rows[b], 0] for b in range(len(prep.lengths))]
  outcome = pool_event_weighted(model_outcome, csr, axes)
  observed = pool_event_weighted([prep.observed[b, :Tb] for b, Tb in enumerate(prep.lengths)], csr, axes)
  data = []
  for name, axis, y in zip(agg_names, axes, outcome):
    num_pre = axis.L - axis.gap
    if num_pre < 3:
      raise ValueError(f"aggregate {name!r}: pre_period must span at least 3 time points on the event "
                       f"axis its members share. Got {max(num_pre, 0)}")
    try:
      # (integer periods are POSITIONS into the index: tau = -L .. -1 - gap and 0 .. Hwin - 1)
      data.append(cid.CausalImpactData(pd.DataFrame({outcome_name: y}, index=axis.index),
                                       (0, num_pre - 1), (axis.L, axis.L + axis.Hwin - 1),
                                       standardize_data=False))
    except ValueError as e:
      raise ValueError(f"aggregate {name!r}: {e}") from e
  return EventPlan(list(agg_names), csr, axes, observed, data)


def _event_aggregate_analyses(plan: EventPlan, pooled: np.ndarray, means: Sequence[np.ndarray],
                              alpha: float, ranks, device: int = 0,
                              windows: Optional[WindowPlan] = None, joint_bands: bool = False):
  """The results of `_frame_analyses` for a panel from the pooled draws [G, N, stride] (float64,
  data scale; group g owns its first width_g columns) and the series' posterior means over their own
  steps on the data scale.  Per group the posterior mean is pooled over the members' windows like the
  outcome (`pool_event_weighted`, the member order of the draws), the flags are the axis', and the
  frames are built by `_frame_analyses` on the group's `event_time` index."""
  mean = pool_event_weighted(means, plan.csr, plan.axes)
  wins = None
  if windows is not None:
    # on the group's own axis: tau is a value of its `event_time` index, step L + tau; a window the
    # axis' post-period (0 .. Hwin - 1) does not cover is left out (NaN rows)
    wins = (windows.names,
            [[lib.EffectWindow(name, lo, hi, axis.L + lo, hi - lo + 1)
              for name, (lo, hi) in zip(windows.names, windows.windows) if hi < axis.Hwin]
             for axis in plan.axes])
  return _frame_analyses(
      [(name, plan.data[g], plan.observed[g], axis.flags, mean[g], pooled[g][:, :axis.width])
       for g, (name, axis) in enumerate(zip(plan.names, plan.axes))], alpha, ranks, device, wins,
      joint_bands)


# ------------------------------------------------------------------------------------------
# Placebo forecasts of the pooled effects (`placebo=` with `aggregates=` / `event_aggregates=`)
# ------------------------------------------------------------------------------------------
@dataclasses.dataclass
class PlaceboPoolPlan:
  """What the pooled placebo forecasts of a fit's aggregates are taken over: the group table, per
  ENTRY of it the member's origins as its own model steps, and per group the same origins as
  positions on the group's own axis (`labels[g]`), its one horizon and the steps of its post-period.
  -1: an unused slot, at the end of a row; a group without room for an origin has a row of -1.
  horizons (`Placebo(horizons=...)`, else None): per group the horizons its forecasts are read at,
  ascending, the last used one its `horizon`; a group whose horizon is below 1 has a row of -1."""
  csr: Tuple[np.ndarray, np.ndarray, np.ndarray]
  origins: np.ndarray           # [K, O] int32
  columns: np.ndarray           # [G, O] int32
  horizon: np.ndarray           # [G] int32
  n_post: np.ndarray            # [G]
  labels: List[pd.Index]
  horizons: Optional[np.ndarray] = None   # [G, K] int32

  @property
  def shape(self) -> Tuple[int, ...]:
    """The slots of the pooled sums: [G, O], with horizons [G, O, K]."""
    return self.columns.shape if self.horizons is None else self.columns.shape + (self.horizons.shape[1],)

  def last_column(self, g: int) -> int:
    """The horizon slot of group g that holds its `horizon` (the last used one; 0 without any)."""
    return max(int(np.count_nonzero(self.horizons[g] >= 1)) - 1, 0)

  def entries_of(self, b: int):
    """[(group, entry)] of the series at position b, groups ascending; groups without an origin left out."""
    offsets, members, _ = self.csr
    out = []
    for g in range(len(offsets) - 1):
      k = offsets[g] + int(np.searchsorted(members[offsets[g]:offsets[g + 1]], b))
      if k < offsets[g + 1] and members[k] == b and np.any(self.columns[g] >= 0):
        out.append((g, int(k)))
    return out


def batch_placebo_pool_plan(csr, origins, horizon, n_post, labels: pd.Index,
                            placebo: Optional[lib.Placebo] = None) -> PlaceboPoolPlan:
  """The plan of a batch: every group has the origins [O] and the horizon every series of the batch
  has (they share `num_pre` and the post-period), on the batch's model index.  placebo (with
  `Placebo(horizons=...)`): every group takes `lib.placebo_horizon_list(placebo, horizon)`, strictly."""
  G, K = len(csr[0]) - 1, len(csr[1])
  origins = np.asarray(origins, np.int32).reshape(-1)
  return PlaceboPoolPlan(csr, np.tile(origins, (K, 1)), np.tile(origins, (G, 1)), np.full(G, int(horizon), np.int32),
                         np.full(G, int(n_post)), [labels] * G,
                         placebo_horizon_tables(placebo, np.full(G, int(horizon))))


def event_placebo_pool_plan(placebo: lib.Placebo, plan: EventPlan, state_dim: int) -> PlaceboPoolPlan:
  """The plan of a panel's event-time aggregates: group g has `lib.placebo_plan(placebo, L - gap,
  Hwin, state_dim)` on its `EventAxis` -- the pre-period and the window all its members share -- and
  member k forecasts from its own step first[k] + column, so every window lies inside every member's
  own pre-period.  The frames are indexed by `event_time` (column - L).  With `Placebo(horizons=...)`
  a group keeps the listed horizons <= its own H_g (lenient, as for a panel's series)."""
  offsets = plan.csr[0]
  plans = [lib.placebo_plan(placebo, axis.L - axis.gap, axis.Hwin, state_dim) for axis in plan.axes]
  width = max(1, max(len(o) for _, o in plans))
  columns = np.full((len(plans), width), -1, np.int32)
  origins = np.full((len(plan.csr[1]), width), -1, np.int32)
  for g, ((_, cols), axis) in enumerate(zip(plans, plan.axes)):
    columns[g, :len(cols)] = cols
    for k, first in zip(range(offsets[g], offsets[g + 1]), axis.first):
      origins[k, :len(cols)] = np.asarray(cols, np.int64) + int(first)
  horizon = np.array([h for h, _ in plans], np.int32)
  return PlaceboPoolPlan(plan.csr, origins, columns, horizon,
                         np.array([axis.Hwin for axis in plan.axes]), [axis.index for axis in plan.axes],
                         placebo_horizon_tables(placebo, horizon, strict=False))


def _placebo_pool_observed(pp: PlaceboPoolPlan, entry_seen) -> Dict[str, np.ndarray]:
  """{seen_sum, actual, n_counted: [G, O]} of the pooled sums: seen_sum and actual the weighted sums
  over a group's entries, ascending, of the members' (`lib._placebo_entry_seen`), n_counted the plain
  sum -- member-steps.  entry_seen(g, k) -> that dict of entry k, or None before it is known.  With
  `pp.horizons` every array is [G, O, K]: the same sums per horizon slot."""
  offsets, _, weights = pp.csr
  out = {k: np.zeros(pp.shape) for k in ("seen_sum", "actual", "n_counted")}
  for g in range(len(offsets) - 1):
    if not np.any(pp.columns[g] >= 0):
      continue
    for k in range(offsets[g], offsets[g + 1]):
      one = entry_seen(g, k)
      out["seen_sum"][g] = out["seen_sum"][g] + weights[k] * one["seen_sum"]
      out["actual"][g] = out["actual"][g] + weights[k] * one["actual"]
      out["n_counted"][g] = out["n_counted"][g] + one["n_counted"]
  return out


def _fit_placebo_observed(pp: PlaceboPoolPlan, fit: "_Fit") -> Dict[str, np.ndarray]:
  """`_placebo_pool_observed` of a one-launch fit, from the arrays its launches read: every member
  as its sampler saw it (float32), on the data scale with its own scaler's statistics; under the
  fit's outcome link the members' raw outcomes (`lib._placebo_entry_seen`)."""
  members = pp.csr[1]
  known: Dict[Any, Dict] = {}        # (a series of a batch has the same windows in every group)

  def entry_seen(g, k):
    b = int(members[k])
    hz = None if pp.horizons is None else pp.horizons[g]
    key = (b, int(pp.horizon[g]), pp.origins[k].tobytes(), None if hz is None else hz.tobytes())
    if key not in known:
      Tb = int(fit.lengths[b])
      one = lib.SeriesInputs(fit.y[b, :Tb], fit.mask[b, :Tb], None, None, (), False, {})
      known[key] = lib._placebo_entry_seen(one, fit.own_scale[b], fit.own_shift[b], fit.observed[b, :Tb],   # pylint: disable=protected-access
                                           pp.origins[k], int(pp.horizon[g]), fit.link, hz)
    return known[key]
  return _placebo_pool_observed(pp, entry_seen)


class SimulatedPool(NamedTuple):
  """`Placebo(simulate=True, pool=True)`: what the SIMULATED pooled placebo forecasts need beyond the
  plan -- the `_native.LINK_*` the totals are formed under and the (lower, upper) quantiles the frames
  report."""
  link: int
  quantiles: Tuple[float, float]

  def means(self, stats: Dict[str, np.ndarray], ranks, num_draws: int) -> Dict[str, np.ndarray]:
    """The summary the frames read (`lib._simulated_placebo_means`) from the statistics [G, O] of the
    pooled totals."""
    return lib._simulated_placebo_means(stats, ranks, num_draws, self.quantiles)   # pylint: disable=protected-access

  def finish_host(self, acc: np.ndarray, seen, counted) -> Dict[str, np.ndarray]:
    """`_native.finish_simulated_placebo_host` of the sums [G, O, N], as that summary."""
    num_draws = acc.shape[-1]
    ranks = lib._placebo_sim_ranks(num_draws, self.quantiles)   # pylint: disable=protected-access
    return self.means(_native.finish_simulated_placebo_host(acc, seen, counted, ranks), ranks, num_draws)


class HostPlaceboPool:
  """The running sums of the pooled placebo forecasts in numpy, for batches and panels that are fitted
  series by series: `add(b, forecast)` for b = 0, 1, ... with the `forecast(origins, horizon)` a fit
  hands to its `_placebo_sink`; every group that has b takes the terms of its own origins and horizon
  (`_native.pool_placebo_host`'s arithmetic, one entry at a time, entries ascending).  simulated (a
  `SimulatedPool`): the forecast hands the member's simulated totals (`lib._placebo_entry_simulated_host`)
  and the sums are those of `_native.pool_simulated_placebo_host`, [G, O, N].  With `pp.horizons` the
  forecast is asked for the group's horizon row as well and the sums are [G, O, K, 2, N]
  (`_native.pool_placebo_horizons_host`'s)."""

  def __init__(self, pp: PlaceboPoolPlan, simulated: Optional[SimulatedPool] = None):
    self.pp = pp
    self.simulated = simulated
    self.acc: Optional[np.ndarray] = None
    self._seen: Dict[int, Dict] = {}

  def add(self, b: int, forecast):
    pp = self.pp
    weights = pp.csr[2]
    for g, k in pp.entries_of(b):
      if pp.horizons is not None:
        one = forecast(pp.origins[k], int(pp.horizon[g]), pp.horizons[g])
      else:
        one = forecast(pp.origins[k], int(pp.horizon[g]))
      w = np.float64(weights[k])
      if pp.horizons is not None:
        if self.acc is None:
          self.acc = np.zeros(pp.shape + (2, one["s"].shape[-1]))
        self.acc[g, :, :, 0] = self.acc[g, :, :, 0] + w * one["s"]
        self.acc[g, :, :, 1] = self.acc[g, :, :, 1] + (w * w) * one["v"]
      elif self.simulated is not None:
        if self.acc is None:
          self.acc = np.zeros(pp.columns.shape + (one["totals"].shape[1],))
        self.acc[g] = self.acc[g] + w * one["totals"]
      else:
        if self.acc is None:
          self.acc = np.zeros(pp.columns.shape + (2, one["s"].shape[1]))
        self.acc[g, :, 0] = self.acc[g, :, 0] + w * one["s"]
        self.acc[g, :, 1] = self.acc[g, :, 1] + (w * w) * one["v"]
      self._seen[k] = {name: one[name] for name in ("seen_sum", "actual", "n_counted")}

  def result(self):
    """(means, observed): `_native.finish_placebo_host` of the sums (simulated: `SimulatedPool.finish_host`),
    and `_placebo_pool_observed`."""
    observed = _placebo_pool_observed(self.pp, lambda g, k: self._seen[k])
    if self.acc is None:                       # (no group has room for an origin)
      return None, observed
    if self.simulated is not None:
      return self.simulated.finish_host(self.acc, observed["seen_sum"], observed["n_counted"]), observed
    if self.pp.horizons is not None:
      return _native.finish_placebo_horizons_host(self.acc, observed["seen_sum"]), observed
    return _native.finish_placebo_host(self.acc, observed["seen_sum"]), observed


def _simulated_pool(placebo: Optional[lib.Placebo], link: int, alpha: float) -> Optional[SimulatedPool]:
  """The `SimulatedPool` of `Placebo(simulate=True, pool=True)` under the `_native.LINK_*` link, else
  None: the analytic pooled placebo."""
  if placebo is None or not placebo.pool:
    return None
  return SimulatedPool(int(link), (alpha / 2.0, 1.0 - alpha / 2.0))


def _new_placebo_chain(launches, pp: PlaceboPoolPlan, observed: Dict[str, np.ndarray], fit: "_Fit",
                       placebo: lib.Placebo, alpha: float) -> "_PlaceboChain":
  """The `_PlaceboChain` of a one-launch fit: analytic, or with `Placebo(pool=True)` simulated -- every
  series on the stream its fit runs on (`_launch_request`'s)."""
  sim = _simulated_pool(placebo, fit.link, alpha)
  on_device = bool(getattr(fit.inference_options, "summarize_on_device", True))
  if sim is None:
    return _PlaceboChain(launches, pp, observed["seen_sum"], on_device=on_device)
  num_chains = fit.inference_options.num_chains
  streams = lambda ids: [lib.placebo_stream(fit.seed, None if fit.shared_streams else int(b), range(num_chains))   # pylint: disable=unnecessary-lambda-assignment
                         for b in ids]
  return _PlaceboChain(launches, pp, observed["seen_sum"], sim, observed["n_counted"].astype(np.int32), streams,
                       on_device=on_device)


def placebo_pool_route(sess, has_slope: bool, num_seasons: Sequence[int], simulated: bool = False) -> str:
  """Where the pooled placebo forecasts of the open session `sess` are filtered: "one_lane"
  (`pool_placebo`: a trend with at most one block of 2 to 7 seasons), "blocks" (`pool_placebo_blocks`:
  any other block list whose state the block-model filter takes) or "host" (numpy, from the
  parameter draws: HMC and float64 sessions, a library without the entry, a wider state).  simulated:
  the same choice between `pool_simulated_placebo` and `pool_simulated_placebo_blocks`."""
  one_lane, blocks = (("pool_simulated_placebo", "pool_simulated_placebo_blocks") if simulated else
                      ("pool_placebo", "pool_placebo_blocks"))
  if "placebo" not in getattr(sess, "summaries", ()):
    return "host"
  if hasattr(sess, one_lane) and lib.device_predictions_supported(num_seasons):
    return "one_lane"
  if hasattr(sess, blocks) and lib.device_block_predictions_supported(has_slope, num_seasons):
    return "blocks"
  return "host"


class _PlaceboChain(_PoolChain):
  """The second chain of a fit with aggregates and `placebo=`: the accumulators [G, O, 2, N] of the
  pooled placebo forecasts (csrc/ci_placebo.h, ci_session_pool_placebo), handed from launch to launch
  in the order of the trajectories' sum -- list order: class key, then position -- so a group's sums
  do not depend on how the fit is cut into launches and devices, bit for bit.  The last launch hands
  the finished sums back with `seen`, the pooled observed sums, and gets the three means.
  simulated (a `SimulatedPool`; counted [G, O]: the member-steps every window counts, `streams(ids)`:
  the `lib.placebo_stream` of the positions `ids`): the same chain for the accumulators [G, O, N] of the
  SIMULATED pooled placebo forecasts (ci_session_pool_simulated_placebo) -- the same launch order, the
  same hand-on, the same choice of route; the last launch finishes with `seen`, `counted` and the
  ranks of `lib._placebo_sim_ranks`, and `means` is the summary `SimulatedPool.means` makes of it.
  With `pp.horizons` (`Placebo(horizons=...)`) the chain carries [G, O, K, 2, N] in the same order and
  with the same hand-on: a launch pools through ONE filter pass (`lib.pool_placebo_horizon_columns`:
  `Session.pool_placebo_horizons`, for a block model its `_blocks` entry, K calls where the library lacks
  it) and the last launch finishes the O * K slots; `seen` and `means` are [G, O, K]."""

  simulated: Optional[SimulatedPool] = None      # (the analytic chain, unless `__init__` says otherwise)
  pp: Optional[PlaceboPoolPlan] = None
  counted: Optional[np.ndarray] = None
  streams = None
  on_device = True

  def __init__(self, launches, pp: PlaceboPoolPlan, seen: np.ndarray, simulated: Optional[SimulatedPool] = None,
               counted: Optional[np.ndarray] = None, streams=None, on_device: bool = True):
    super().__init__(launches, pp.csr)
    self.pp, self.seen = pp, seen
    self.simulated, self.counted, self.streams = simulated, counted, streams
    self.on_device = on_device     # `InferenceOptions.summarize_on_device`: off, a session without entries filters in numpy
    self.means: Optional[Dict[str, np.ndarray]] = None

  def groups_of(self, ids: Sequence[int]):
    """Per group ({place within the launch: weight}, {place: origin row}) over the positions `ids`;
    both empty for a group without a member there or without an origin."""
    offsets, members, weights = self.csr
    place = {int(b): i for i, b in enumerate(ids)}
    out = []
    for g in range(len(offsets) - 1):
      here = [k for k in range(offsets[g], offsets[g + 1])
              if int(members[k]) in place and np.any(self.pp.columns[g] >= 0)]
      out.append(({place[int(members[k])]: float(weights[k]) for k in here},
                  {place[int(members[k])]: self.pp.origins[k] for k in here}))
    return out

  def session_pool(self, sess, scale, shift, series_inputs=None, observed=None, ids=None):
    """(pool, finish) of the open session `sess`: pool(groups, origins, horizon, init) -> acc of the
    groups handed in, finish(acc, seen) -> the three means.  `placebo_pool_route` chooses: a session
    whose model the one-lane filter takes runs both through `pool_placebo`, one whose model the
    block-model filter takes through `pool_placebo_blocks`; a session without the entries (HMC) through
    those of a `_native.DrawsSession` made from its parameter draws, which the pair then holds for
    `step` to close; any other (a state beyond 64, `summarize_on_device=False`) filters its members in
    numpy from the parameter draws (`lib._placebo_entry_host`) and pools with the host twin."""
    if self.simulated is not None:
      return self._simulated_session_pool(sess, scale, shift, series_inputs, ids)
    route = placebo_pool_route(sess, series_inputs[0].has_slope, series_inputs[0].num_seasons)
    draws, held = None, ()
    if route == "host":
      # a session without the entries (HMC): a session made from its parameter draws has them
      draws = sess.fetch(list(lib._PARAMETER_DRAWS))               # pylint: disable=protected-access
      drawn, blocks = lib._draws_session_beside(sess, series_inputs, draws, self.on_device)   # pylint: disable=protected-access
      if drawn is not None:
        sess, held, route = drawn, (drawn,), "blocks" if blocks else "one_lane"
    several = getattr(self.pp, "horizons", None) is not None
    if route != "host":
      T, B = int(sess.pb.T), int(sess.pb.num_series)
      entry = sess.pool_placebo if route == "one_lane" else sess.pool_placebo_blocks

      def pool(groups, origins, horizon, init):
        if several:                  # (`horizon`: the groups' horizon rows)
          return lib.pool_placebo_horizon_columns(sess, route == "blocks", scale, shift, groups, origins, horizon, init)
        return entry(scale, shift, groups, origins, horizon, init)["acc"]

      def finish(acc, seen):
        # no slot row is longer than the session's steps: as many slots at a time as it takes
        shape = seen.shape
        if several and lib.pool_placebo_horizons_available(route == "blocks"):
          # the entry itself with empty groups: no filter pass, the accumulators handed in and finished
          hz = self.pp.horizons
          rows = np.where((hz > 0).any(axis=1)[:, None], hz, np.array([1] + [-1] * (hz.shape[1] - 1), np.int32)[None, :])
          out = {k: np.zeros(shape) for k in _native.PLACEBO_OUTPUTS}
          room = max(1, (1 << 30) // max(acc[:, :1].nbytes, 1))     # (the accumulators a call may hold)
          for j in range(0, shape[1], min(T, room)):
            w = min(T, room, shape[1] - j)
            got = sess.pool_placebo_horizons(scale, shift, [{}] * shape[0], np.full((B, w), -1, np.int32), rows,
                                             np.ascontiguousarray(acc[:, j:j + w]), np.ascontiguousarray(seen[:, j:j + w]),
                                             blocks=route == "blocks")
            for k in out:
              out[k][:, j:j + w] = got[k]
          return out
        if several:                  # (a library without it: the O * K slots of a group, one after another)
          acc, seen = acc.reshape((shape[0], -1) + acc.shape[-2:]), seen.reshape(shape[0], -1)
        out = {k: np.zeros(seen.shape) for k in _native.PLACEBO_OUTPUTS}
        for j in range(0, acc.shape[1], T):
          w = min(T, acc.shape[1] - j)
          got = entry(scale, shift, [{}] * acc.shape[0], np.full((B, w), -1, np.int32),
                      np.ones(acc.shape[0], np.int32), np.ascontiguousarray(acc[:, j:j + w]),
                      np.ascontiguousarray(seen[:, j:j + w]))
          for k in out:
            out[k][:, j:j + w] = got[k]
        return {k: v.reshape(shape) for k, v in out.items()}
      return (pool, finish) + held

    def host_pool(groups, origins, horizon, init):
      csr = _native.groups_csr(groups, len(series_inputs))
      entries = [(g, int(m)) for g in range(len(groups)) for m in csr[1][csr[0][g]:csr[0][g + 1]]]
      if several:                    # (`horizon`: the groups' horizon rows)
        terms = [lib._placebo_entry_host(                           # pylint: disable=protected-access
            series_inputs[i], lib._pooled_draws(draws, i), scale[i], shift[i], observed[i],   # pylint: disable=protected-access
            origins[g][i], int(np.max(horizon[g])), horizon[g]) for g, i in entries]
        return _native.pool_placebo_horizons_host(np.stack([t["s"] for t in terms]), np.stack([t["v"] for t in terms]),
                                                  csr, init)
      terms = [lib._placebo_entry_host(                             # pylint: disable=protected-access
          series_inputs[i], lib._pooled_draws(draws, i), scale[i], shift[i], observed[i],   # pylint: disable=protected-access
          origins[g][i], int(horizon[g])) for g, i in entries]
      return _native.pool_placebo_host(np.stack([t["s"] for t in terms]), np.stack([t["v"] for t in terms]),
                                       csr, init)
    return host_pool, (_native.finish_placebo_horizons_host if several else _native.finish_placebo_host)

  def _simulated_session_pool(self, sess, scale, shift, series_inputs, ids):
    """`session_pool` of the simulated mode: (pool, finish) through `pool_simulated_placebo`
    (`.._blocks`) where `placebo_pool_route` finds the entry and the model, else in numpy from the
    session's parameter draws (`lib._placebo_simulated_host` on every member's own stream,
    `_native.pool_simulated_placebo_host`, `SimulatedPool.finish_host`).  ids: the launch's positions."""
    sim, counted = self.simulated, self.counted
    route = placebo_pool_route(sess, series_inputs[0].has_slope, series_inputs[0].num_seasons, simulated=True)
    draws, held = None, ()
    if route == "host":
      draws = sess.fetch(list(lib._PARAMETER_DRAWS))               # pylint: disable=protected-access
      drawn, blocks = lib._draws_session_beside(sess, series_inputs, draws, self.on_device)   # pylint: disable=protected-access
      if drawn is not None:
        sess, held, route = drawn, (drawn,), "blocks" if blocks else "one_lane"
    if route != "host":
      T, B = int(sess.pb.T), int(sess.pb.num_series)
      num_draws = int(sess.pb.num_chains * sess.pb.num_results)
      ranks = lib._placebo_sim_ranks(num_draws, sim.quantiles)    # pylint: disable=protected-access
      entry = sess.pool_simulated_placebo if route == "one_lane" else sess.pool_simulated_placebo_blocks

      def pool(groups, origins, horizon, init):
        return entry(scale, shift, groups, origins, horizon, sim.link, init)["acc"]

      def finish(acc, seen):
        # no slot row is longer than the session's steps: as many slots at a time as it takes
        G, R = acc.shape[0], len(ranks)
        out = dict(predicted_mean=np.zeros(seen.shape), spread_mean=np.zeros(seen.shape),
                   below=np.zeros(seen.shape), total_order=np.zeros((G, R, seen.shape[1])))
        for j in range(0, acc.shape[1], T):
          w = min(T, acc.shape[1] - j)
          got = entry(scale, shift, [{}] * G, np.full((B, w), -1, np.int32), np.ones(G, np.int32), sim.link,
                      np.ascontiguousarray(acc[:, j:j + w]), np.ascontiguousarray(seen[:, j:j + w]),
                      np.ascontiguousarray(counted[:, j:j + w]), ranks)
          for k in out:
            out[k][..., j:j + w] = got[k]
        return sim.means(out, ranks, num_draws)
      return (pool, finish) + held
    streams = self.streams(ids)

    def host_pool(groups, origins, horizon, init):
      csr = _native.groups_csr(groups, len(series_inputs))
      totals = [lib._placebo_simulated_host(                        # pylint: disable=protected-access
          *series_inputs[i].filter_inputs(), lib._pooled_draws(draws, i), scale[i], shift[i],   # pylint: disable=protected-access
          np.asarray(origins[g][i]).reshape(-1), int(horizon[g]), sim.link, streams[i])["totals"]
                for g in range(len(groups)) for i in (int(m) for m in csr[1][csr[0][g]:csr[0][g + 1]])]
      return _native.pool_simulated_placebo_host(np.stack(totals), csr, init)
    return host_pool, lambda acc, seen: sim.finish_host(acc, seen, counted)

  def step(self, launch, pool):            # pylint: disable=arguments-renamed
    """The step of `launch`, its session still open; pool: the pair of `session_pool`.  Only the
    groups with a member in the launch are added to; the last launch of the list finishes all."""
    pool, finish, *held = pool             # held: a draws session `session_pool` opened for the pair
    k = self._index[int(launch[2][0])]
    try:
      acc = self._futures[k - 1].result() if k else None
      groups = self.groups_of(launch[2])
      active = [g for g, (members, _) in enumerate(groups) if members]
      if active:
        used = self.pp.columns[active] >= 0
        width = max(1, int(used.sum(axis=1).max()))
        origins = [{i: row[:width] for i, row in groups[g][1].items()} for g in active]
        init = None if acc is None else np.ascontiguousarray(acc[active][:, :width])
        horizon = np.maximum(self.pp.horizon[active], 1) if self.pp.horizons is None else self.pp.horizons[active]
        part = pool([groups[g][0] for g in active], origins, horizon, init)
        if acc is None:
          acc = np.zeros(self.pp.columns.shape + part.shape[2:])
        else:
          acc = acc.copy()
        acc[active, :width] = part
      if k == len(self._futures) - 1 and acc is not None:
        self.means = finish(acc, self.seen)
      if self._futures[k].done():            # failed meanwhile by a launch in front that ended in an error
        self._futures[k].result()
      self._futures[k].set_result(acc)
    except BaseException as e:
      self.fail(launch, e)
      raise
    finally:
      for one in held:
        one.close()


def _take_aggregate_placebo(res, pp: PlaceboPoolPlan, names, means: Optional[Dict[str, np.ndarray]],
                            observed: Dict[str, np.ndarray], alpha: float):
  """Gives every `res.aggregates[name]` its `placebo` and `placebo_quality`
  (`lib._aggregate_placebo_frames`; fit_relative_effect: the aggregate's own cumulative `rel_effect`)
  and `res` its `aggregate_placebo_quality`, one row per aggregate.  means None: no group has room
  for an origin.  With `pp.horizons` means and observed are [G, O, K]: `placebo` and `placebo_quality`
  are read from each group's last used column (its H), every aggregate gains `placebo_by_horizon` and
  `placebo_profile` (`lib._aggregate_placebo_horizon_frames`) and `res` its `aggregate_placebo_profile`,
  indexed by (aggregate, horizon) with NaN rows where a group lacks a horizon."""
  rows, profiles = [], []
  for g, name in enumerate(names):
    one = res.aggregates[name]
    rel = one.summary.loc["cumulative", "rel_effect"]
    used = pp.columns[g] >= 0
    psum, actual = None, observed["actual"][g]
    if means is not None and np.any(used):
      seen = observed["seen_sum"][g]
      psum = dict({k: v[g] for k, v in means.items()}, n_counted=observed["n_counted"][g],
                  seen_sum=np.where(used if seen.ndim == 1 else used[:, None], seen, np.nan))
    if pp.horizons is not None:
      one.placebo_by_horizon, one.placebo_profile = lib._aggregate_placebo_horizon_frames(   # pylint: disable=protected-access
          psum, actual, pp.columns[g], pp.horizons[g], alpha, pp.labels[g], int(pp.n_post[g]), rel)
      profiles.append(one.placebo_profile)
      # the frames at H: the group's last used column
      last = pp.last_column(g)
      psum, actual = None if psum is None else {k: v[:, last] for k, v in psum.items()}, actual[:, last]
    one.placebo, one.placebo_quality = lib._aggregate_placebo_frames(   # pylint: disable=protected-access
        psum, actual, pp.columns[g], int(pp.horizon[g]), alpha, pp.labels[g], int(pp.n_post[g]), rel)
    rows.append(one.placebo_quality)
  res.aggregate_placebo_quality = pd.DataFrame(rows, index=pd.Index(list(names), name="aggregate"))
  if pp.horizons is not None:
    res.aggregate_placebo_profile = _stack_profiles(profiles, list(names), "aggregate")


# ------------------------------------------------------------------------------------------
# The one launch-and-assemble path of batches and panels
# ------------------------------------------------------------------------------------------
def _options(alpha, data_options, model_options, inference_options):
  """The options of a fit function with their defaults filled in, after its argument checks."""
  data_options = data_options or lib.DataOptions()
  model_options = model_options or lib.ModelOptions()
  inference_options = inference_options or lib.InferenceOptions()
  if not 0 < alpha < 1:
    raise ValueError("`alpha` must be between 0 and 1.")
  if inference_options.sampler not in ("gibbs", "hmc"):
    raise ValueError(f"sampler must be 'gibbs' or 'hmc', got {inference_options.sampler!r}")
  if inference_options.prediction_errors:     # (a state too wide for the filter: refused before any fit)
    lib.check_prediction_state(model_options.local_linear_trend, model_options.seasons)
  return data_options, model_options, inference_options


def _state_dim(model_options, inference_options) -> int:
  """The state dimension `fit_quality` scores from; 0 (unused, unchecked) without the option."""
  if not inference_options.prediction_errors:
    return 0
  return lib.check_prediction_state(model_options.local_linear_trend, model_options.seasons)


def _frames_outcome_first(data, data_options):
  """(`data` as a list of DataFrames, the columns of the first with the outcome in front)."""
  frames = [pd.DataFrame(d) for d in data]
  if not frames:
    raise ValueError("`data` is empty")
  first = frames[0]
  oc = data_options.outcome_column if data_options.outcome_column is not None else first.columns[0]
  return frames, [oc] + [c for c in first.columns if c != oc]


def _fit_per_series(frames, periods, names, outcome_column, alpha, seed, data_options, model_options,
                    inference_options, shared_streams, aggregates=None,
                    event_aggregates: Optional[EventPlan] = None,
                    windows: Optional[WindowPlan] = None, series_windows=None,
                    placebo=None, placebo_lenient: bool = False,
                    joint_bands: bool = False,
                    placebo_pool: Optional[PlaceboPoolPlan] = None,
                    outcome_link=None) -> PerSeriesBatchAnalysis:
  """`fit_causalimpact` on every series in turn: the routes the one-launch path does not have.
  float64 compute (csrc/ci_gibbs64.h) and raw-scale outcomes (their per-series internal
  conditioning, causalimpact_lib._internal_conditioning) exist on the single-series path, and so do
  the HMC fits that `hmc_batch_route` / `panel_route` send here.  Same container, same summary
  table, every series keyed like the one-launch path: series b on the Philox key of series id b
  (ci_series_stream_key), so the Monte-Carlo errors of different series are independent; with
  shared_streams=True every series equals `fit_causalimpact` on it alone with this seed.  B
  sequential fits on one device (see the docstrings of the fit functions).

  aggregates (batches only): (aggregate names, csr, prep) -- the group table of `aggregate_groups`
  and the `PreparedBatch` of the shared calendar.  The running sums of csrc/ci_pool.h are then
  accumulated in numpy, series by series in order, from every fit's data-scale trajectories in
  float64 (same order, same formula), before its draws are dropped.

  event_aggregates (panels only): the `EventPlan`.  The same in event time (`HostPool` with the
  axes): every series is a class of its own on this route, so (class key, position) order is position
  order.

  windows, series_windows (`effect_windows`): the `WindowPlan` and, per series, the `effect_windows`
  its own `fit_causalimpact` takes (a panel: the windows it covers, as positions into its index; None
  for a series that covers none).  `window_summary` stacks the fits' own tables, NaN rows for the
  windows a series does not cover.

  placebo: the `placebo=` every fit takes; placebo_lenient (panels): a series whose pre-period has
  no room for an origin gets an empty `placebo` frame and a NaN quality row instead of a ValueError.

  placebo_pool (`placebo` with aggregates): the `PlaceboPoolPlan`.  Every fit hands its
  `_placebo_sink` the per-draw terms of the origins and the horizon of every group it belongs to, and
  `HostPlaceboPool` adds them up in position order, as `HostPool` adds the trajectories.

  outcome_link: the `outcome_link=` every fit takes, on the RAW frames; a fit then hands its
  `_trajectory_sink` the linked draws and their mean, on the data scale already (scale 1, shift 0)."""
  opts = dataclasses.replace(data_options, outcome_column=outcome_column)
  base_seed = lib._sanitize_seed(seed)   # pylint: disable=protected-access
  analyses = []
  host_pool, extra = None, {}
  if aggregates is not None:
    agg_names, csr, prep = aggregates
    host_pool = HostPool(csr)
  elif event_aggregates is not None:
    host_pool = HostPool(event_aggregates.csr, event_aggregates.axes)
  host_placebo = None
  if placebo_pool is not None:
    host_placebo = HostPlaceboPool(placebo_pool, _simulated_pool(placebo, lib.resolve_outcome_link(outcome_link), alpha))
  for b, frame in enumerate(frames):
    seed_b = base_seed if shared_streams else _native.series_stream_key(base_seed, b)
    if host_pool is not None:
      extra = dict(_trajectory_sink=lambda *a, b=b: host_pool.add(b, *a))
    if placebo is not None:
      extra = dict(extra, placebo=placebo, _placebo_lenient=placebo_lenient)
    if host_placebo is not None:
      extra = dict(extra, _placebo_sink=lambda forecast, b=b: host_placebo.add(b, forecast))
    if joint_bands:
      extra = dict(extra, joint_bands=True)
    if outcome_link is not None:
      extra = dict(extra, outcome_link=outcome_link)
    one = lib.fit_causalimpact(frame, periods[b][0], periods[b][1], alpha=alpha, seed=seed_b,
                               data_options=opts, model_options=model_options,
                               inference_options=inference_options,
                               effect_windows=None if series_windows is None else series_windows[b],
                               **extra)
    analyses.append(dataclasses.replace(one, posterior_samples=None,   # (draws are not kept)
                                        window_summary=one.window_summary, placebo=one.placebo,
                                        placebo_quality=one.placebo_quality, joint_bands=one.joint_bands,
                                        joint_summary=one.joint_summary,
                                        window_joint_summary=one.window_joint_summary,
                                        placebo_by_horizon=one.placebo_by_horizon,
                                        placebo_profile=one.placebo_profile))
  res = PerSeriesBatchAnalysis(names, alpha, analyses)
  if windows is not None:
    full = pd.MultiIndex.from_product([windows.names, ["average", "cumulative"]], names=["window", None])
    blank = pd.DataFrame(np.nan, index=full, columns=analyses[0].summary.columns)
    for a in analyses:
      a.window_summary = blank if a.window_summary is None else a.window_summary.reindex(full)
    res.window_summary = pd.concat([a.window_summary for a in analyses], keys=list(names),
                                   names=["series", "window", None])
    if joint_bands:
      full = pd.MultiIndex.from_product([windows.names, list(lib.JOINT_PATHS)], names=["window", None])
      blank = lib.joint_table_frame([None] * len(full), full)
      for a in analyses:
        a.window_joint_summary = (blank if a.window_joint_summary is None
                                  else a.window_joint_summary.reindex(full))
      res.window_joint_summary = pd.concat([a.window_joint_summary for a in analyses], keys=list(names),
                                           names=["series", "window", None])
  if host_pool is not None:
    ranks = lib._summary_ranks(host_pool.pooled.shape[1], (alpha / 2.0, 1.0 - alpha / 2.0))   # pylint: disable=protected-access
    devs = list(inference_options.devices) if inference_options.devices else [0]
    if event_aggregates is not None:
      _take_aggregates(res, _event_aggregate_analyses(
          event_aggregates, host_pool.pooled, host_pool.means, alpha, ranks, devs[0], windows, joint_bands))
    else:
      _take_aggregates(res, _aggregate_analyses(
          agg_names, csr, host_pool.pooled, np.stack(host_pool.means), prep, outcome_column, alpha,
          ranks, devs[0], windows, joint_bands))
    if host_placebo is not None:
      _take_aggregate_placebo(res, placebo_pool, list(res.aggregates), *host_placebo.result(), alpha)
  return res


@dataclasses.dataclass
class _Fit:
  """What the launches of one fit read: the prepared arrays, series first and time padded to the
  longest series as in `PreparedPanel`, and the fit options."""
  y: np.ndarray                 # [B, T_max] standardised outcome as the sampler sees it
  mask: np.ndarray              # [B, T_max] bool
  design: Optional[np.ndarray]  # [B, T_max, P] or None
  lengths: np.ndarray           # [B] model steps of every series
  scale: np.ndarray             # [B] the outcomes' sd: value = trajectory * scale + shift
  shift: np.ndarray             # [B] the outcomes' mean
  observed: np.ndarray          # [B, T_max] data-scale outcome, NaN in gap / tail / padding
  flags: np.ndarray             # window flags: [T_max] when the series share them, else [B, T_max]
  params: List[Dict]            # per series: `_model.series_params`
  ranks: Sequence[int]          # the order statistics the summaries return
  seed: Tuple[int, int]
  shared_streams: bool
  model_options: lib.ModelOptions
  inference_options: lib.InferenceOptions
  # InferenceOptions.prediction_errors only: (sd [B], mean [B]) of every series' pre-period outcome
  # as its OWN scaler fits them (`scaler_stats`) -- the prediction summary is put on the data scale
  # with these, so that a series' frames equal its single fit's bit for bit (`scale` and `shift`
  # come from the vectorised pass and may differ from them in the last bit)
  own_scale: Optional[np.ndarray] = None
  own_shift: Optional[np.ndarray] = None
  # `effect_windows=` only: the resolved windows, every series' own first / count [B, W]
  windows: Optional[WindowPlan] = None
  # `placebo=` only: every series' origins [B, O] (model steps ascending, -1: unused, at the end)
  # and horizon [B] (`placebo_plans`); the summary is put on the data scale with own_scale / own_shift
  placebo_origins: Optional[np.ndarray] = None
  placebo_horizon: Optional[np.ndarray] = None
  # `Placebo(horizons=...)` only: every series' horizons [B, K] (`placebo_horizon_tables`)
  placebo_horizons: Optional[np.ndarray] = None
  # `Placebo(simulate=True)` only: the (lower, upper) quantiles of the simulated totals the frames report
  placebo_quantiles: Optional[Tuple[float, float]] = None
  # `joint_bands=True` only: every series' windows of `summarize_paths` [B, 1 + W] (`lib.joint_windows`:
  # window 0 its post-period) and the order statistics of the excursions
  paths: Optional[lib.Windows] = None
  path_ranks: Sequence[int] = ()
  # `outcome_link`: the `_native.LINK_*` of the effect summaries and the pooled sums (`observed` is then
  # the raw outcome, `scale` and `shift` the model's)
  link: int = 0


def _sampler_outcome(prep, data_options) -> np.ndarray:
  """prep.y as the sampler sees it: in DataOptions.dtype (data.py:121-128), priors included."""
  return prep.y.astype(cid._as_numpy_dtype(data_options.dtype)).astype(np.float64)  # pylint: disable=protected-access


def _new_fit(prep, y, lengths, pre_sd, alpha, seed, model_options, inference_options,
             shared_streams, windows: Optional[WindowPlan] = None, placebo=None,
             joint_bands: bool = False, placebo_simulate: bool = False, placebo_horizons=None) -> _Fit:
  """The `_Fit` of a prepared batch or panel: y = `_sampler_outcome(prep)`, lengths [B], pre_sd [B]
  the sd of every series' own pre-period outcome; placebo: (origins [B, O], horizon [B]) or None."""
  own_shift = own_scale = None
  if inference_options.prediction_errors or placebo is not None:
    src = prep.model if prep.link else prep          # (the outcome the model read)
    if isinstance(prep, PreparedPanel):
      stats = [scaler_stats(src.raw[b][prep.model_rows[b][:nb], 0][None])
               for b, nb in enumerate(prep.num_pre)]
      own_shift, own_scale = (np.array([st[i][0] for st in stats]) for i in (0, 1))
    else:
      own_shift, own_scale = scaler_stats(src.values[:, prep.model_rows[:prep.num_pre], 0])
  with np.errstate(invalid="ignore"):
    params = [_model.series_params(
        y[b, :Tb], prep.mask[b, :Tb], None if prep.design is None else prep.design[b, :Tb],
        prior_level_sd=model_options.prior_level_sd, num_seasonal_blocks=len(model_options.seasons),
        has_slope=model_options.local_linear_trend, outcome_sd=float(pre_sd[b]))
              for b, Tb in enumerate(int(t) for t in lengths)]
  num_draws = inference_options.num_chains * inference_options.num_results
  paths = None
  if joint_bands:
    flags = np.broadcast_to(prep.flags, prep.observed.shape)
    paths = lib.joint_windows(flags, None if windows is None else lib.Windows(windows.first, windows.count))
  return _Fit(y=y, mask=prep.mask, design=prep.design, lengths=np.asarray(lengths),
              scale=prep.outcome_sd, shift=prep.outcome_mean, observed=prep.observed,
              flags=prep.flags, params=params,
              ranks=lib._summary_ranks(num_draws, (alpha / 2.0, 1.0 - alpha / 2.0)),   # pylint: disable=protected-access
              seed=lib._sanitize_seed(seed), shared_streams=shared_streams,   # pylint: disable=protected-access
              model_options=model_options, inference_options=inference_options,
              own_scale=own_scale, own_shift=own_shift, windows=windows,
              placebo_origins=None if placebo is None else placebo[0],
              placebo_horizon=None if placebo is None else placebo[1],
              placebo_horizons=None if placebo is None else placebo_horizons,
              placebo_quantiles=(alpha / 2.0, 1.0 - alpha / 2.0) if placebo is not None and placebo_simulate else None,
              paths=paths,
              path_ranks=lib._path_ranks(num_draws, alpha) if joint_bands else (),   # pylint: disable=protected-access
              link=prep.link)


def placebo_plans(placebo: lib.Placebo, num_pre, num_post, state_dim: int):
  """(origins [B, O] int32 -- -1: unused, at the end of a row; O at least 1 --, horizon [B] int32) of
  B series from their pre- and post-period step counts: `lib.placebo_plan` of every series.  A
  series whose pre-period has no room for an origin has a row of -1."""
  plans = [lib.placebo_plan(placebo, int(a), int(b), state_dim) for a, b in zip(num_pre, num_post)]
  width = max(1, max(len(o) for _, o in plans))
  origins = np.full((len(plans), width), -1, np.int32)
  for b, (_, o) in enumerate(plans):
    origins[b, :len(o)] = o
  return origins, np.array([h for h, _ in plans], np.int32)


def placebo_horizon_tables(placebo: Optional[lib.Placebo], horizon, strict: bool = True) -> Optional[np.ndarray]:
  """horizons [B, K] int32 (-1: unused, at the end of a row) of B series from their plans' horizons
  [B] -- `lib.placebo_horizon_list` of every series -- or None without `Placebo(horizons=...)`.  strict
  (batches): a listed horizon beyond a series' H is a ValueError; off (panels): the series keeps the
  listed horizons <= its own H.  A series whose H is below 1 has a row of -1."""
  if placebo is None or placebo.horizons is None:
    return None
  rows = [lib.placebo_horizon_list(placebo, int(h), strict) for h in horizon]
  table = np.full((len(rows), max(1, max(0 if r is None else len(r) for r in rows))), -1, np.int32)
  for b, r in enumerate(rows):
    if r is not None:
      table[b, :len(r)] = r
  return table


def _run_launch(launch, kind: str, fit: _Fit, chain: Optional[_PoolChain] = None,
                placebo_chain: Optional[_PlaceboChain] = None):
  """One launch of the Gibbs sampler and its summaries on the device.  launch: (device, key,
  positions) as `panel_launches` lists them; kind: the session the positions run in --
    "ordinary"         `_native.Session`: series b of the launch is keyed by positions[0] + b, hence
                       runs of consecutive positions (or shared streams), all of one length;
    "ragged"           `_native.Session.ragged`: every series on its own length and keyed by its
                       position (`series_ids`), the stride the longest series of the launch;
    "ragged_seasonal"  the same with the table of positional change flags of the launch (every
                       series starts at its own step 0) and the stride rounded up to a multiple of 4
                       (every row 16-byte aligned), the padding as in `PreparedPanel`: y NaN, mask
                       True, design 0, observed NaN, flags 0.
  Returns (out, record): `fetch` of posterior_means [n, C, T] and `_DRAW_SCALARS` [n, C, S], and the
  `lib.SummaryRecord` of `_launch_request` (`lib.take_summaries`).  Every array keeps the series axis,
  and T is the longest series of the launch on every route.
  chain (aggregates of a batch, event-time aggregates of a panel): the launch's pool step runs after
  the summaries, the session still open; placebo_chain (the same with `placebo=`): the step of the
  pooled placebo forecasts after it."""
  dev, _, ids = launch
  ids = np.asarray(ids, dtype=np.int64)
  mo, io = fit.model_options, fit.inference_options
  T = int(fit.lengths[ids].max())
  stride = (T + 3) & ~3 if kind == "ragged_seasonal" else T

  def rows(a, fill):
    a = a[ids, :T]
    if stride == T:
      return a
    return np.concatenate([a, np.full((len(ids), stride - T) + a.shape[2:], fill, a.dtype)], axis=1)

  y, mask = rows(fit.y, np.nan), rows(fit.mask, True)
  design = None if fit.design is None else rows(fit.design, 0.0)
  observed = rows(fit.observed, np.nan)
  flags = fit.flags[:T] if fit.flags.ndim == 1 else rows(fit.flags, 0)
  scale, shift = fit.scale[ids], fit.shift[ids]
  num_seasons, season_change = _model.expand_seasons(mo.seasons, stride)
  problem = dict(T=stride, P=0 if design is None else design.shape[2], has_slope=mo.local_linear_trend,
                 num_seasons=num_seasons, num_warmup=io.num_warmup_steps, num_results=io.num_results,
                 num_chains=io.num_chains, num_series=len(ids), seed=fit.seed, device=dev,
                 flags=int(getattr(io, "kernel_flags", 0)) |
                 (_native.FLAG_SHARED_SERIES_STREAMS if fit.shared_streams else 0))
  par = _native.make_params([fit.params[b] for b in ids])
  if kind == "ordinary":
    sess = _native.Session(_native.make_problem(series_offset=int(ids[0]), **problem), y, mask,
                           design, season_change, par)
  else:
    sess = _native.Session.ragged(
        _native.make_problem(**problem), fit.lengths[ids], y, mask, design, par, series_ids=ids,
        season_change=season_change if kind == "ragged_seasonal" else None)
  try:
    sess.run()
    out = sess.fetch(["posterior_means", *_DRAW_SCALARS])
    inputs = _series_inputs(fit, ids, season_change, num_seasons)
    record = lib.take_summaries(sess, _launch_request(fit, ids, observed, flags), inputs)
    if chain is not None:
      # (`outcome_link`: the session keeps the link `take_summaries` set -- the pool adds linked values)
      chain.step(launch, chain.session_pool(sess, scale, shift))
    if placebo_chain is not None:
      placebo_chain.step(launch, placebo_chain.session_pool(
          sess, fit.own_scale[ids], fit.own_shift[ids], inputs,
          [fit.observed[b, :int(fit.lengths[b])] for b in ids], ids))
  finally:
    sess.close()
  if stride != T:            # (back at the stride of the longest series)
    out, record = _cut(out, T, "fetched"), record.map(lambda kind, arrays: _cut(arrays, T, kind))
  return out, record


def _launch_request(fit: _Fit, ids, observed, flags) -> lib.SummaryRequest:
  """What the fit wants of the launch of the series `ids`; observed, flags: theirs at its stride."""
  io, own = fit.inference_options, None
  if fit.own_scale is not None:
    own = lib.Affine(fit.own_scale[ids], fit.own_shift[ids])
  simulated = {}
  if fit.placebo_quantiles is not None:
    # (every series on the key its fit runs on, the chains of a launch being all of its chains)
    simulated = dict(quantiles=fit.placebo_quantiles, link=fit.link, streams=[
        lib.placebo_stream(fit.seed, None if fit.shared_streams else int(b), range(io.num_chains)) for b in ids])
  return lib.SummaryRequest(
      scale=fit.scale[ids], shift=fit.shift[ids], observed=observed, flags=flags, ranks=fit.ranks,
      components=io.components, predictions=own if io.prediction_errors else None,
      windows=None if fit.windows is None else lib.Windows(fit.windows.first[ids], fit.windows.count[ids]),
      placebo=None if fit.placebo_origins is None else lib.PlaceboPart(
          *own, fit.placebo_origins[ids], fit.placebo_horizon[ids], **simulated,
          horizons=None if fit.placebo_horizons is None else fit.placebo_horizons[ids]),
      paths=None if fit.paths is None else lib.Windows(fit.paths.first[ids], fit.paths.count[ids]),
      path_ranks=fit.path_ranks, link=fit.link, on_device=bool(getattr(io, "summarize_on_device", True)))


def _series_inputs(fit: _Fit, ids, season_change, num_seasons) -> Optional[List[lib.SeriesInputs]]:
  """The series `ids` as their sampler saw them, each over its own steps, for the summaries taken in
  numpy (None when the fit asks for none of them)."""
  if fit.own_scale is None:
    return None
  season_change = np.asarray(season_change)
  return [lib.SeriesInputs(fit.y[b, :Tb], fit.mask[b, :Tb], None if fit.design is None else fit.design[b, :Tb],
                           season_change[:, :Tb], num_seasons, fit.model_options.local_linear_trend,
                           fit.params[b]) for b, Tb in ((int(b), int(fit.lengths[b])) for b in ids)]


def _run_hmc_launch(launch, fit: _Fit, chain: Optional[_PoolChain] = None,
                    placebo_chain: Optional[_PlaceboChain] = None):
  """`_run_launch` for the one-launch HMC path (`_hmc.fit_hmc_batch`: B x chains HMC chains, then
  the latent paths and the predictive trajectories on the device): consecutive positions of a batch,
  series b keyed by positions[0] + b.  Its session (`_native.BatchLogLikSession`) has the effect
  summary and the window totals; it keeps no latent draws, hence no component summary, and prediction
  errors and placebo forecasts are filtered from its parameter draws: by one `_native.DrawsSession`
  over the launch's series (`lib.take_summaries`, `_PlaceboChain.session_pool`), in numpy with
  `InferenceOptions(summarize_on_device=False)`."""
  from causalimpact import _hmc  # pylint: disable=import-outside-toplevel
  dev, _, ids = launch
  ids = np.asarray(ids, dtype=np.int64)
  mo, io = fit.model_options, fit.inference_options

  def resident(sess):            # (the session still open: the summaries, then the pool step)
    inputs = _series_inputs(fit, ids, np.zeros((0, fit.y.shape[1]), np.uint8), ())
    record = lib.take_summaries(sess, _launch_request(fit, ids, fit.observed[ids], fit.flags), inputs)
    if chain is not None:
      chain.step(launch, chain.session_pool(sess, fit.scale[ids], fit.shift[ids]))
    if placebo_chain is not None:          # (no filter on this session: a session made from its parameter draws)
      placebo_chain.step(launch, placebo_chain.session_pool(
          sess, fit.own_scale[ids], fit.own_shift[ids], inputs, list(fit.observed[ids]), ids))
    return record

  res = _hmc.fit_hmc_batch(
      fit.y[ids], fit.mask[ids], None if fit.design is None else fit.design[ids],
      [fit.params[b] for b in ids], has_slope=mo.local_linear_trend, num_results=io.num_results,
      num_warmup=io.num_warmup_steps, num_chains=io.num_chains, seed=fit.seed, device=dev,
      series_offset=int(ids[0]), shared_streams=fit.shared_streams, prior=io.hmc_prior,
      resident=resident)
  return {k: res[k] for k in ("posterior_means", *_DRAW_SCALARS)}, res["resident"]


def _scatter(parts, num_series: int, num_steps: int, kind: str) -> Dict[str, np.ndarray]:
  """{name: [num_series, ...]} of parts = [(positions, {name: [len(positions), ...]})], arrays of
  `kind`: those over time (last axis) are padded from a launch's stride to `num_steps` with the
  kind's fill."""
  whole, fill = _KINDS[kind].whole + _KINDS[kind].also, _KINDS[kind].fill
  out = {k: (np.zeros((num_series,) + v.shape[1:], v.dtype) if k in whole else
             np.full((num_series,) + v.shape[1:-1] + (num_steps,), fill, v.dtype))
         for k, v in parts[0][1].items()}
  for ids, arrays in parts:
    for k, v in arrays.items():
      if k in whole:
        out[k][ids] = v
      else:
        out[k][ids, ..., :v.shape[-1]] = v
  return out


def _assemble(launches, run, num_series: int, num_steps: int):
  """Runs `launches` [(device, key, positions)] through `run(launch) -> (out, record)`
  (`_run_launch`; the launches of a device in turn, the devices side by side) and puts the series
  axis back together.  Returns what the containers take:
    means [B, T_max]  the chain mean of posterior_means, 0 beyond a series' length (under
                      `outcome_link` the record's value_mean: data scale, NaN beyond it);
    record            the `lib.SummaryRecord` {name: [B, ...]} per kind (None: a kind the launches
                      did not take); arrays over time are NaN beyond a series' length;
    diag_draws        {name: [B, C, S]} of `_DRAW_SCALARS`, or None for one chain.
  One launch that holds all B series in order at full stride is the result as it stands: its blocks
  (512 series: 24 MB of summary in pinned memory) are not copied a second time."""
  results = lib.map_by_device(run, launches)
  # per launch: the chain mean with the scalar draws
  fetched = [dict({k: out[k] for k in _DRAW_SCALARS}, means=out["posterior_means"].mean(axis=1))
             for out, _ in results]
  if (len(launches) == 1 and list(launches[0][2]) == list(range(num_series))
      and fetched[0]["means"].shape[-1] == num_steps):
    fetched, record = fetched[0], results[0][1]
  else:
    def gather(kind, per_launch):
      return _scatter([(list(launch[2]), arrays) for launch, arrays in zip(launches, per_launch)],
                      num_series, num_steps, kind)
    fetched = gather("fetched", fetched)
    record = results[0][1].map(lambda kind, _: gather(kind, [getattr(rec, kind) for _, rec in results]))
  means = fetched.pop("means")
  if "value_mean" in record.effect:     # (`outcome_link`: the means of the linked draws, on the data scale)
    means = record.effect["value_mean"]
  diag_draws = fetched if fetched[_DRAW_SCALARS[0]].shape[1] > 1 else None
  return means, record, diag_draws


def fit_causalimpact_batch(data: Union[Sequence[pd.DataFrame], np.ndarray],
                           pre_period, post_period, alpha: float = 0.05, seed=None,
                           data_options: Optional[lib.DataOptions] = None,
                           model_options: Optional[lib.ModelOptions] = None,
                           inference_options: Optional[lib.InferenceOptions] = None,
                           index: Optional[pd.Index] = None,
                           names: Optional[Sequence[Any]] = None,
                           shared_streams: bool = False,
                           aggregates=None, effect_windows=None,
                           placebo=None, joint_bands: bool = False,
                           outcome_link=None) -> CausalImpactBatchAnalysis:
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

  aggregates: the POOLED effect of groups of series -- the total over all geos, per region -- with
  its credible bands.  A mapping {aggregate name: members}; members are a sequence of series names
  (entries of `names`; weight 1), a mapping {series name: weight}, or the string "all".  The effect
  of a group is that of its pooled outcome y_g = sum_b w_b y_b: interval ends do not add (a sum of
  2.5 % quantiles is not the 2.5 % quantile of the sum), so the members' predictive trajectories are
  added draw by draw -- draw n of the group is sum_b w_b * (draw n of series b on the data scale),
  over b ascending in float64 -- on the device that holds them (csrc/ci_pool.h; the [B, draws, T]
  trajectories are never downloaded), and the [draws, T] sums are summarised like a single series'.
  The sum is handed from launch to launch in series order, so the result does not depend on how the
  batch is cut into launches and devices, bit for bit.  Series are independent given their own
  data, and so are their default random streams: draw n of every series pairs up to a draw of the
  joint posterior.  `shared_streams=True` is refused with aggregates: common random numbers make the
  Monte-Carlo errors of all series move together.  The result then has `aggregates` ({name:
  CausalImpactAnalysis} with the reference's `series` and `summary` frames of the pooled outcome;
  `plot` takes it as any other; no `posterior_samples`) and `aggregate_summary` (the 15 summary
  columns indexed by (aggregate, average|cumulative)); both are None without the argument, and
  nothing else changes with it.  The pooled outcome is NaN wherever a member's is.  ValueError for an
  unknown series name, a member listed twice, a weight that is not finite or a group without a
  member of non-zero weight.  Batches fitted series by series (float64, raw scale, most HMC) add up
  the same sum in numpy from every fit's trajectories.

  effect_windows: {name: (start, end)}, sub-windows of the post-period as labels on the shared index
  (both ends inclusive, read as `post_period` is): how the effect unfolds.  The result then has
  `window_summary`, the 15 summary columns indexed by (series, window, average|cumulative) --
  `result[b].window_summary` is the slice of series b -- from every draw's totals over every window,
  summed where the trajectories lie (csrc/ci_windows.h: one pass over the windows' own columns, no
  draws downloaded; `_native.window_totals_host` on the routes fitted series by series), and with
  `aggregates` also `aggregate_window_summary` (aggregate, window, average|cumulative) from the
  pooled draws.  ValueError before any fit, naming the window, for one that leaves the post-period or
  holds no row.  None: both attributes are None and nothing runs.

  placebo: None (the default: nothing runs, no result differs), True or a `lib.Placebo` -- the
  fixed-parameter placebo check of `fit_causalimpact` for every series: `result[b].placebo`,
  `result[b].placebo_quality`, and `result.placebo_quality` as one table with a row per series, the
  companion of `fit_quality` at the horizon of the post-period.  Forecast on the device that holds
  the draws (csrc/ci_placebo.h) inside every launch; in numpy on the routes `prediction_errors`
  takes in numpy.  ValueError before any fit when the pre-period has no room for an origin.  With
  `aggregates` every pooled group gets the same check -- it is where it matters most: a pooled band adds
  the members' predictive variances as if no shock were common to them, and only a placebo on the
  pooled sum can show that it is too narrow.  `result.aggregates[name]` then has `placebo` (the
  `PLACEBO_COLUMNS` on the batch's index: the origins and the horizon every series has) and
  `placebo_quality`, and `result.aggregate_placebo_quality` has one row per aggregate.  The members'
  forecasts are added draw by draw with the group's weights, their variances with the squared weights,
  where the draws lie (csrc/ci_placebo.h, ci_session_pool_placebo; for any other block list up to 64
  state components csrc/ci_placebo_blocks.h, ci_session_pool_placebo_blocks), chained from launch to
  launch like the trajectories' sums; in numpy (`_native.pool_placebo_host`) on the routes that filter there.
  Given every member's draw the pooled sum is normal with these two moments IF the members are
  independent of each other: the assumption the check tests.  `actual` and `n_counted` are the
  weighted sum and the plain sum (member-steps) of the members'.

  `Placebo(horizons=...)` (see `lib.Placebo`): every `result[b]` gains `placebo_by_horizon` and
  `placebo_profile`, and `result.placebo_profile` is one table indexed by (series, horizon) -- one
  filter pass of the launch for all horizons (ci_session_summarize_placebo_horizons).  ValueError before
  any fit for a listed horizon beyond H.  With `aggregates` every `result.aggregates[name]` gains the same
  two frames for the pooled effect (`placebo_by_horizon` indexed by (origin, horizon), `placebo_profile`
  with empirical_p on the row h == n_post against the aggregate's own cumulative rel_effect) and
  `result.aggregate_placebo_profile` is one table indexed by (aggregate, horizon) -- one filter pass per
  launch for every horizon of every group (ci_session_pool_placebo_horizons, `_blocks` for the block
  models), the pooled `placebo` at H read from its last column.

  joint_bands: False (the default: nothing runs, no result differs) or True -- the simultaneous bands
  and the whole-path test of `fit_causalimpact` for every series: `result[b].joint_bands`,
  `result[b].joint_summary`, `result.joint_summary` as one table indexed by (series,
  pointwise|cumulative) and, with `effect_windows`, `window_joint_summary` indexed by (series, window,
  pointwise|cumulative).  Every draw's largest standardised excursion is taken where the trajectories
  lie (csrc/ci_paths.h; no draws downloaded), in numpy on the routes fitted series by series.  With
  `aggregates` every pooled group gets the same: `result.aggregates[name]` has `joint_bands`,
  `joint_summary` and `window_joint_summary` over the batch's calendar, `result.aggregate_joint_summary`
  is indexed by (aggregate, pointwise|cumulative) and, with `effect_windows`,
  `result.aggregate_window_joint_summary` by (aggregate, window, pointwise|cumulative) -- one device call
  on the pooled float64 draws of all groups (ci_summarize_draw_paths_f64), on every route.

  outcome_link: None (the default: nothing runs, no result differs), "log" or "log1p" -- multiplicative
  outcomes as in `fit_causalimpact`: every series is modelled as log y (log1p y), and `summary`,
  `result[b]`, `window_summary`, the joint tables and every pooled `aggregates[name]` are on the data
  scale, from the linked draws.  A pooled draw is the sum over the members of w_b * exp(draw of series
  b): the link is applied where the draws lie, inside the summary and pool kernels
  (`_native.Session.set_link`), so a one-launch batch still downloads no draws; the routes fitted
  series by series apply `_native.link_values_host` in numpy.  A one-launch HMC batch asked for a link
  takes the per-series route (as with `components=True`).  ValueError before any fit, the series and
  the label named, for a value outside the link's domain on a row a model conditions on.
  `components` and `prediction_errors` stay on the transformed scale; the analytic `placebo=` is refused,
  `placebo=Placebo(simulate=True)` runs the simulated placebo; together with `aggregates` as
  `Placebo(simulate=True, pool=True)`, which adds the SIMULATED pooled placebo: every member's simulated
  totals at the group's origins and horizon, added draw by draw with the group's weights
  (ci_session_pool_simulated_placebo; `_native.pool_simulated_placebo_host` on the routes that filter in
  numpy), `result.aggregates[name].placebo` with the columns of the per-series simulated frame.
  """
  data_options, model_options, inference_options = _options(alpha, data_options, model_options,
                                                             inference_options)
  link = lib.resolve_outcome_link(outcome_link)
  lib.check_link_placebo(link, placebo)
  placebo = lib.resolve_placebo(placebo)
  lib.check_simulated_placebo_pool(placebo, None if aggregates is None else "aggregates")
  pl_dim = None if placebo is None else lib.placebo_state_dim(model_options.local_linear_trend,
                                                              model_options.seasons)
  if isinstance(data, np.ndarray):
    values = np.asarray(data, np.float64)
    index = pd.RangeIndex(values.shape[1]) if index is None else pd.Index(index)
    columns = ["y"] + [f"x{j}" for j in range(values.shape[2] - 1)]
  else:
    frames, columns = _frames_outcome_first(data, data_options)
    first = frames[0]
    for f in frames:
      if not f.index.equals(first.index) or list(f.columns) != list(first.columns):
        raise ValueError("all series of a batch must share the index and the columns")
    values = np.stack([f[columns].to_numpy(dtype=np.float64) for f in frames])
    index = first.index
  B = values.shape[0]
  names = list(range(B)) if names is None else list(names)
  agg = None if aggregates is None else _check_aggregates(aggregates, names, shared_streams)
  hmc = inference_options.sampler == "hmc"
  raw_values = values
  if link:
    # the models' copy: log y (log1p y) of the outcome column alone; `raw_values` stays what every
    # data-scale frame reads.  Refusals first, the series named.
    pre, _ = indices.parse_and_validate_date_data(
        data=pd.DataFrame({"y": np.zeros(len(index))}, index=index), pre_period=pre_period, post_period=post_period)
    values = raw_values.copy()
    values[:, :, 0] = lib.link_column(raw_values[:, :, 0], index, pre, link, columns[0], names)
  # float64 and raw-scale batches go series by series; every other batch is standardised float32
  per_series = (cid._as_numpy_dtype(data_options.dtype) == np.float64   # pylint: disable=protected-access
                or not data_options.standardize_data)
  if not per_series:
    prep = prepare_batch(values, index, pre_period, post_period)
    T = prep.y.shape[1]
    # the one-launch HMC path keeps no latent draws and has no component summary: asked for
    # components, an HMC batch takes the per-series route, where `fit_causalimpact` has the draws;
    # its session has no link either: asked for `outcome_link`, the same
    per_series = hmc and (inference_options.components or hmc_batch_route(
        float64=False, standardize_data=True, num_seasonal_blocks=len(model_options.seasons), T=T,
        P=0 if prep.design is None else prep.design.shape[2],
        hmc_init=inference_options.hmc_init, outcome_link=bool(link)) == "per_series")
  if per_series:
    shared = None
    if agg is not None or effect_windows is not None:   # (the shared calendar: pooled outcome, window flags)
      shared = prepare_batch(raw_values, index, pre_period, post_period, data_options.standardize_data)
    if agg is not None:
      agg = (*agg, shared)
    plan = None if effect_windows is None else batch_windows(effect_windows, shared)
    pool_plan = None
    if agg is not None and placebo is not None:
      n_post = int(np.count_nonzero(shared.flags & 2))
      pl_h, pl_o = lib.placebo_plan(placebo, shared.num_pre, n_post, pl_dim)
      pool_plan = batch_placebo_pool_plan(agg[1], pl_o if len(pl_o) else [-1], pl_h, n_post,
                                          shared.index[shared.model_rows], placebo)
    return _fit_per_series((pd.DataFrame(raw_values[b], index=index, columns=columns) for b in range(B)),
                           [(pre_period, post_period)] * B, names, columns[0], alpha, seed,
                           data_options, model_options, inference_options, shared_streams, agg,
                           windows=plan, series_windows=None if plan is None else [effect_windows] * B,
                           placebo=placebo, joint_bands=joint_bands, placebo_pool=pool_plan,
                           outcome_link=outcome_link)
  if link:
    prep = _under_link(prep, prepare_batch(raw_values, index, pre_period, post_period), link)
  plan = None if effect_windows is None else batch_windows(effect_windows, prep)
  pl_plan = pl_post = None
  if placebo is not None:
    pl_post = np.full(B, int(np.count_nonzero(prep.flags & 2)))
    pl_plan = placebo_plans(placebo, [prep.num_pre] * B, pl_post, pl_dim)
    if not np.any(pl_plan[0] >= 0):
      raise ValueError(f"placebo: a pre-period of {prep.num_pre} steps has no room for an origin with "
                       f"horizon {int(pl_plan[1][0])} and the history it needs")
  pl_hz = None if pl_plan is None else placebo_horizon_tables(placebo, pl_plan[1])
  y = _sampler_outcome(prep, data_options)
  with np.errstate(invalid="ignore"):
    pre_sd = np.nanstd(y[:, :prep.num_pre], axis=1, ddof=1)
  fit = _new_fit(prep, y, np.full(B, T), pre_sd, alpha, seed, model_options, inference_options,
                 shared_streams, plan, pl_plan, joint_bands, placebo is not None and placebo.simulate, pl_hz)
  # a batch is the panel of one group of equal lengths: consecutive positions on every device
  launches = panel_launches(dict(route="equal_length", groups=[(T, list(range(B)))]),
                            inference_options.devices, shared_streams)
  if hmc:
    from causalimpact import _hmc  # pylint: disable=import-outside-toplevel
    # one launch per part of a device's share that fits the HBM budget
    step = _hmc.series_per_launch(T, 0 if prep.design is None else prep.design.shape[2],
                                  inference_options.num_chains, inference_options.num_results)
    launches = [(dev, key, ids[lo:lo + step]) for dev, key, ids in launches
                for lo in range(0, len(ids), step)]
  chain = None if agg is None else _PoolChain(launches, agg[1])
  pool_plan = pool_seen = pl_chain = None
  if agg is not None and placebo is not None:
    pool_plan = batch_placebo_pool_plan(agg[1], pl_plan[0][0], pl_plan[1][0], pl_post[0],
                                        prep.index[prep.model_rows], placebo)
    pool_seen = _fit_placebo_observed(pool_plan, fit)
    pl_chain = _new_placebo_chain(launches, pool_plan, pool_seen, fit, placebo, alpha)
  if hmc:
    run = lambda launch: _run_hmc_launch(launch, fit, chain, pl_chain)          # pylint: disable=unnecessary-lambda-assignment
  else:
    run = lambda launch: _run_launch(launch, "ordinary", fit, chain, pl_chain)   # pylint: disable=unnecessary-lambda-assignment
  for guard in (chain, pl_chain):
    run = run if guard is None else guard.guarded(run)
  means, record, diag_draws = _assemble(launches, run, B, T)
  res = CausalImpactBatchAnalysis(
      prep, names, alpha, means, record.effect, fit.ranks, columns, diag_draws, record,
      _state_dim(model_options, inference_options),
      None if placebo is None else dict(origins=pl_plan[0], horizon=pl_plan[1], n_post=pl_post, horizons=pl_hz))
  if plan is not None:
    res.window_summary = _window_summary(res, plan, record.windows)
  if joint_bands:
    res.set_joint(record.windows, fit.path_ranks, None if plan is None else plan.names)
  if chain is not None:
    # the posterior means on the data scale with the statistics every series' own frame uses
    # (`outcome_link`: the means of the linked draws are there already)
    if link:
      data_means = np.asarray(means, np.float64)
    else:
      mu, sd = scaler_stats(prep.values[:, prep.model_rows[:prep.num_pre], 0])
      data_means = means.astype(np.float64) * sd[:, None] + mu[:, None]
    _take_aggregates(res, _aggregate_analyses(
        agg[0], agg[1], chain.result(), data_means, prep,
        columns[0], alpha, fit.ranks, launches[0][0], plan, joint_bands))
    if pl_chain is not None:
      _take_aggregate_placebo(res, pool_plan, agg[0], pl_chain.means, pool_seen, alpha)
  return res


def _window_summary(res: CausalImpactBatchAnalysis, plan: WindowPlan, wsum) -> pd.DataFrame:
  """`window_summary` of a one-launch batch or panel from the assembled window totals: the
  observations and the data-scale posterior mean of `_build_summary`, every window's own steps."""
  p = res._prep                                                  # pylint: disable=protected-access
  post_mean = res._data_means()                                  # pylint: disable=protected-access
  classes = None
  if isinstance(p, PreparedPanel):       # (the groups `panel_window_stats` reduces together)
    groups: Dict[Any, List[int]] = {}
    for b, Tb in enumerate(p.lengths):
      groups.setdefault((int(Tb), (p.flags[b, :Tb] & 2).tobytes()), []).append(b)
    classes = [(Tg, sel) for (Tg, _), sel in groups.items()]
  totals = {k: v for k, v in wsum.items() if not k.startswith("path_")}     # (`joint_bands` travels with them)
  return window_table(res._names, res.alpha, res._ranks, plan, totals, p.observed, post_mean, classes)   # pylint: disable=protected-access


def fit_causalimpact_panel(data: Sequence[pd.DataFrame], periods, alpha: float = 0.05, seed=None,
                           data_options: Optional[lib.DataOptions] = None,
                           model_options: Optional[lib.ModelOptions] = None,
                           inference_options: Optional[lib.InferenceOptions] = None,
                           names: Optional[Sequence[Any]] = None,
                           shared_streams: bool = False,
                           event_aggregates=None, effect_windows=None,
                           placebo=None, joint_bands: bool = False,
                           outcome_link=None) -> CausalImpactBatchAnalysis:
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
  does, and series b equals the single fit seeded with `_native.series_stream_key(seed, b)`.

  event_aggregates: the POOLED effect of groups of series in EVENT TIME -- the roll-out as a whole,
  every unit aligned on its own treatment start -- with its credible bands.  (There is no
  `aggregates` argument here: series with their own calendars share no calendar axis to add their
  trajectories on; `fit_causalimpact_batch(aggregates=...)` pools series of ONE calendar.)  A mapping
  {aggregate name: members} with the member syntax of `fit_causalimpact_batch(aggregates=...)`: a
  sequence of series names (weight 1), a mapping {series name: weight}, or the string "all".
  Event time tau counts the ROWS of a series from its treatment start (tau = 0 is the first step of
  its post-period), not calendar units: the series of a panel are expected to share a sampling
  interval.  The axis of a group is what all its members of non-zero weight have (`event_axes`):
  tau = -L .. H - 1 with L the fewest steps a member has before its start and H the fewest from it
  on; its pre-period ends before the longest gap any member leaves between pre-period and start, its
  post-period is the shortest window, 0 .. Hwin - 1.  Draw n of the group at tau is the sum over its
  members b of w_b * (draw n of series b at its own step start_b + tau, on the data scale), in
  float64, added on the device that holds the trajectories (csrc/ci_pool.h; they are never
  downloaded) and handed from launch to launch.  The order of addition is (length class of the
  route, position in the panel) -- the order `panel_launches` lists the launches in, ascending
  positions within a launch -- which is a function of the model and the series alone: the result is
  the same on any number of devices, bit for bit, but the order is not plain position order when
  the members fall in different length classes.  Panels fitted series by series (float64, raw
  scale, HMC) add the same windows in numpy in position order (every series is its own class
  there).  The pooled outcome and the pooled posterior mean are the same weighted sums; the pooled
  outcome is NaN wherever a member's is (gap, tail, missing value).  The result then has
  `aggregates` ({name: CausalImpactAnalysis}: the reference's `series` frame on an integer index
  named `event_time`, and `summary`; `plot` takes it as any other; no `posterior_samples`) and
  `aggregate_summary` (the 15 summary columns indexed by (aggregate, average|cumulative)); both are
  None without the argument, and nothing else changes with it.  `shared_streams=True` is refused
  with it (common random numbers make the Monte-Carlo errors of all series move together).
  ValueError, before any fit, for an unknown series name, a member listed twice, a weight that is not
  finite, a group without a member of non-zero weight, and a group whose common axis keeps fewer
  than 3 pre-period steps.

  effect_windows: {name: (tau_first, tau_last)}, windows in EVENT TIME as above (integers, both ends
  inclusive, 0 <= tau_first <= tau_last; `event_windows(7, 4)` gives four weeks of daily rows): the
  rows tau_first .. tau_last since every series' own treatment start.  The result then has
  `window_summary`, the 15 summary columns indexed by (series, window, average|cumulative), as in
  `fit_causalimpact_batch`; a series whose post-period does not reach tau_last has NaN rows for that
  window, and a window that no series covers is a ValueError before any fit.  With
  `event_aggregates` also `aggregate_window_summary`, the windows taken on every group's own axis
  (NaN rows where its post-period, the shortest of its members', does not cover them).

  placebo: as in `fit_causalimpact_batch`, every series with the horizon and the origins of its OWN
  pre- and post-period.  A series whose pre-period has no room for an origin has an empty
  `placebo` frame and a NaN row (n_origins 0) in `placebo_quality` -- no error.  With
  `event_aggregates` every pooled group gets the check as in `fit_causalimpact_batch`, in EVENT TIME:
  group g has the horizon and the origins of `lib.placebo_plan` on the pre-period and the window all
  its members share (L - gap steps, Hwin), member k forecasts from its own step first_k + column --
  inside its own pre-period -- and `result.aggregates[name].placebo` is indexed by `event_time`
  (negative: before the treatment start).  A group without room for an origin has the empty frame and
  the NaN row; `result.aggregate_placebo_quality` has one row per aggregate.  With
  `Placebo(horizons=...)` every series keeps the listed horizons <= its own H (none is refused) and
  `result.placebo_profile`, indexed by (series, horizon), has NaN rows for the horizons a series lacks;
  with `event_aggregates` every group keeps the listed horizons <= its own H_g likewise:
  `result.aggregates[name].placebo_by_horizon` / `.placebo_profile` on the group's event-time axis and
  `result.aggregate_placebo_profile`, indexed by (aggregate, horizon), with NaN rows where a group lacks
  a horizon.

  joint_bands: as in `fit_causalimpact_batch`, every series over its OWN post-period and the
  `effect_windows` in event time; `window_joint_summary` has NaN rows where a series' post-period does
  not reach a window.  With `event_aggregates` every pooled group gets `joint_bands`, `joint_summary`
  and `window_joint_summary` on its own `event_time` axis, and the result
  `aggregate_joint_summary` and `aggregate_window_joint_summary` as in `fit_causalimpact_batch`, with
  blank rows where a group's axis does not reach a window.

  outcome_link: as in `fit_causalimpact_batch` -- every series modelled as log y (log1p y), every
  table, frame and pooled `aggregates[name]` on the data scale from the linked draws, the link applied
  by the summary and pool kernels of every ragged launch; panels fitted series by series in numpy.
  ValueError before any fit, the series and the label named, for a value outside the link's domain on
  a row its model conditions on.  `components` and `prediction_errors` stay on the transformed scale;
  the analytic `placebo=` is refused; `placebo=Placebo(simulate=True)` runs the simulated placebo, together
  with `event_aggregates` as `Placebo(simulate=True, pool=True)`: the simulated pooled placebo in event
  time, as in `fit_causalimpact_batch`."""
  data_options, model_options, inference_options = _options(alpha, data_options, model_options,
                                                             inference_options)
  link = lib.resolve_outcome_link(outcome_link)
  lib.check_link_placebo(link, placebo)
  placebo = lib.resolve_placebo(placebo)
  lib.check_simulated_placebo_pool(placebo, None if event_aggregates is None else "event_aggregates",
                                   "event_aggregates")
  pl_dim = None if placebo is None else lib.placebo_state_dim(model_options.local_linear_trend,
                                                              model_options.seasons)
  frames, columns = _frames_outcome_first(data, data_options)
  B = len(frames)
  periods = list(periods)
  if len(periods) != B:
    raise ValueError(f"`periods` must hold one (pre_period, post_period) per series: {B} series, "
                     f"{len(periods)} periods")
  names = list(range(B)) if names is None else list(names)
  agg = (None if event_aggregates is None else
         _check_aggregates(event_aggregates, names, shared_streams, "event_aggregates"))
  for b, f in enumerate(frames):
    if list(f.columns) != list(frames[0].columns):
      raise ValueError(f"series {names[b]!r}: all series of a panel must share the columns")
  float64 = cid._as_numpy_dtype(data_options.dtype) == np.float64  # pylint: disable=protected-access
  num_blocks = len(model_options.seasons)
  model_frames = None
  if link:
    # the models' copies (log y, log1p y of the outcome column alone); refusals first, the series named
    model_frames = [lib.link_outcome(f[columns], periods[b][0], periods[b][1], columns[0], link, names[b])
                    for b, f in enumerate(frames)]
  # (which panels go series by series does not depend on the lengths: the frames' bound them here)
  if panel_route(float64=float64, standardize_data=data_options.standardize_data,
                 sampler=inference_options.sampler, num_seasonal_blocks=num_blocks,
                 P=len(columns), lengths=[len(f) for f in frames])["route"] == "per_series":
    plan = wplan = own = None
    if agg is not None or effect_windows is not None:
      # (the event axes and the windows come from the prepared panel; the fits prepare their own data)
      shared = prepare_panel([f[columns] for f in frames], periods, data_options.standardize_data,
                             names=names)
      plan = None if agg is None else event_plan(*agg, shared, columns[0])
    if effect_windows is not None:
      wplan = panel_windows(effect_windows, shared)
      # every fit reads integers as POSITIONS into its own index: the rows of its covered windows
      own = [{name: (int(shared.model_rows[b][f]), int(shared.model_rows[b][f + c - 1]))
              for name, f, c in zip(wplan.names, wplan.first[b], wplan.count[b]) if c > 0} or None
             for b in range(B)]
    return _fit_per_series(frames, periods, names, columns[0], alpha, seed, data_options,
                           model_options, inference_options, shared_streams, event_aggregates=plan,
                           windows=wplan, series_windows=own, placebo=placebo, placebo_lenient=True,
                           joint_bands=joint_bands,
                           placebo_pool=None if plan is None or placebo is None else
                           event_placebo_pool_plan(placebo, plan, pl_dim), outcome_link=outcome_link)
  prep = prepare_panel(model_frames or [f[columns] for f in frames], periods, names=names)
  if link:
    prep = _under_link(prep, prepare_panel([f[columns] for f in frames], periods, names=names), link)
  pl_plan = pl_post = None
  if placebo is not None:
    pl_post = np.array([np.count_nonzero(prep.flags[b, :Tb] & 2) for b, Tb in enumerate(prep.lengths)])
    pl_plan = placebo_plans(placebo, prep.num_pre, pl_post, pl_dim)
  pl_hz = None if pl_plan is None else placebo_horizon_tables(placebo, pl_plan[1], strict=False)
  plan = None if agg is None else event_plan(*agg, prep, columns[0])
  wplan = None if effect_windows is None else panel_windows(effect_windows, prep)
  route = panel_route(float64=False, standardize_data=True, sampler="gibbs",
                      num_seasonal_blocks=num_blocks,
                      P=0 if prep.design is None else prep.design.shape[2], lengths=prep.lengths,
                      num_seasons=_model.expand_seasons(model_options.seasons, 1)[0])
  y = _sampler_outcome(prep, data_options)
  with np.errstate(invalid="ignore"):
    pre_sd = [np.nanstd(y[b, :nb], ddof=1) for b, nb in enumerate(prep.num_pre)]
  fit = _new_fit(prep, y, prep.lengths, pre_sd, alpha, seed, model_options, inference_options,
                 shared_streams, wplan, pl_plan, joint_bands, placebo is not None and placebo.simulate, pl_hz)
  kind = "ordinary" if route["route"] == "equal_length" else route["route"]
  launches = panel_launches(route, inference_options.devices, shared_streams)
  chain = None if plan is None else _PoolChain(launches, plan.csr, plan.axes)
  pool_plan = pool_seen = pl_chain = None
  if plan is not None and placebo is not None:
    pool_plan = event_placebo_pool_plan(placebo, plan, pl_dim)
    pool_seen = _fit_placebo_observed(pool_plan, fit)
    pl_chain = _new_placebo_chain(launches, pool_plan, pool_seen, fit, placebo, alpha)
  run = lambda launch: _run_launch(launch, kind, fit, chain, pl_chain)   # pylint: disable=unnecessary-lambda-assignment
  for guard in (chain, pl_chain):
    run = run if guard is None else guard.guarded(run)
  means, record, diag_draws = _assemble(launches, run, B, prep.y.shape[1])
  res = CausalImpactPanelAnalysis(
      prep, names, alpha, means, record.effect, fit.ranks, columns, diag_draws, record,
      _state_dim(model_options, inference_options),
      None if placebo is None else dict(origins=pl_plan[0], horizon=pl_plan[1], n_post=pl_post, horizons=pl_hz))
  if wplan is not None:
    res.window_summary = _window_summary(res, wplan, record.windows)
  if joint_bands:
    res.set_joint(record.windows, fit.path_ranks, None if wplan is None else wplan.names)
  if chain is not None:
    # the posterior means on the data scale with the statistics every series' own frame uses
    data_means = []
    for b, (Tb, nb) in enumerate(zip(prep.lengths, prep.num_pre)):
      if link:                 # (the means of the linked draws are on the data scale already)
        data_means.append(np.asarray(means[b, :Tb], np.float64))
        continue
      mu, sd = scaler_stats(prep.raw[b][prep.model_rows[b][:nb], 0][None])
      data_means.append(means[b, :Tb].astype(np.float64) * sd[0] + mu[0])
    _take_aggregates(res, _event_aggregate_analyses(
        plan, chain.result(), data_means, alpha, fit.ranks, launches[0][0], wplan, joint_bands))
    if pl_chain is not None:
      _take_aggregate_placebo(res, pool_plan, plan.names, pl_chain.means, pool_seen, alpha)
  return res
