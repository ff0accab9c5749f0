"""fit_causalimpact() on MI355X: the reference's public surface over the HIP Gibbs kernel.

Drop-in for /root/reference/causalimpact/causalimpact_lib.py: same function / dataclass
names, argument meaning, result frames and error behaviour.  What changed underneath:

  * `_train_causalimpact_sts` (reference :503-606) no longer builds a TFP model and traces a
    tf.function; it packs plain arrays and calls the C-ABI (`_native.fit_gibbs`), which runs
    every Gibbs iteration of every chain inside one persistent HIP kernel.
  * tensors in the results are numpy arrays (subclass with a `.numpy()` method so code written
    against the reference keeps working).
  * extensions BASELINE.json asks for, all optional: `InferenceOptions.num_chains`,
    `InferenceOptions.devices`, `ModelOptions.local_linear_trend`.

Host-side post-processing (reference :635-1093) is re-implemented on numpy arrays and pinned
against the reference's own output by tests/test_golden_postprocessing.py.
"""
import collections.abc
import copy
import dataclasses
import math
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import pandas as pd

from causalimpact import _diagnostics
from causalimpact import _model
from causalimpact import _native
from causalimpact import data as cid
from causalimpact import indices
from causalimpact import posterior_processing
from causalimpact.indices import InputDateType
from causalimpact.indices import OutputDateType
from causalimpact.indices import OutputPeriodType

_SeedType = Union[int, Tuple[int, int], Sequence[int]]
_KEPT_AFTER_POST = ["observed", "posterior_mean", "posterior_lower", "posterior_upper"]


class Tensor(np.ndarray):
  """numpy array that also answers `.numpy()` like the reference's tf.Tensor results."""

  def numpy(self):
    return np.asarray(self)


def _tensor(a) -> Tensor:
  return np.asarray(a).view(Tensor)


class _LazyMapping(collections.abc.Mapping):
  """A read-only dict whose content is computed on first use (the convergence diagnostics cost
  as much host time as a third of the fit; most callers never read them)."""

  def __init__(self, make):
    self._make, self._value = make, None

  def _get(self):
    if self._value is None:
      self._value = dict(self._make())
      self._make = None
    return self._value

  def __getitem__(self, key):
    return self._get()[key]

  def __iter__(self):
    return iter(self._get())

  def __len__(self):
    return len(self._get())

  def __repr__(self):
    return repr(self._get())

  def __reduce__(self):
    # pickles (multiprocessing, joblib, caches) as the plain dict it stands for
    return (dict, (self._get(),))


@dataclasses.dataclass
class CausalImpactPosteriorSamples:
  """Draws of the model's latents (reference :44-58).  Leading axis = pooled draws
  (chains x num_results, chain-major)."""
  observation_noise_scale: np.ndarray           # [draws]
  level_scale: Optional[np.ndarray]             # [draws]
  level: Optional[np.ndarray]                   # [draws, T]
  weights: Optional[np.ndarray]                 # [draws, covariates + 1] or None
  seasonal_drift_scales: Optional[np.ndarray]   # [draws, K] or None
  seasonal_levels: Optional[np.ndarray]         # [draws, T, K]
  slope_scale: Optional[np.ndarray] = None      # [draws]      (local_linear_trend only)
  slope: Optional[np.ndarray] = None            # [draws, T]   (local_linear_trend only)


@dataclasses.dataclass
class CausalImpactAnalysis:
  """series / summary frames + posterior draws (reference :61-144; schemas SURVEY App. E)."""
  series: pd.DataFrame
  summary: pd.DataFrame
  posterior_samples: CausalImpactPosteriorSamples
  diagnostics: Optional[Dict[str, Any]] = None   # split-R-hat per scalar when num_chains > 1
  # InferenceOptions(components=True) only.  `components`: indexed like `series`; posterior mean and
  # alpha/2, 1 - alpha/2 quantiles of the trend, every seasonal block and the regression term on the
  # data scale (trend, trend_lower, trend_upper, seasonal_<k>..., regression...).  `coefficients`:
  # one row per design column (the intercept included) with inclusion_probability, mean, lower,
  # upper of its weight on the model's scale; None for a model without covariates.
  components: Optional[pd.DataFrame] = None
  coefficients: Optional[pd.DataFrame] = None
  # InferenceOptions(prediction_errors=True) only.  `prediction_errors`: indexed like `series`, NaN on
  # the rows the model never sees; per step the one-step-ahead forecast of the Kalman filter run with
  # every draw's scales and weights (forecast: mean over the draws; forecast_lower / forecast_upper:
  # alpha/2 and 1 - alpha/2 quantiles over the draws; forecast_sd: root of the mean predictive
  # variance), error = observed - forecast, standardized_error = error / forecast_sd and pit, the
  # mean over the draws of Phi(v / sqrt F) -- the mixture-predictive CDF at the observation.  The last
  # three are NaN where the model does not condition on the observation (post-period, missing
  # values); `forecast` is the several-steps-ahead forecast from the last observation there.
  # `fit_quality`: n_scored, rmse, mae, mase (below 1: the model beats a random walk), coverage
  # (share of scored steps with alpha/2 <= pit <= 1 - alpha/2; nominal 1 - alpha), loglik_mean,
  # loglik_sd (over the draws, in the sampler's units) over the observed pre-period steps t >= the
  # state dimension.  (Init-only pseudo-fields kept as plain attributes: `dataclasses.fields` and
  # `asdict` of this class stay what they were.)
  prediction_errors: dataclasses.InitVar[Optional[pd.DataFrame]] = None
  fit_quality: dataclasses.InitVar[Optional[pd.Series]] = None
  # `effect_windows=` only: the 15 columns of `summary` for every sub-window of the post-period,
  # indexed by (window, average|cumulative).  (Init-only and kept as a plain attribute, as the two above.)
  window_summary: dataclasses.InitVar[Optional[pd.DataFrame]] = None
  # `placebo=` only (see `Placebo`).  `placebo`: one row per placebo origin, indexed by the origin's
  # label on the series' index, with the `PLACEBO_COLUMNS`: horizon_end (the label of the window's
  # last step), n_counted (observed steps of the window), actual (the sum of the data over them),
  # predicted (the forecast of that sum from the origin without any update, mean over the draws),
  # predicted_sd (root of the mixture's predictive variance, observation noise included), effect,
  # relative_effect, pit (the mixture-predictive CDF at the actual sum), p = 2 min(pit, 1 - pit) and
  # significant (pit outside [alpha/2, 1 - alpha/2]).  `placebo_quality`: the `PLACEBO_QUALITY_ENTRIES`
  # n_origins, horizon, false_positive_rate (nominal alpha), mean_relative_effect, mde_relative (the
  # 1 - alpha quantile of |relative_effect|: the smallest relative effect the data could tell from
  # noise at this horizon) and empirical_p (the rank of the fit's cumulative relative effect among
  # the placebo ones; NaN unless the horizon is the post-period's).  The windows OVERLAP: the
  # origins are not independent trials.  (Init-only and kept as plain attributes, as those above.)
  placebo: dataclasses.InitVar[Optional[pd.DataFrame]] = None
  placebo_quality: dataclasses.InitVar[Optional[pd.Series]] = None
  # `joint_bands=True` only.  `joint_bands`: indexed like `series`, NaN outside the post-period; the
  # `JOINT_BAND_COLUMNS` -- SIMULTANEOUS bands: the counterfactual path lies inside posterior_lower ..
  # posterior_upper at every step at once with probability 1 - alpha (center -+ c * spread of the
  # draws, c the 1 - alpha quantile of every draw's largest standardised excursion), the same for the
  # point effects (observed minus that band) and, with its own c, for the cumulative effect; `outside`:
  # the observation lies outside the posterior band at that step.  `joint_summary`: one row for
  # `pointwise` (the observed path against the predictive paths) and one for `cumulative` (the
  # cumulative effect against 0) with the `JOINT_SUMMARY_COLUMNS`: critical_value (c), max_excursion
  # (the observed path's largest standardised excursion), at (its label), n_outside, first_outside,
  # p = (1 + #{draws whose excursion reaches it}) / (1 + draws) and significant = max_excursion >
  # critical_value = some step is outside.  An effect that rises and reverses shows here and not in
  # `summary`.  `window_joint_summary` (with `effect_windows=`): the same table per window, indexed by
  # (window, pointwise|cumulative), critical value and test taken over the window's steps alone.
  # The analysis of a pooled group (`aggregates`, `event_aggregates`) carries all three as well, from
  # its pooled draws (`batch._aggregate_paths`).  (Init-only and kept as plain attributes, as those above.)
  joint_bands: dataclasses.InitVar[Optional[pd.DataFrame]] = None
  joint_summary: dataclasses.InitVar[Optional[pd.DataFrame]] = None
  window_joint_summary: dataclasses.InitVar[Optional[pd.DataFrame]] = None
  # `placebo=Placebo(horizons=...)` only: the placebo check at several horizons h <= H from the SAME
  # origins (those of the plan at H).  `placebo_by_horizon`: the `PLACEBO_COLUMNS` indexed by (origin,
  # horizon), horizon_end, n_counted, actual and the rest taken per horizon; `.xs(H, level="horizon")`
  # is `placebo`.  `placebo_profile`: indexed by horizon, the `PLACEBO_PROFILE_COLUMNS` -- the entries
  # of `placebo_quality` at that horizon (its last row is `placebo_quality`; empirical_p only on the row
  # h == n_post) and relative_sd, the median over the counted origins of predicted_sd / |predicted|:
  # how mde_relative and the false-positive rate move with the window's length, and from which horizon
  # on the model drifts.  (Init-only and kept as plain attributes, as those above.)
  placebo_by_horizon: dataclasses.InitVar[Optional[pd.DataFrame]] = None
  placebo_profile: dataclasses.InitVar[Optional[pd.DataFrame]] = None

  def __post_init__(self, prediction_errors, fit_quality, window_summary=None, placebo=None,
                    placebo_quality=None, joint_bands=None, joint_summary=None, window_joint_summary=None,
                    placebo_by_horizon=None, placebo_profile=None):
    self.placebo_by_horizon, self.placebo_profile = placebo_by_horizon, placebo_profile
    self.prediction_errors, self.fit_quality = prediction_errors, fit_quality
    self.window_summary = window_summary
    self.placebo, self.placebo_quality = placebo, placebo_quality
    self.joint_bands, self.joint_summary = joint_bands, joint_summary
    self.window_joint_summary = window_joint_summary


@dataclasses.dataclass
class DataOptions:
  """reference :147-159.  dtype may be numpy / python float types (or anything with a
  `.name` of "float32"/"float64").  The Gibbs sampler computes in that type (float64: the kernels
  of csrc/ci_gibbs64.h, draw for draw equal to the float64 oracle); the HMC extension computes in
  float32 for either."""
  outcome_column: Optional[str] = None
  standardize_data: bool = True
  dtype: Any = np.float32


@dataclasses.dataclass(frozen=True)
class Seasons:
  """One seasonal effect (reference :162-180): int, per-season tuple or per-cycle table."""
  num_seasons: int
  num_steps_per_season: Union[int, Tuple[int, ...], Tuple[Tuple[int, ...], ...]] = 1


@dataclasses.dataclass
class ModelOptions:
  """reference :183-203 (+ local_linear_trend, the BASELINE cfg2 extension)."""
  prior_level_sd: float = 0.01
  seasons: List[Seasons] = dataclasses.field(default_factory=list)
  local_linear_trend: bool = False


@dataclasses.dataclass
class InferenceOptions:
  """reference :206-220 (+ num_chains / devices / sampler extensions; defaults reproduce the
  reference: one Gibbs chain)."""
  num_results: int = 900
  num_warmup_steps: Optional[int] = None
  num_chains: int = 1
  devices: Optional[Sequence[int]] = None
  sampler: str = "gibbs"          # "gibbs" (the reference's sampler) or "hmc" (extension, _hmc.py)
  hmc_init: str = "gibbs"         # HMC chains start at the Gibbs initial state, or ("vi") at draws
                                  # of a mean-field surrogate posterior (_vi.py), as tfp.sts.fit_with_hmc
  hmc_prior: str = "slab"         # HMC regression prior: "slab" (Gaussian slab of the reference's
                                  # spike-and-slab prior) or "horseshoe" (tfp.sts.SparseLinearRegression)
  # Quantiles / effect sums of the T x (chains * draws) predictive draws computed on the GPU that
  # holds them (csrc/ci_summary.h) instead of pandas on the host.  Single-device Gibbs fits only;
  # `False` keeps the reference's host arithmetic (and downloads the trajectories).
  summarize_on_device: bool = True
  # CI_FLAG_* bits handed to the C-ABI (include/causalimpact_amd.h), e.g. `_native.FLAG_NO_CLUSTER`
  # on a GPU shared with other jobs: the time-parallel seasonal kernel then runs one workgroup per
  # chain instead of spin-synchronised clusters of CUs (same draws, bit for bit).
  kernel_flags: int = 0
  # Also summarise the trend, every seasonal block, the regression term and the regression weights
  # over the draws (`CausalImpactAnalysis.components` / `.coefficients`): on the GPU that holds the
  # draws wherever the predictive summary runs there (csrc/ci_components.h), also for batches and
  # panels, which keep no draws; in numpy from the pooled draws on the other routes.
  components: bool = False
  # Also score the model: one-step-ahead prediction errors of the Kalman filter run with every
  # draw's parameters (`CausalImpactAnalysis.prediction_errors` / `.fit_quality`, the check `bsts`
  # users know as bsts.prediction.errors).  On the GPU that holds the draws wherever the predictive
  # summary runs there (csrc/ci_predict.h), also for batches and panels; in numpy from the parameter
  # draws on the other routes.  (An init-only pseudo-field kept as a plain attribute: the fields,
  # `asdict` and equality of the options stay what they were.)
  prediction_errors: dataclasses.InitVar[bool] = False

  def __post_init__(self, prediction_errors=False):
    self.prediction_errors = bool(prediction_errors)
    if self.num_warmup_steps is None:
      self.num_warmup_steps = math.ceil(self.num_results / 9)


def fit_causalimpact(data: pd.DataFrame,
                     pre_period: Tuple[InputDateType, InputDateType],
                     post_period: Tuple[InputDateType, InputDateType],
                     alpha: float = 0.05,
                     seed: Optional[_SeedType] = None,
                     data_options: Optional[DataOptions] = None,
                     model_options: Optional[ModelOptions] = None,
                     inference_options: Optional[InferenceOptions] = None,
                     effect_windows=None,
                     placebo=None,
                     joint_bands=False,
                     outcome_link=None,
                     **kwargs) -> CausalImpactAnalysis:
  """Fits the CausalImpact model and summarises the effect (reference :223-339).

  outcome_link (extension): None (the default: nothing runs, no result differs), "log" or "log1p",
  for outcomes that move multiplicatively (revenue, conversions, counts).  The outcome column alone
  is transformed (log y, log1p y) before standardisation -- the model, the kernels and the draws are
  exactly those of fitting the pre-transformed frame, and `posterior_samples` stay on the model's
  scale -- but `series`, `summary`, `window_summary` and the joint bands are on the DATA scale, from
  the linked draws: exp (expm1) is applied to every predictive draw before any mean, sum or
  quantile, because E[exp z] != exp E[z].  The posterior mean is the mean of the linked draws.
  `observed` is the input column itself.  On the GPU that holds the draws wherever the summaries run
  there (`_native.Session.set_link`), the same definitions in numpy (`_native.link_values_host`) on
  the routes that pool the draws on the host.  Every row the model conditions on needs y > 0 (log)
  or y > -1 (log1p): ValueError before any fit, the first offending label named; a post-period value
  outside the domain (sales driven to 0) is a missing value to the model's copy alone.
  `components=True` and `prediction_errors=True` describe the model, which is Gaussian on the
  TRANSFORMED scale: they are reported there.  The analytic `placebo=` with a link is refused
  (ValueError): a sum of lognormals has no closed-form variance; `placebo=Placebo(simulate=True)` runs
  the simulated placebo instead (see `Placebo`).

  effect_windows (extension): {name: (start, end)}, sub-windows of the post-period given as labels
  on the index, both ends inclusive, parsed and aligned exactly as `post_period` is.  The result then
  has `window_summary`: the 15 columns of `summary` for every window, indexed by (window,
  average|cumulative) -- how the effect unfolds (week 1 against week 4, a promotion's second phase).
  The bands, the relative effect and `p_value` of a window come from every draw's total over that
  window (csrc/ci_windows.h on the GPU that holds the draws; `_native.window_totals_host` on the
  routes that pool them on the host).  ValueError, before any fit and with the window named, for a
  window that leaves the post-period or contains no model row.  None (the default): `window_summary`
  is None and nothing runs.

  placebo (extension): None (the default: nothing runs, no result differs), True or a `Placebo`.
  The treatment is pretended to begin at several earlier dates inside the pre-period and the model
  forecasts a post-period's length from each without updating: the result then has `placebo` (one row
  per origin) and `placebo_quality` (false-positive rate, the minimal detectable relative effect, the
  empirical p-value of the fit's cumulative effect) -- whether a cumulative band of that length can
  be trusted.  This is the FIXED-PARAMETER placebo: every draw's scales and weights come from the one
  fit of the whole pre-period, nothing is refitted, which makes the check cheap and somewhat
  optimistic; the windows overlap, so the origins are not independent trials.  On the GPU that holds
  the draws wherever the predictive summary runs there (csrc/ci_placebo.h; csrc/ci_placebo_blocks.h for
  more than one seasonal block or a block of more than 7 seasons), in numpy from the
  parameter draws on the other routes, exactly as `InferenceOptions.prediction_errors`.  ValueError
  before any fit when the pre-period has no room for one origin, or the state has more than
  `PREDICTION_MAX_STATE` components.  `Placebo(simulate=True)`: the simulated placebo -- one path of
  every window per draw, the link applied step by step, band and `p` from the N totals
  (csrc/ci_placebo.h `placebo_sim_kernel`; `_placebo_simulated_host` on the other routes); the frame
  gains `predicted_lower` and `predicted_upper`.  `Placebo(horizons=...)`: the same check at several
  horizons h <= H from the origins of the plan at H, in one pass of the filter
  (ci_session_summarize_placebo_horizons; one call of the block-model entry per horizon for the
  other block lists, `_placebo_summary_host(horizons=...)` in numpy): the result gains
  `placebo_by_horizon` and `placebo_profile`; ValueError before any fit for a listed horizon beyond
  H, for more than `MAX_PLACEBO_HORIZONS` and together with `simulate=True`.

  joint_bands (extension): False (the default: nothing runs, no result differs) or True.  The bands
  of `series` are pointwise: over a long post-period the observed series leaves them at several steps
  by chance alone, and the total of `summary` misses an effect that rises and then reverses.  The
  result then has `joint_bands` (simultaneous bands: the whole counterfactual path lies inside with
  probability 1 - alpha), `joint_summary` (one p-value for "the observed path is unlike every
  predictive path", for the prediction and for the cumulative effect) and, with `effect_windows`,
  `window_joint_summary` -- see `CausalImpactAnalysis`.  They need every draw's largest standardised
  excursion over its whole path: computed where the draws lie (csrc/ci_paths.h on the GPU that holds
  them; `_native.path_excursions_host` on the routes that pool them on the host).  The bands are of
  the posterior predictive; nothing is refitted."""
  data_options = data_options if data_options is not None else DataOptions()
  model_options = model_options if model_options is not None else ModelOptions()
  inference_options = inference_options if inference_options is not None else InferenceOptions()
  experimental_model = kwargs.pop("experimental_model", None)
  kwargs.pop("experimental_tf_function_cache_key_addition", 0)   # no graph cache to key
  # (internal, batch.py: the running sums of a batch's aggregates on the routes that fit series by
  #  series) called with (posterior_means [T], posterior_trajectories [draws, T], scale, shift):
  #  data-scale value = array * scale + shift
  trajectory_sink = kwargs.pop("_trajectory_sink", None)
  # (internal, batch.py: the pooled placebo forecasts of the same routes) called with
  #  forecast(origins [O], horizon) -> `_placebo_entry_host` of this fit's draws: the per-draw terms
  #  of whatever origins and horizon a group asks of this series, on the data scale
  placebo_sink = kwargs.pop("_placebo_sink", None)
  # (internal, batch.py: a panel's series without room for a placebo origin gets the NaN row)
  placebo_lenient = kwargs.pop("_placebo_lenient", False)
  if kwargs:
    raise TypeError(f"Received unknown {kwargs=}")
  if experimental_model is not None:
    raise NotImplementedError(
        "experimental_model takes a tfp.sts.StructuralTimeSeries; this build has no TFP. Use "
        "ModelOptions(local_linear_trend=..., seasons=...) instead.")
  link = resolve_outcome_link(outcome_link)
  check_link_placebo(link, placebo)
  if placebo_sink is None:
    check_single_fit_placebo(placebo)
  raw_data = None
  if link:
    raw_data, data = data, link_outcome(data, pre_period, post_period, data_options.outcome_column, link)

  ci_data = cid.CausalImpactData(
      data=data, pre_period=pre_period, post_period=post_period,
      outcome_column=data_options.outcome_column,
      standardize_data=data_options.standardize_data, dtype=data_options.dtype)
  if not 0 < alpha < 1:
    raise ValueError("`alpha` must be between 0 and 1.")
  base = _device_summary_request(ci_data, alpha)
  # under a link: the effect is summarised on the data scale, against the raw outcome; `ci_view` is
  # `ci_data` as the data-scale frames see it, `model_observed` what the model's own checks compare
  ci_view, model_observed = ci_data, base["observed"]
  if link:
    ci_view = _data_scale_view(ci_data, raw_data)
    base = dict(base, observed=_device_summary_request(ci_view, alpha)["observed"])
  windows = None
  if effect_windows is not None:
    windows = resolve_windows(effect_windows, ci_data.data.index,
                              posterior_processing.model_index(ci_data), ci_data.post_period)
  if inference_options.prediction_errors:
    state_dim = check_prediction_state(model_options.local_linear_trend, model_options.seasons)
  placebo_part = None
  placebo = resolve_placebo(placebo)
  sink_simulated = None
  if placebo is not None and placebo.pool and placebo_sink is not None:
    # (batch.py, the simulated pooled placebo: the sink's totals are drawn from this fit's own stream)
    seed = _sanitize_seed(seed)
    sink_simulated = (link, placebo_stream(seed, None, range(inference_options.num_chains)))
  if placebo is not None:
    n_post = int(np.count_nonzero(base["flags"] & 2))
    n_pre = base["flags"].shape[0] - ci_data.model_after_pre_data.shape[0]
    horizon, origins = placebo_plan(
        placebo, n_pre, n_post, placebo_state_dim(model_options.local_linear_trend, model_options.seasons))
    if origins.size == 0 and not placebo_lenient:
      raise ValueError(f"placebo: a pre-period of {n_pre} steps has no room for an origin with "
                       f"horizon {horizon} and the history it needs")
    # (`Placebo(horizons=...)`: refused here, before the fit, where a listed horizon is beyond H)
    placebo_horizons = placebo_horizon_list(placebo, horizon, strict=not placebo_lenient)
    if origins.size:
      placebo_part = PlaceboPart(base["scale"], base["shift"], origins, horizon, horizons=placebo_horizons)
      if placebo.simulate:
        # (the simulation draws from the fit's own streams: a seed of None is settled here, once;
        #  one device or several, the chains are pooled in the order of their global ids)
        seed = _sanitize_seed(seed)
        placebo_part = placebo_part._replace(
            quantiles=base["quantiles"], link=link,
            streams=placebo_stream(seed, None, range(inference_options.num_chains)))
  num_draws = inference_options.num_chains * inference_options.num_results
  ranks = _summary_ranks(num_draws, base["quantiles"])
  path_windows = None
  if joint_bands:
    path_windows = joint_windows(base["flags"], None if not windows else
                                 Windows([w.first for w in windows], [w.count for w in windows]))
  request = SummaryRequest(
      scale=base["scale"], shift=base["shift"], observed=base["observed"], flags=base["flags"],
      ranks=ranks, components=inference_options.components,
      predictions=Affine(base["scale"], base["shift"]) if inference_options.prediction_errors else None,
      windows=Windows([w.first for w in windows], [w.count for w in windows]) if windows else None,
      placebo=placebo_part, on_device=inference_options.summarize_on_device,
      keep_trajectories=trajectory_sink is not None,
      paths=path_windows, path_ranks=_path_ranks(num_draws, alpha) if joint_bands else (), link=link)
  samples, posterior_means, posterior_trajectories, record = _run_sampler(
      ci_data=ci_data, prior_level_sd=model_options.prior_level_sd, seed=seed,
      num_results=inference_options.num_results,
      num_warmup_steps=inference_options.num_warmup_steps, dtype=data_options.dtype,
      seasons=model_options.seasons, num_chains=inference_options.num_chains,
      devices=inference_options.devices, local_linear_trend=model_options.local_linear_trend,
      sampler=inference_options.sampler, request=request,
      hmc_init=inference_options.hmc_init, hmc_prior=inference_options.hmc_prior,
      kernel_flags=inference_options.kernel_flags, placebo_sink=placebo_sink, sink_simulated=sink_simulated)
  if link:
    # the predictive arrays on the data scale: the linked draws (where the host has them) and the mean
    # of the linked draws, never the link of the mean
    if posterior_trajectories is not None:
      posterior_trajectories = _native.link_values_host(
          np.asarray(posterior_trajectories, np.float64) * np.float64(base["scale"]) + np.float64(base["shift"]),
          link)
    posterior_means = (record.effect["value_mean"] if record.effect is not None
                       else posterior_trajectories.mean(axis=0))
  if trajectory_sink is not None:
    trajectory_sink(posterior_means, posterior_trajectories, *((1.0, 0.0) if link else
                                                               (base["scale"], base["shift"])))
  # (draws pooled on the host -- several devices, float64, HMC -- were summarised inside
  #  _run_sampler, in the sampler's internal units)
  if record.effect is not None:
    series, summary, window_summary = _compute_impact_device(
        posterior_means, record.effect, base["observed"], base["flags"], ranks, ci_view, alpha,
        windows=windows or (),
        window_totals=None if record.windows is None else record.windows.get("per_draw"))
  else:
    series, summary, window_summary = _compute_impact(
        posterior_means=posterior_means, posterior_trajectories=posterior_trajectories,
        ci_data=ci_view, alpha=alpha, windows=windows or ())
  has_weights = samples["weights"].shape[-1] > 0
  has_seasons = samples["seasonal_drift_scales"].shape[-1] > 0
  posterior = CausalImpactPosteriorSamples(
      observation_noise_scale=_tensor(samples["observation_noise_scale"]),
      level_scale=_tensor(samples["level_scale"]),
      level=_tensor(samples["level"]),
      weights=_tensor(samples["weights"]) if has_weights else None,                 # :330-331
      seasonal_drift_scales=(_tensor(samples["seasonal_drift_scales"])
                             if has_seasons else None),                              # :332-334
      seasonal_levels=_tensor(samples["seasonal_levels"]),                           # :312-322
      slope_scale=_tensor(samples["slope_scale"]) if model_options.local_linear_trend else None,
      slope=_tensor(samples["slope"]) if model_options.local_linear_trend else None)
  components = coefficients = None
  if inference_options.components:
    csum = record.components
    if csum is None:
      # the routes that pool the draws on the host: the same definitions in numpy.  X is the design
      # as the sampler saw it (float64 for the float64 Gibbs kernels, float32 otherwise).
      X = None
      if has_weights:
        f64 = (cid._as_numpy_dtype(data_options.dtype) == np.float64   # pylint: disable=protected-access
               and inference_options.sampler == "gibbs")
        X = np.asarray(ci_data.feature_ts.values, np.float64 if f64 else np.float32)
      csum = _component_summary_host(samples["level"], samples["seasonal_levels"],
                                     samples["weights"] if has_weights else None, X,
                                     base["scale"], base["shift"], ranks)
    components, coefficients = _component_frames(
        csum, ranks, samples["level"].shape[0], alpha, posterior_processing.model_index(ci_data),
        ci_data.data.index,
        list(ci_data.feature_ts.columns) if ci_data.feature_ts is not None else None)
  prediction_errors = fit_quality = None
  if record.predictions is not None:
    prediction_errors, fit_quality = _prediction_frames(
        record.predictions, ranks, alpha, model_observed, ~_model_mask(ci_data), state_dim,
        posterior_processing.model_index(ci_data), ci_data.data.index)
  placebo_frame = placebo_quality = None
  if placebo is not None:
    placebo_frame, placebo_quality = _placebo_frames(
        record.placebo, origins, horizon, alpha, base["observed"],
        posterior_processing.model_index(ci_data), n_post, summary.loc["cumulative", "rel_effect"])
  by_horizon = (None, None)
  if placebo is not None and placebo.horizons is not None:
    by_horizon = _placebo_horizon_frames(
        record.placebo, origins, placebo_horizons, alpha, base["observed"],
        posterior_processing.model_index(ci_data), n_post, summary.loc["cumulative", "rel_effect"])
  joint = (None, None, None)
  if joint_bands:
    joint = _joint_frames(record.windows, request.path_ranks, num_draws, alpha, base["observed"],
                          posterior_processing.model_index(ci_data), ci_data.data.index,
                          [w.name for w in windows] if windows else None)
  return CausalImpactAnalysis(series, summary, posterior, samples.get("diagnostics"), components,
                              coefficients, prediction_errors, fit_quality, window_summary,
                              placebo_frame, placebo_quality, *joint, *by_horizon)


OUTCOME_LINKS = {None: _native.LINK_IDENTITY, "log": _native.LINK_LOG, "log1p": _native.LINK_LOG1P}
_LINK_PLACEBO_REFUSAL = ("`placebo=` is not available with `outcome_link`: the placebo forecasts are "
                         "Gaussian on the transformed scale, and a sum of lognormals has no closed-form "
                         "variance; `placebo=Placebo(simulate=True)` runs the simulated placebo instead, "
                         "whose band and p-value come from one simulated path of every window per draw")


def resolve_outcome_link(outcome_link) -> int:
  """`outcome_link` (None, "log", "log1p") as the `_native.LINK_*` it stands for; ValueError else."""
  try:
    return OUTCOME_LINKS[outcome_link]
  except (KeyError, TypeError):
    raise ValueError(f"`outcome_link` must be None, 'log' or 'log1p', got {outcome_link!r}") from None


def link_outcome(data, pre_period, post_period, outcome_column, link: int, series=None) -> pd.DataFrame:
  """The model's copy of `data` under an outcome link: the outcome column alone as log y (LINK_LOG)
  or log1p y (LINK_LOG1P), the covariates untouched.  The rows the model conditions on -- those of the
  pre-period -- must lie in the domain (y > 0, y > -1; a missing value stays missing): ValueError
  naming the first offending label, and `series` where given.  A row the model never reads with a
  value outside the domain becomes NaN, in this copy only.  No device is touched."""
  frame = pd.DataFrame(data).copy()
  column = frame.columns[0] if outcome_column is None else outcome_column
  if column not in frame.columns:
    raise KeyError(f"Specified `outcome_column` ({column}) not found in data")
  pre, _ = indices.parse_and_validate_date_data(data=frame, pre_period=pre_period, post_period=post_period)
  frame[column] = link_column(frame[column].to_numpy(dtype=np.float64), frame.index, pre, link, column, series)
  return frame


def link_column(y: np.ndarray, index: pd.Index, pre_period, link: int, column="y", series=None) -> np.ndarray:
  """`link_outcome` on the outcome values alone, `pre_period` parsed already: y [T_all], or [B, T_all]
  for series that share `index`, `series` then their names."""
  low = 0.0 if link == _native.LINK_LOG else -1.0
  outside = ~np.isnan(y) & ~(y > low)
  conditioned = np.asarray((index >= pre_period[0]) & (index <= pre_period[1]))
  bad = np.argwhere(outside & conditioned)             # (row-major: the first series, its first label)
  if bad.size:
    at = tuple(bad[0])
    name = "log" if link == _native.LINK_LOG else "log1p"
    who = series if y.ndim == 1 else series[at[0]]
    where = "" if who is None else f" of series {who!r}"
    raise ValueError(f"outcome_link={name!r} needs {column!r} > {low:g} on every row the model conditions on: "
                     f"row {index[at[-1]]}{where} holds {float(y[at])!r}")
  y = np.where(outside, np.nan, y)
  with np.errstate(invalid="ignore", divide="ignore"):
    return np.log(y) if link == _native.LINK_LOG else np.log1p(y)


def _data_scale_view(ci_data, raw_data):
  """`ci_data` (of the model's copy under an outcome link) as the frames of the effect read it: the
  raw outcome column in `data`, `pre_data` and `after_pre_data`, and nothing left to unstandardise --
  the linked values are on the data scale already.  The model's own arrays stay where they are."""
  view = copy.copy(ci_data)
  raw = pd.DataFrame(raw_data)
  data = ci_data.data.copy()
  data[ci_data.outcome_column] = raw[ci_data.outcome_column].reindex(data.index)
  idx = data.index
  view.data = data
  view.pre_data = data.loc[(idx >= ci_data.pre_period[0]) & (idx <= ci_data.pre_period[1])]
  view.after_pre_data = data.loc[idx > ci_data.pre_period[1]]
  view.standardize_data = False
  return view


@dataclasses.dataclass(frozen=True)
class EffectWindow:
  """One resolved entry of `effect_windows`: its bounds as values of the index (aligned like
  `post_period`) and its model steps first .. first + count - 1."""
  name: Any
  start: Any
  end: Any
  first: int
  count: int


def _window_items(effect_windows):
  """[(name, (lower, upper))] of an `effect_windows` argument; ValueError with the window named."""
  if not hasattr(effect_windows, "items"):
    raise ValueError("`effect_windows` must be a mapping {name: (start, end)}")
  items = list(effect_windows.items())
  if not items:
    raise ValueError("`effect_windows` is empty")
  for name, bounds in items:
    if isinstance(bounds, str) or not hasattr(bounds, "__len__") or len(bounds) != 2:
      raise ValueError(f"effect window {name!r}: expected (start, end), got {bounds!r}")
  return items


def resolve_windows(effect_windows, index: pd.Index, model_idx: pd.Index, post_period) -> List[EffectWindow]:
  """The `effect_windows` of a fit on `index` as `EffectWindow`s over the model steps `model_idx`
  (`posterior_processing.model_index`).  The bounds are converted and aligned exactly as `post_period`
  is (`indices`: a string is a date, an integer a POSITION into the index, a bound between two index
  values shrinks the window).  ValueError naming the window for bounds that cannot be read, a window
  that leaves the (aligned) post-period, or one without a model row.  The post-period is a contiguous
  run of model steps, hence so is every window."""
  out = []
  for name, bounds in _window_items(effect_windows):
    try:
      start, end = indices._align(                               # pylint: disable=protected-access
          tuple(indices._to_index_value(v, index) for v in bounds), index)   # pylint: disable=protected-access
    except (ValueError, IndexError, TypeError) as e:
      raise ValueError(f"effect window {name!r}: {e}") from e
    if start < post_period[0] or end > post_period[1]:
      raise ValueError(f"effect window {name!r}: ({start}, {end}) leaves the post-period "
                       f"({post_period[0]}, {post_period[1]})")
    steps = np.flatnonzero(np.asarray((model_idx >= start) & (model_idx <= end)))
    if steps.size == 0:
      raise ValueError(f"effect window {name!r}: ({start}, {end}) contains no row of the data")
    out.append(EffectWindow(name, start, end, int(steps[0]), int(steps.size)))
  return out


def _window_tables(windows: Sequence[EffectWindow], table_of) -> Optional[pd.DataFrame]:
  """`window_summary` of one fit: table_of(position, window) -> the 2 x 15 frame of that window."""
  if not windows:
    return None
  return pd.concat([table_of(w, win) for w, win in enumerate(windows)],
                   keys=[win.name for win in windows], names=["window", None])


def _component_summary_host(level, seasonal_levels, weights, X, scale, shift, ranks) -> Dict:
  """The component summary of one series in numpy, from pooled draws: level [N, T],
  seasonal_levels [N, T, K], weights [N, P] (or None), X [T, P].  The definitions of
  ci_session_summarize_components (include/causalimpact_amd.h), in float64:
    trend = level * scale + shift; seasonal_k = seasonal_levels[..., k] * scale;
    regression = (sum over j ascending of X[:, j] * weights[:, j]) * scale;
  per component and step the mean over the draws and the order statistics `ranks`; per design
  column the share of non-zero weights, their mean and their order statistics.  Arrays are laid out
  as the device returns them for one series: *_mean [T], *_order [R, T], seasonal_mean [K, T],
  seasonal_order [K, R, T], inclusion_prob / weight_mean [P], weight_order [R, P]."""
  scale, shift = np.float64(scale), np.float64(shift)
  ranks = list(ranks)

  def stats(m):                       # [N, T] -> mean [T], order [R, T]
    return m.mean(axis=0), np.sort(m, axis=0)[ranks]

  out = {}
  out["trend_mean"], out["trend_order"] = stats(np.asarray(level, np.float64) * scale + shift)
  seasonal = np.asarray(seasonal_levels, np.float64)
  if seasonal.ndim == 3 and seasonal.shape[-1] > 0:
    per = [stats(seasonal[:, :, k] * scale) for k in range(seasonal.shape[-1])]
    out["seasonal_mean"] = np.stack([m for m, _ in per])
    out["seasonal_order"] = np.stack([o for _, o in per])
  if weights is not None and np.shape(weights)[-1] > 0:
    w, X = np.asarray(weights, np.float64), np.asarray(X, np.float64)
    acc = np.zeros((w.shape[0], X.shape[0]))
    for j in range(w.shape[1]):
      acc += w[:, j, None] * X[None, :, j]
    out["regression_mean"], out["regression_order"] = stats(acc * scale)
    out["inclusion_prob"] = np.count_nonzero(w, axis=0) / w.shape[0]
    out["weight_mean"], out["weight_order"] = stats(w)
  return out


def _component_frames(csum: Dict, ranks, num_draws: int, alpha: float, model_idx: pd.Index,
                      full_idx: pd.Index, design_columns):
  """(components, coefficients) frames from the component summary of one series (device or host:
  the layout of `_component_summary_host`).  `components` is indexed like the `series` frame --
  `full_idx`, NaN on the rows before the pre-period, which the model never sees; `coefficients`
  by the design columns' names (None without covariates)."""
  rank_pos = {r: i for i, r in enumerate(ranks)}
  (lo_a, hi_a, g_a), (lo_b, hi_b, g_b) = _quantile_ranks(num_draws, (alpha / 2.0, 1.0 - alpha / 2.0))

  def band(order):                    # [R, X] -> lower, upper
    by_rank = {r: order[rank_pos[r]] for r in (lo_a, hi_a, lo_b, hi_b)}
    return _lerp_order_stats(by_rank, lo_a, hi_a, g_a), _lerp_order_stats(by_rank, lo_b, hi_b, g_b)

  cols = {}

  def add(name, mean, order):
    cols[name] = np.asarray(mean, np.float64)
    cols[name + "_lower"], cols[name + "_upper"] = band(order)

  add("trend", csum["trend_mean"], csum["trend_order"])
  if "seasonal_mean" in csum:
    for k in range(csum["seasonal_mean"].shape[0]):
      add(f"seasonal_{k}", csum["seasonal_mean"][k], csum["seasonal_order"][k])
  if "regression_mean" in csum:
    add("regression", csum["regression_mean"], csum["regression_order"])
  components = pd.DataFrame(cols, index=model_idx)
  if not model_idx.equals(full_idx):
    components = components.reindex(full_idx, fill_value=np.nan)
  coefficients = None
  if "weight_mean" in csum and design_columns is not None:
    lower, upper = band(csum["weight_order"])
    coefficients = pd.DataFrame(
        {"inclusion_probability": np.asarray(csum["inclusion_prob"], np.float64),
         "mean": np.asarray(csum["weight_mean"], np.float64), "lower": lower, "upper": upper},
        index=pd.Index(list(design_columns)))
  return components, coefficients


# the most state components the prediction-error filter takes (== CI_MAX_D of the oracle)
PREDICTION_MAX_STATE = 64
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def prediction_state_dim(has_slope: bool, num_seasons: Sequence[int]) -> int:
  """State components of the model: level, [slope], n - 1 effects per seasonal block."""
  return 1 + int(bool(has_slope)) + sum(int(n) - 1 for n in num_seasons)


def check_prediction_state(local_linear_trend: bool, seasons: Sequence) -> int:
  """The state dimension of ModelOptions(local_linear_trend, seasons); ValueError when it is more
  than the prediction-error filter takes (raised before anything is fitted)."""
  d = prediction_state_dim(local_linear_trend, [
      int(getattr(s, "num_seasons", s[0] if isinstance(s, (tuple, list)) else s)) for s in seasons])
  if d > PREDICTION_MAX_STATE:
    raise ValueError(f"InferenceOptions(prediction_errors=True) takes a state of at most "
                     f"{PREDICTION_MAX_STATE} components, this model has {d}")
  return d


def device_predictions_supported(num_seasons: Sequence[int]) -> bool:
  """The block lists ci_session_summarize_predictions takes: none, or one block of 2 to 7 seasons."""
  return len(num_seasons) == 0 or (len(num_seasons) == 1 and 2 <= int(num_seasons[0]) <= 7)


def device_block_predictions_supported(has_slope: bool, num_seasons: Sequence[int]) -> bool:
  """The models ci_session_summarize_predictions_blocks and ci_session_summarize_placebo_blocks take:
  any block list whose state has at most `PREDICTION_MAX_STATE` components."""
  return (all(int(n) >= 2 for n in num_seasons)
          and prediction_state_dim(has_slope, num_seasons) <= PREDICTION_MAX_STATE)


def _prediction_summary_host(y, mask, X, season_change, num_seasons, has_slope, params, draws,
                             scale, shift, ranks) -> Dict:
  """The prediction-error summary of one series in numpy, from the pooled PARAMETER draws alone:
  for every draw the Kalman filter of that draw's model over the observed series -- the definitions
  of ci_session_summarize_predictions (include/causalimpact_amd.h) in float64, for any block list.
  Vectorised over the draws, a loop over time, a dense d x d recursion.
    y, mask [T]: the outcome the sampler saw and its missing flags (y is not read where masked);
    X [T, P] or None; season_change [K, T]; num_seasons [K]; params: the series' parameter dict
    (`_model.series_params`: init_level_loc, init_level_scale, init_slope_scale, init_seasonal_scale);
    draws: observation_noise_scale, level_scale, slope_scale [N], seasonal_drift_scales [N, K],
    weights [N, P], all in the sampler's units; scale, shift: the map to the data scale.
  Returns forecast_mean [T], forecast_order [R, T], variance_mean [T], pit_mean [T] (0 where
  masked) and loglik [N], as the device returns them for one series."""
  y = np.asarray(y, np.float64)
  mask = np.asarray(mask, bool)
  T = y.shape[0]
  scale, shift = np.float64(scale), np.float64(shift)
  num_seasons = [int(n) for n in num_seasons]
  K, hs = len(num_seasons), int(bool(has_slope))
  d = prediction_state_dim(hs, num_seasons)
  if d > PREDICTION_MAX_STATE:
    raise ValueError(f"prediction errors take a state of at most {PREDICTION_MAX_STATE} components, "
                     f"this model has {d}")
  sc = np.asarray(season_change, np.uint8).reshape(K, T) if K else np.zeros((0, T), np.uint8)
  so = np.asarray(draws["observation_noise_scale"], np.float64).reshape(-1)
  N = so.shape[0]
  H = so * so
  sl = np.asarray(draws["level_scale"], np.float64).reshape(N)
  ss = np.asarray(draws["slope_scale"], np.float64).reshape(N) if hs else None
  sd = np.asarray(draws["seasonal_drift_scales"], np.float64).reshape(N, -1) if K else None
  reg = np.zeros((N, T))
  w = draws.get("weights")
  if X is not None and w is not None and np.shape(w)[-1] > 0:
    w, X = np.asarray(w, np.float64).reshape(N, -1), np.asarray(X, np.float64)
    for j in range(w.shape[1]):
      reg += w[:, j, None] * X[None, :, j]
  offsets = np.cumsum([1 + hs] + [n - 1 for n in num_seasons])[:-1] if K else []
  Z = np.zeros(d)
  Z[0] = 1.0
  for o in offsets:
    Z[o] = 1.0
  a = np.zeros((N, d))
  a[:, 0] = float(params["init_level_loc"])
  P = np.zeros((N, d, d))
  P[:, 0, 0] = float(params["init_level_scale"]) ** 2
  if hs:
    P[:, 1, 1] = float(params["init_slope_scale"]) ** 2
  for o, n in zip(offsets, num_seasons):
    P[:, o:o + n - 1, o:o + n - 1] = float(params["init_seasonal_scale"]) ** 2 * (np.eye(n - 1) - 1.0 / n)
  forecast, variance, pit = np.zeros((N, T)), np.zeros((N, T)), np.zeros((N, T))
  loglik = np.zeros(N)
  for t in range(T):
    pz = P @ Z                                      # [N, d]
    F = pz @ Z + H
    f = a @ Z + reg[:, t]
    forecast[:, t] = f * scale + shift
    variance[:, t] = (F * scale) * scale
    if not mask[t]:
      v = y[t] - f
      pit[:, t] = 0.5 * _erfc(-v / np.sqrt(2.0 * F))
      loglik += -0.5 * (math.log(2.0 * math.pi) + np.log(F) + v * v / F)
      a = a + (pz / F[:, None]) * v[:, None]
      P = P - pz[:, :, None] * pz[:, None, :] / F[:, None, None]
    if t + 1 < T:
      Tm = np.eye(d)
      if hs:
        Tm[0, 1] = 1.0
      Q = np.zeros((N, d, d))
      Q[:, 0, 0] = sl * sl
      if hs:
        Q[:, 1, 1] = ss * ss
      for k, (o, n) in enumerate(zip(offsets, num_seasons)):
        if sc[k, t]:
          blk = np.zeros((n - 1, n - 1))
          blk[:-1, 1:] = np.eye(n - 2)
          blk[-1, :] = -1.0
          Tm[o:o + n - 1, o:o + n - 1] = blk
          q = sd[:, k] / n
          Q[:, o:o + n - 1, o:o + n - 1] = (q * q)[:, None, None]
      a = a @ Tm.T
      P = Tm @ P @ Tm.T + Q
  ranks = list(ranks)
  return dict(forecast_mean=forecast.mean(axis=0), forecast_order=np.sort(forecast, axis=0)[ranks],
              variance_mean=variance.mean(axis=0), pit_mean=pit.mean(axis=0), loglik=loglik)


PREDICTION_COLUMNS = ("forecast", "forecast_lower", "forecast_upper", "forecast_sd", "error",
                      "standardized_error", "pit")
FIT_QUALITY_ENTRIES = ("n_scored", "rmse", "mae", "mase", "coverage", "loglik_mean", "loglik_sd")


def _prediction_columns(psum: Dict, ranks, alpha: float, observed, conditioned) -> Dict[str, np.ndarray]:
  """The `PREDICTION_COLUMNS` over the model's steps from the prediction summary of one series
  (device or host: the layout of `_prediction_summary_host`).  observed [T]: the outcome on the data
  scale (NaN: none); conditioned [T] bool: the steps whose observation the model conditions on.
  error, standardized_error and pit are NaN on every other step."""
  num_draws = np.shape(psum["loglik"])[-1]
  rank_pos = {r: i for i, r in enumerate(ranks)}
  (lo_a, hi_a, g_a), (lo_b, hi_b, g_b) = _quantile_ranks(num_draws, (alpha / 2.0, 1.0 - alpha / 2.0))
  order = np.asarray(psum["forecast_order"], np.float64)
  by_rank = {r: order[rank_pos[r]] for r in (lo_a, hi_a, lo_b, hi_b)}
  observed = np.asarray(observed, np.float64)
  conditioned = np.asarray(conditioned, bool) & ~np.isnan(observed)
  forecast = np.asarray(psum["forecast_mean"], np.float64)
  with np.errstate(invalid="ignore", divide="ignore"):
    sd = np.sqrt(np.asarray(psum["variance_mean"], np.float64))
    error = np.where(conditioned, observed - forecast, np.nan)
    return {
        "forecast": forecast,
        "forecast_lower": _lerp_order_stats(by_rank, lo_a, hi_a, g_a),
        "forecast_upper": _lerp_order_stats(by_rank, lo_b, hi_b, g_b),
        "forecast_sd": sd,
        "error": error,
        "standardized_error": error / sd,
        "pit": np.where(conditioned, np.asarray(psum["pit_mean"], np.float64), np.nan)}


def _fit_quality(cols: Dict[str, np.ndarray], loglik, alpha: float, observed, state_dim: int) -> pd.Series:
  """The `FIT_QUALITY_ENTRIES` of one series from its `_prediction_columns`, the per-draw
  log-likelihoods and the data-scale outcome: over the SCORED steps, those the model conditions on
  (error is not NaN) from step `state_dim` on -- the earlier ones only measure the initial prior."""
  observed = np.asarray(observed, np.float64)
  scored = ~np.isnan(cols["error"])
  scored[:state_dim] = False
  e, pit = cols["error"][scored], cols["pit"][scored]
  # the random walk's error at the scored steps whose predecessor is observed
  prev_ok = np.concatenate([[False], ~np.isnan(observed[:-1])])
  naive = np.abs(np.diff(observed, prepend=np.nan))[scored & prev_ok]
  ll = np.asarray(loglik, np.float64)
  with np.errstate(invalid="ignore", divide="ignore"):
    mae = np.mean(np.abs(e)) if e.size else np.nan
    return pd.Series({
        "n_scored": float(e.size),
        "rmse": np.sqrt(np.mean(e * e)) if e.size else np.nan,
        "mae": mae,
        "mase": mae / np.mean(naive) if naive.size else np.nan,
        "coverage": np.mean((pit >= alpha / 2.0) & (pit <= 1.0 - alpha / 2.0)) if e.size else np.nan,
        "loglik_mean": np.mean(ll),
        "loglik_sd": np.std(ll, ddof=1) if ll.size > 1 else np.nan}, name="fit_quality")


def _prediction_frames(psum: Dict, ranks, alpha: float, observed, conditioned, state_dim: int,
                       model_idx: pd.Index, full_idx: pd.Index):
  """(prediction_errors, fit_quality) of one series: `_prediction_columns` indexed like the `series`
  frame -- `full_idx`, NaN on the rows the model never sees -- and `_fit_quality`."""
  cols = _prediction_columns(psum, ranks, alpha, observed, conditioned)
  frame = pd.DataFrame(cols, index=model_idx)
  if not model_idx.equals(full_idx):
    frame = frame.reindex(full_idx, fill_value=np.nan)
  return frame, _fit_quality(cols, psum["loglik"], alpha, observed, state_dim)


@dataclasses.dataclass(frozen=True)
class Placebo:
  """Options of the placebo (A/A) check, `placebo=` of the three fit functions.
    horizon      steps every placebo window forecasts; None: min(n_post, n_pre // 3) of the series
                 (the post-period's own length wherever the pre-period is three times as long);
    max_origins  the most origins per series, spread evenly over the admissible ones;
    min_history  the first admissible origin (steps of history before it); None: max(horizon,
                 state dimension + 1);
    simulate     False (the default): the exact Gaussian moments of every window's sum.  True: the
                 SIMULATED placebo -- for every posterior draw one path of the window is drawn from
                 that draw's predictive, the outcome link applied step by step and the values summed;
                 band, `p` and `significant` come from the N simulated totals, and the frame gains
                 `predicted_lower` / `predicted_upper`.  The only placebo under `outcome_link`, where
                 a window's total has no closed-form distribution; under the identity an independent
                 check of the analytic one.  The Monte-Carlo floor of `p` is 1 / (N + 1).
    pool         False (the default).  True, with `simulate=True` and `aggregates=` /
                 `event_aggregates=` of the batch and panel fits only: the SIMULATED POOLED placebo
                 next to the per-series one -- every member's simulated totals at the group's origins
                 and horizon, added draw by draw with the group's weights; `result.aggregates[name]`
                 gets `placebo` and `placebo_quality` from the N pooled totals.  The members' paths are
                 drawn independently of each other: the assumption a pooled band rests on, and the one
                 this check tests.  The only pooled placebo under `outcome_link`.
    horizons     None (the default: nothing more runs, no result or bit differs).  Else the check at
                 SEVERAL horizons h <= H (H: the horizon above) from the SAME origins -- those of the plan
                 at H, so that the rows are comparable -- in one pass of the filter
                 (ci_session_summarize_placebo_horizons): the result gains `placebo_by_horizon` and
                 `placebo_profile`, the batch and panel results `placebo_profile`.  An int k >= 2: k
                 horizons spread over 1..H, unique(max(1, (H i) // k)), i = 1..k; a sequence of ints:
                 these horizons, each >= 1 and <= H (sorted, duplicates dropped; a panel's series keeps
                 those <= its own H).  H is always the last one; at most `MAX_PLACEBO_HORIZONS` (64)
                 remain.  Not with `simulate=True` (hence not under `outcome_link`).  With
                 `aggregates=` / `event_aggregates=` the pooled effects get the same two tables
                 (`result.aggregates[name].placebo_by_horizon`, `.placebo_profile`) and the result
                 `aggregate_placebo_profile`; a panel's group keeps the listed horizons <= its H_g.
  Fixed-parameter: every draw's scales and weights are those of the one fit of the whole pre-period,
  so the check is cheap and somewhat optimistic; the windows overlap, so the origins are not
  independent trials."""
  horizon: Optional[int] = None
  max_origins: int = 32
  min_history: Optional[int] = None
  simulate: bool = False
  pool: bool = False
  horizons: Any = None

  def __post_init__(self):
    if self.horizons is not None:
      hs = self.horizons
      if isinstance(hs, (bool, np.bool_)):
        raise TypeError(f"Placebo.horizons must be None, an int >= 2 or a sequence of ints, got {hs!r}")
      if isinstance(hs, (int, np.integer)):
        if int(hs) < 2:
          raise ValueError(f"Placebo.horizons as a number of horizons must be at least 2, got {hs}")
        if int(hs) > MAX_PLACEBO_HORIZONS:
          raise ValueError(f"Placebo.horizons: at most {MAX_PLACEBO_HORIZONS} horizons, got {hs}")
        object.__setattr__(self, "horizons", int(hs))
      else:
        try:
          listed = [h for h in hs]
        except TypeError:
          raise TypeError(f"Placebo.horizons must be None, an int >= 2 or a sequence of ints, got {hs!r}") from None
        if not listed or any(isinstance(h, (bool, np.bool_)) or not isinstance(h, (int, np.integer)) for h in listed):
          raise TypeError(f"Placebo.horizons must list ints (at least one), got {hs!r}")
        if min(listed) < 1:
          raise ValueError(f"Placebo.horizons must be at least 1 each, got {min(listed)}")
        listed = tuple(sorted({int(h) for h in listed}))
        if len(listed) > MAX_PLACEBO_HORIZONS:
          raise ValueError(f"Placebo.horizons: at most {MAX_PLACEBO_HORIZONS} horizons, got {len(listed)}")
        object.__setattr__(self, "horizons", listed)
      if self.simulate:
        raise ValueError("Placebo.horizons is not available with `simulate=True` (hence not under `outcome_link`): "
                         "the several-horizons table reads the analytic forecast's running moments, and a "
                         "simulated path is drawn for one horizon")
    if not isinstance(self.simulate, (bool, np.bool_)):
      raise TypeError(f"Placebo.simulate must be True or False, got {self.simulate!r}")
    if not isinstance(self.pool, (bool, np.bool_)):
      raise TypeError(f"Placebo.pool must be True or False, got {self.pool!r}")
    if self.pool and not self.simulate:
      raise ValueError("Placebo(pool=True) is the SIMULATED pooled placebo and needs `simulate=True`; the analytic "
                       "pooled placebo runs with `Placebo()` wherever aggregates are asked for")
    if self.horizon is not None and int(self.horizon) < 1:
      raise ValueError(f"Placebo.horizon must be at least 1, got {self.horizon}")
    if int(self.max_origins) < 1:
      raise ValueError(f"Placebo.max_origins must be at least 1, got {self.max_origins}")
    if self.min_history is not None and int(self.min_history) < 0:
      raise ValueError(f"Placebo.min_history must not be negative, got {self.min_history}")


def resolve_placebo(placebo) -> Optional[Placebo]:
  """`placebo=` as given -> None (off), or the `Placebo` to run (True: the defaults)."""
  if placebo is None or placebo is False:
    return None
  if placebo is True:
    return Placebo()
  if isinstance(placebo, Placebo):
    return placebo
  raise TypeError(f"`placebo` must be None, True or a Placebo, got {placebo!r}")


def check_link_placebo(link: int, placebo) -> None:
  """`placebo=` under an outcome link runs only as the simulated placebo: ValueError
  (`_LINK_PLACEBO_REFUSAL`) for True or a `Placebo` without `simulate`, before anything is fitted."""
  if link and placebo is not None and placebo is not False and not (
      isinstance(placebo, Placebo) and placebo.simulate):
    raise ValueError(_LINK_PLACEBO_REFUSAL)


def check_simulated_placebo_pool(placebo: Optional[Placebo], argument: Optional[str],
                                 wanted: str = "aggregates") -> None:
  """The simulated placebo pools only where it is asked to: ValueError naming `argument` ("aggregates",
  "event_aggregates"; None: no pooled effects were asked for) for `Placebo(simulate=True)` without
  `pool=True` together with pooled effects, and naming `wanted` for `pool=True` without any, before
  anything is fitted."""
  if placebo is None:
    return
  if placebo.pool and argument is None:
    raise ValueError(f"`Placebo(pool=True)` pools the simulated placebo forecasts over `{wanted}`, and none "
                     "were asked for")
  if placebo.simulate and not placebo.pool and argument is not None:
    raise ValueError(f"`{argument}` cannot be combined with `Placebo(simulate=True)`: the pooled placebo "
                     "forecasts add the members' exact Gaussian moments, and a simulated pooled placebo is "
                     "asked for with `Placebo(simulate=True, pool=True)`; use that, or `Placebo()` (without "
                     "`outcome_link`) for the analytic pooled check")


def check_single_fit_placebo(placebo) -> None:
  """`fit_causalimpact` has no pooled effects: ValueError for `Placebo(pool=True)`, before anything is
  fitted."""
  if isinstance(placebo, Placebo) and placebo.pool:
    raise ValueError("`Placebo(pool=True)` is not available on `fit_causalimpact`: it pools over the `aggregates` "
                     "of `fit_causalimpact_batch` or the `event_aggregates` of `fit_causalimpact_panel`")


def placebo_horizon(placebo: Placebo, n_pre: int, n_post: int) -> int:
  """Steps every placebo window of a series forecasts: the option, else min(n_post, n_pre // 3)."""
  return int(placebo.horizon) if placebo.horizon is not None else min(int(n_post), int(n_pre) // 3)


def placebo_min_history(placebo: Placebo, horizon: int, state_dim: int) -> int:
  """The first admissible origin: the option, else max(horizon, state_dim + 1)."""
  return int(placebo.min_history) if placebo.min_history is not None else max(int(horizon), int(state_dim) + 1)


def placebo_origins(n_pre: int, horizon: int, min_history: int, max_origins: int) -> np.ndarray:
  """The origins (model steps, strictly ascending) of a series with `n_pre` pre-period steps:
  lo = min_history, hi = n_pre - horizon, m = min(max_origins, hi - lo + 1) of them at
  lo + ((hi - lo) i) // (m - 1); the single origin of m = 1 is hi; none (an empty array) when
  hi < lo or the horizon is below 1."""
  lo, hi = int(min_history), int(n_pre) - int(horizon)
  if hi < lo or horizon < 1:
    return np.zeros(0, np.int32)
  m = min(int(max_origins), hi - lo + 1)
  if m == 1:
    return np.array([hi], np.int32)
  return np.array([lo + ((hi - lo) * i) // (m - 1) for i in range(m)], np.int32)


def placebo_plan(placebo: Placebo, n_pre: int, n_post: int, state_dim: int):
  """(horizon, origins) of one series: `placebo_horizon`, `placebo_min_history`, `placebo_origins`."""
  horizon = placebo_horizon(placebo, n_pre, n_post)
  return horizon, placebo_origins(n_pre, horizon, placebo_min_history(placebo, horizon, state_dim),
                                  placebo.max_origins)


MAX_PLACEBO_HORIZONS = _native.MAX_PLACEBO_HORIZONS


def placebo_horizon_list(placebo: Placebo, horizon: int, strict: bool = True) -> Optional[np.ndarray]:
  """The horizons [K] (ascending, int32, the last one `horizon` = H) of `Placebo.horizons` for a series
  whose plan has the horizon H; None when the option is off or H < 1.  An int k: unique(max(1, (H i) //
  k)), i = 1..k.  A sequence: its entries (sorted, unique) -- one above H is a ValueError naming the
  option, or with strict off (a panel's series) dropped -- and H.  More than `MAX_PLACEBO_HORIZONS`:
  ValueError."""
  if placebo is None or placebo.horizons is None or int(horizon) < 1:
    return None
  H, hs = int(horizon), placebo.horizons
  if isinstance(hs, int):
    out = sorted({max(1, (H * i) // hs) for i in range(1, hs + 1)})
  else:
    if strict and hs[-1] > H:
      raise ValueError(f"Placebo.horizons: the horizon {hs[-1]} is beyond the placebo horizon {H} "
                       "(Placebo.horizon, else min(n_post, n_pre // 3)): every listed horizon must be <= it")
    out = sorted({h for h in hs if h <= H} | {H})
  if len(out) > MAX_PLACEBO_HORIZONS:
    raise ValueError(f"Placebo.horizons: at most {MAX_PLACEBO_HORIZONS} horizons, got {len(out)} with H = {H}")
  return np.array(out, np.int32)


def placebo_state_dim(local_linear_trend: bool, seasons: Sequence) -> int:
  """The state dimension of ModelOptions(local_linear_trend, seasons); ValueError when it is more than
  the placebo filter takes (raised before anything is fitted)."""
  d = prediction_state_dim(local_linear_trend, [
      int(getattr(s, "num_seasons", s[0] if isinstance(s, (tuple, list)) else s)) for s in seasons])
  if d > PREDICTION_MAX_STATE:
    raise ValueError(f"placebo forecasts take a state of at most {PREDICTION_MAX_STATE} components, "
                     f"this model has {d}")
  return d


class _PlaceboFilter:
  """The filter the placebo forecasts of one series start from, in numpy, from the pooled PARAMETER
  draws alone: that of `_prediction_summary_host` (whose arguments the first eight are), for any
  block list of up to `PREDICTION_MAX_STATE` state components.  origins [O]: steps, strictly ascending
  (-1: an unused slot, at the end); horizon: steps per window, origin + horizon <= T.  `at_origins`
  runs it and yields, at every used origin, (slot, t, a [N, d], P [N, d, d]): the predicted moments of
  x_t given y[0 .. t - 1], which the caller forecasts from and must not modify.  Z [d], H [N], reg
  [N, T], y, mask [T], `transition(t)` -> (T_t [d, d], Q_t [N, d, d]) of step t -> t + 1."""

  def __init__(self, y, mask, X, season_change, num_seasons, has_slope, params, draws, origins, horizon):
    self.y = y = np.asarray(y, np.float64)
    self.mask = np.asarray(mask, bool)
    self.T = T = y.shape[0]
    self.origins = origins = [int(o) for o in np.asarray(origins).reshape(-1)]
    self.Hn = Hn = int(horizon)
    self.used = used = [o for o in origins if o >= 0]
    if Hn < 1:
      raise ValueError(f"the placebo horizon must be at least 1, got {Hn}")
    if any(o < -1 for o in origins) or used != origins[:len(used)] or any(b <= a for a, b in zip(used, used[1:])):
      raise ValueError("placebo origins must be strictly ascending steps with the unused slots (-1) at the end")
    if used and used[-1] + Hn > T:
      raise ValueError(f"placebo origin {used[-1]} with horizon {Hn} reaches beyond the series' {T} steps")
    self.num_seasons = num_seasons = [int(n) for n in num_seasons]
    K, hs = len(num_seasons), int(bool(has_slope))
    self.hs = hs
    self.d = d = prediction_state_dim(hs, num_seasons)
    if d > PREDICTION_MAX_STATE:
      raise ValueError(f"placebo forecasts take a state of at most {PREDICTION_MAX_STATE} components, "
                       f"this model has {d}")
    self.sc = np.asarray(season_change, np.uint8).reshape(K, -1)[:, :T] if K else np.zeros((0, T), np.uint8)
    so = np.asarray(draws["observation_noise_scale"], np.float64).reshape(-1)
    self.N = N = so.shape[0]
    self.H = so * so
    self.sl = np.asarray(draws["level_scale"], np.float64).reshape(N)
    self.ss = np.asarray(draws["slope_scale"], np.float64).reshape(N) if hs else None
    self.sd = np.asarray(draws["seasonal_drift_scales"], np.float64).reshape(N, -1) if K else None
    self.reg = reg = np.zeros((N, T))
    w = draws.get("weights")
    if X is not None and w is not None and np.shape(w)[-1] > 0:
      w, X = np.asarray(w, np.float64).reshape(N, -1), np.asarray(X, np.float64)
      for j in range(w.shape[1]):
        reg += w[:, j, None] * X[None, :, j]
    self.offsets = offsets = np.cumsum([1 + hs] + [n - 1 for n in num_seasons])[:-1] if K else []
    self.Z = Z = np.zeros(d)
    Z[0] = 1.0
    for o in offsets:
      Z[o] = 1.0
    self.a0 = a = np.zeros((N, d))
    a[:, 0] = float(params["init_level_loc"])
    self.P0 = P = np.zeros((N, d, d))
    P[:, 0, 0] = float(params["init_level_scale"]) ** 2
    if hs:
      P[:, 1, 1] = float(params["init_slope_scale"]) ** 2
    for o, n in zip(offsets, num_seasons):
      P[:, o:o + n - 1, o:o + n - 1] = float(params["init_seasonal_scale"]) ** 2 * (np.eye(n - 1) - 1.0 / n)

  def transition(self, t):            # (T_t [d, d], Q_t [N, d, d]) of step t -> t + 1
    d, N, hs = self.d, self.N, self.hs
    Tm = np.eye(d)
    if hs:
      Tm[0, 1] = 1.0
    Q = np.zeros((N, d, d))
    Q[:, 0, 0] = self.sl * self.sl
    if hs:
      Q[:, 1, 1] = self.ss * self.ss
    for k, (o, n) in enumerate(zip(self.offsets, self.num_seasons)):
      if self.sc[k, t]:
        blk = np.zeros((n - 1, n - 1))
        blk[:-1, 1:] = np.eye(n - 2)
        blk[-1, :] = -1.0
        Tm[o:o + n - 1, o:o + n - 1] = blk
        q = self.sd[:, k] / n
        Q[:, o:o + n - 1, o:o + n - 1] = (q * q)[:, None, None]
    return Tm, Q

  def at_origins(self):
    a, P, Z, H, used = self.a0, self.P0, self.Z, self.H, self.used
    slot = 0
    for t in range(self.T):
      if slot >= len(used):
        break
      if t == used[slot]:
        yield slot, t, a, P
        slot += 1
        if slot >= len(used):
          break
      pz = P @ Z
      if not self.mask[t]:
        F = pz @ Z + H
        v = self.y[t] - (a @ Z + self.reg[:, t])
        a = a + (pz / F[:, None]) * v[:, None]
        P = P - pz[:, :, None] * pz[:, None, :] / F[:, None, None]
      if t + 1 < self.T:
        Tm, Q = self.transition(t)
        a = a @ Tm.T
        P = Tm @ P @ Tm.T + Q


def _placebo_summary_host(y, mask, X, season_change, num_seasons, has_slope, params, draws,
                          scale, shift, origins, horizon=None, per_draw: bool = False, horizons=None) -> Dict:
  """The placebo summary of one series in numpy, from the pooled PARAMETER draws alone: the
  definitions of ci_session_summarize_placebo (include/causalimpact_amd.h) in float64, for any block
  list of up to `PREDICTION_MAX_STATE` state components.  The arguments but the last three are those
  of `_prediction_summary_host`, whose filter this runs (`_PlaceboFilter`); origins [O]: steps,
  strictly ascending (-1: an unused slot, at the end); horizon: steps per window, origin + horizon <= T.
  Returns predicted_mean, spread_mean, pit_mean [O] (0 in an unused slot and where the window counts
  no observation), as the device returns them for one series; with `per_draw` also C, V [O, N] (the
  conditional mean and predictive variance of the counted sum, in the sampler's units), A and cnt [O].
  horizons [K] (ascending, -1: unused, at the end; `horizon` is then their last one, whatever is passed):
  the one forecast loop records its running values at the checkpoints h == horizons[k] and the three
  outputs are [O, K] -- column k what `horizon=horizons[k]` returns, bit for bit (0 in an unused slot);
  with `per_draw` also C, V [O, K, N], A and cnt [O, K] at the checkpoints (0 in an unused slot): what
  `per_draw` returns for `horizon=horizons[k]`."""
  if horizons is not None:
    hz = [int(h) for h in np.asarray(horizons).reshape(-1)]
    marks = [h for h in hz if h != -1]
    if (not marks or min(marks) < 1 or marks != hz[:len(marks)]
        or any(b <= a for a, b in zip(marks, marks[1:]))):
      raise ValueError("placebo horizons must be at least 1 and strictly ascending with the unused slots (-1) at "
                       "the end, at least one of them")
    horizon = marks[-1]
  flt = _PlaceboFilter(y, mask, X, season_change, num_seasons, has_slope, params, draws, origins, horizon)
  y, mask, reg, Z, H, N, d, Hn, transition = flt.y, flt.mask, flt.reg, flt.Z, flt.H, flt.N, flt.d, flt.Hn, flt.transition
  scale, shift = np.float64(scale), np.float64(shift)
  O = len(flt.origins)
  Cs, Vs, As, cnts = np.zeros((N, O)), np.zeros((N, O)), np.zeros(O), np.zeros(O)
  marks = [Hn] if horizons is None else marks
  # (one [N, O] matrix per checkpoint and output: the means below are taken as those of one horizon)
  sums, spreads, pits = ([np.zeros((N, O)) for _ in marks] for _ in range(3))
  Ck, Vk = np.zeros((O, len(marks), N)), np.zeros((O, len(marks), N))   # (per_draw with horizons)
  Ak, cntk = np.zeros((O, len(marks))), np.zeros((O, len(marks)))
  for slot, t, a, P in flt.at_origins():
    # the forecast branch, from the predicted moments
    fa, fP, r = a, P, np.zeros((N, d))
    V, C, A, cnt = np.zeros(N), np.zeros(N), np.float64(0.0), 0
    for h in range(Hn):
      u = t + h
      pz = fP @ Z
      if not mask[u]:
        C = C + (fa @ Z + reg[:, u])
        A = A + y[u]
        cnt += 1
        V = V + ((2.0 * (r @ Z) + pz @ Z) + H)
        r = r + pz
      if h + 1 in marks:
        k = marks.index(h + 1)
        Ck[slot, k], Vk[slot, k], Ak[slot, k], cntk[slot, k] = C, V, A, cnt
      if h + 1 in marks and cnt:
        k, e = marks.index(h + 1), A - C
        sums[k][:, slot] = C * scale + np.float64(cnt) * shift
        spreads[k][:, slot] = ((V + e * e) * scale) * scale
        pits[k][:, slot] = 0.5 * _erfc(-e / np.sqrt(2.0 * V))
      if h + 1 < Hn:
        Tm, Q = transition(u)
        fa, r = fa @ Tm.T, r @ Tm.T
        fP = Tm @ fP @ Tm.T + Q
    Cs[:, slot], Vs[:, slot], As[slot], cnts[slot] = C, V, A, cnt
  if horizons is not None:
    table = lambda mats: np.stack([m.mean(axis=0) for m in mats] + [np.zeros(O)] * (len(hz) - len(marks)), axis=1)   # pylint: disable=unnecessary-lambda-assignment
    out = dict(predicted_mean=table(sums), spread_mean=table(spreads), pit_mean=table(pits))
    if per_draw:
      pad = lambda x: np.concatenate([x, np.zeros((O, len(hz) - len(marks)) + x.shape[2:])], axis=1)   # pylint: disable=unnecessary-lambda-assignment
      out.update(C=pad(Ck), V=pad(Vk), A=pad(Ak), cnt=pad(cntk))
    return out
  out = dict(predicted_mean=sums[0].mean(axis=0), spread_mean=spreads[0].mean(axis=0), pit_mean=pits[0].mean(axis=0))
  if per_draw:
    out.update(C=Cs.T.copy(), V=Vs.T.copy(), A=As, cnt=cnts)
  return out


def placebo_stream(seed, series_id=None, chains=(0,)):
  """What addresses the random stream of a fit's simulated placebo forecasts: (key, chains) -- the
  Philox key the fit ran on (`_native.series_stream_key(seed, series_id)`; the seed itself for
  series_id None: a single fit, or shared streams) and the GLOBAL ids of the chains whose draws are
  pooled, in pooling order."""
  pair = tuple(int(v) & 0xFFFFFFFF for v in _native.seed_pair(seed))
  key = pair if series_id is None else _native.series_stream_key(pair, int(series_id))
  return key, tuple(int(c) for c in chains)


def _placebo_simulated_host(y, mask, X, season_change, num_seasons, has_slope, params, draws,
                            scale, shift, origins, horizon, link, stream, seen=None, ranks=()) -> Dict:
  """The SIMULATED placebo forecasts of one series in numpy, from the pooled PARAMETER draws alone:
  the definitions of ci_session_simulate_placebo (include/causalimpact_amd.h) in float64, for any block
  list of up to `PREDICTION_MAX_STATE` state components.  The arguments up to `horizon` are those of
  `_placebo_summary_host`, whose filter this runs (`_PlaceboFilter`); link: a `_native.LINK_*`;
  stream: (key, chains) of `placebo_stream` -- pooled draw n = c * S + s is kept draw s of chain
  chains[c], S = N / len(chains), so the result does not depend on how the chains were spread over
  devices; seen [O]: the observed totals on the data scale (None: no spread_mean, no below); ranks:
  the order statistics of total_order.  For every draw ONE path of the window: the filter's own step
  fed with v = sqrt(F) z, z = `_native.normals_host`(key, chain, s, SITE_PLACEBO_SIM, slot, h), the
  link applied step by step, the values summed.  Returns what the device returns for one series --
  predicted_mean, spread_mean, below [O], total_order [R, O], means as `_native.row_means_host` -- and
  totals [O, N], cnt [O]; everything 0 in an unused slot and where the window counts no observation."""
  flt = _PlaceboFilter(y, mask, X, season_change, num_seasons, has_slope, params, draws, origins, horizon)
  mask, reg, Z, H, N, Hn = flt.mask, flt.reg, flt.Z, flt.H, flt.N, flt.Hn
  scale, shift = np.float64(scale), np.float64(shift)
  key, chains = stream
  if not chains or N % len(chains):
    raise ValueError(f"{N} pooled draws are not a whole number of draws for each of {len(chains)} chains")
  kept = N // len(chains)
  chain_of = np.repeat(np.asarray(chains, np.uint64), kept)
  iter_of = np.tile(np.arange(kept, dtype=np.uint64), len(chains))
  O = len(flt.origins)
  totals, cnts = np.zeros((O, N)), np.zeros(O)
  for slot, t, a, P in flt.at_origins():
    z = _native.normals_host(key, chain_of[:, None], iter_of[:, None], _native.SITE_PLACEBO_SIM, slot,
                             np.arange(Hn, dtype=np.uint64)[None, :])                     # [N, H]
    fa, fP, S, cnt = a, P, np.zeros(N), 0
    for h in range(Hn):
      u = t + h
      pz = fP @ Z
      if not mask[u]:
        F = pz @ Z + H
        f = fa @ Z + reg[:, u]
        v = np.sqrt(F) * z[:, h]
        ysim = f + v
        with np.errstate(over="ignore"):
          S = S + _native.link_values_host(ysim * scale + shift, link)
        cnt += 1
        fa = fa + (pz / F[:, None]) * v[:, None]
        fP = fP - pz[:, :, None] * pz[:, None, :] / F[:, None, None]
      if h + 1 < Hn:
        Tm, Q = flt.transition(u)
        fa = fa @ Tm.T
        fP = Tm @ fP @ Tm.T + Q
    cnts[slot] = cnt
    if cnt:
      totals[slot] = S
  some = cnts > 0
  out = dict(predicted_mean=_native.row_means_host(totals), totals=totals, cnt=cnts,
             total_order=np.sort(totals, axis=1)[:, list(ranks)].T.copy())
  if seen is not None:
    seen = np.where(some, np.nan_to_num(np.asarray(seen, np.float64).reshape(O)), 0.0)
    out["below"] = np.where(some, np.count_nonzero(totals <= seen[:, None], axis=1), 0).astype(np.float64)
    dev = totals - seen[:, None]
    out["spread_mean"] = np.where(some, _native.row_means_host(dev * dev), 0.0)
  return out


def _placebo_seen(y_seen, mask, origins, horizon: int, scale, shift, horizons=None):
  """(n_counted [O], seen_sum [O]) of a series' placebo windows: the observed steps of every window
  and the sum over them of the outcome AS THE SAMPLER SAW IT (y_seen, in its number format and
  units), accumulated ascending in float64 and mapped to the data scale: A * scale + cnt * shift --
  the value every route's pit and spread are taken at.  0 and NaN for an unused slot (-1).
  horizons [K] (ascending, -1: unused, at the end; `horizon` at least their last one): both [O, K],
  the PREFIXES of the same running sums -- column k what `horizon=horizons[k]` returns, bit for bit;
  0 and NaN in an unused horizon slot."""
  y_seen = np.asarray(y_seen, np.float64)
  mask = np.asarray(mask, bool)
  origins = np.asarray(origins).reshape(-1)
  shape = (origins.size,) if horizons is None else (origins.size, np.size(horizons))
  n_counted, seen_sum = np.zeros(shape), np.full(shape, np.nan)
  used = origins >= 0
  if used.any():
    steps = origins[used].astype(np.int64)[:, None] + np.arange(int(horizon))[None, :]     # [O, H]
    seen = ~mask[steps]
    # (a masked step adds 0.0; cumsum adds left to right: the ascending sum)
    sums = np.cumsum(np.where(seen, y_seen[steps], 0.0), axis=1)
    if horizons is not None:
      hz = np.asarray(horizons).reshape(-1).astype(np.int64)
      at = np.flatnonzero(hz >= 1)                       # (every used slot at once: the counts are exact integers)
      cnt = np.cumsum(seen, axis=1)[:, hz[at] - 1].astype(np.float64)
      rows = np.flatnonzero(used)[:, None]
      n_counted[rows, at[None, :]] = cnt
      seen_sum[rows, at[None, :]] = sums[:, hz[at] - 1] * np.float64(scale) + cnt * np.float64(shift)
      return n_counted, seen_sum
    A = sums[:, -1]
    cnt = seen.sum(axis=1).astype(np.float64)
    n_counted[used], seen_sum[used] = cnt, A * np.float64(scale) + cnt * np.float64(shift)
  return n_counted, seen_sum


PLACEBO_COLUMNS = ("horizon_end", "n_counted", "actual", "predicted", "predicted_sd", "effect",
                   "relative_effect", "pit", "p", "significant")
# `Placebo(simulate=True)`: the alpha / 2 and 1 - alpha / 2 quantiles of the simulated totals, after them
PLACEBO_SIMULATED_COLUMNS = ("predicted_lower", "predicted_upper")
PLACEBO_QUALITY_ENTRIES = ("n_origins", "horizon", "false_positive_rate", "mean_relative_effect",
                           "mde_relative", "empirical_p")


def _placebo_quality(cols: Optional[Dict[str, np.ndarray]], horizon: int, alpha: float, n_post: int,
                     fit_relative_effect) -> pd.Series:
  """The `PLACEBO_QUALITY_ENTRIES` of one series from its placebo columns (None: a series without
  room for an origin -- NaN but n_origins 0 and the horizon), over the origins whose window counts
  an observation.  empirical_p = (1 + #{|placebo relative effect| >= |the fit's cumulative relative
  effect|}) / (1 + n_origins), NaN unless horizon == n_post."""
  nan = np.float64(np.nan)
  row = dict(n_origins=0.0, horizon=float(horizon), false_positive_rate=nan, mean_relative_effect=nan,
             mde_relative=nan, empirical_p=nan)
  if cols is not None:
    ok = np.asarray(cols["n_counted"]) > 0
    rel = np.asarray(cols["relative_effect"], np.float64)[ok]
    row["n_origins"] = float(rel.size)
    if rel.size:
      row["false_positive_rate"] = float(np.mean(np.asarray(cols["significant"], bool)[ok]))
      row["mean_relative_effect"] = float(np.mean(rel))
      row["mde_relative"] = float(np.quantile(np.abs(rel), 1.0 - alpha))
      fit_rel = np.float64(fit_relative_effect)
      if int(horizon) == int(n_post) and not np.isnan(fit_rel):
        row["empirical_p"] = float((1 + np.count_nonzero(np.abs(rel) >= abs(fit_rel))) / (1 + rel.size))
  return pd.Series(row, name="placebo_quality")


def _placebo_columns(psum: Dict, origins, horizon: int, alpha: float, observed) -> Dict[str, np.ndarray]:
  """The `PLACEBO_COLUMNS` but horizon_end (as the step horizon_end_step) over the USED origins of one
  series, from its placebo summary (device or host: predicted_mean, spread_mean, pit_mean, and
  n_counted, seen_sum of `_placebo_seen`, each [O]).  observed [T]: the outcome on the data scale.
  effect = seen_sum - predicted: the actual sum as the sampler saw it minus the forecast, the e of
  predicted_sd = sqrt(max(spread - e^2, 0)), so that the device and the host route agree."""
  origins = np.asarray(origins).reshape(-1)
  used = origins >= 0
  org = origins[used].astype(np.int64)
  observed = np.asarray(observed, np.float64)
  n_counted = np.asarray(psum["n_counted"], np.float64)[used]
  some = n_counted > 0
  nan = np.where(some, 0.0, np.nan)                  # NaN on the rows whose window counts nothing
  actual = np.array([np.nansum(observed[o:o + int(horizon)]) for o in org], np.float64) + nan
  predicted = np.asarray(psum["predicted_mean"], np.float64)[used] + nan
  effect = np.asarray(psum["seen_sum"], np.float64)[used] - predicted
  pit = np.asarray(psum["pit_mean"], np.float64)[used] + nan
  with np.errstate(invalid="ignore", divide="ignore"):
    sd = np.sqrt(np.maximum(np.asarray(psum["spread_mean"], np.float64)[used] - effect * effect, 0.0)) + nan
    return {
        "horizon_end_step": org + int(horizon) - 1,
        "n_counted": n_counted,
        "actual": actual,
        "predicted": predicted,
        "predicted_sd": sd,
        "effect": effect,
        "relative_effect": effect / predicted,
        "pit": pit,
        "p": 2.0 * np.minimum(pit, 1.0 - pit),
        "significant": some & ((pit < alpha / 2.0) | (pit > 1.0 - alpha / 2.0)),
        # (the simulated route only: the quantiles of the totals)
        **{k: np.asarray(psum[k], np.float64)[used] + nan for k in PLACEBO_SIMULATED_COLUMNS if k in psum}}


def _placebo_frames(psum: Optional[Dict], origins, horizon: int, alpha: float, observed,
                    model_idx: pd.Index, n_post: int, fit_relative_effect):
  """(placebo, placebo_quality) of one series: `_placebo_columns` indexed by the origins' labels on
  the model's index, and `_placebo_quality`.  psum None or no origin: an empty frame and the NaN row."""
  origins = np.asarray(origins).reshape(-1)
  if psum is None or not np.any(origins >= 0):
    frame = pd.DataFrame({k: np.zeros(0) for k in PLACEBO_COLUMNS}, index=model_idx[:0])
    return frame, _placebo_quality(None, horizon, alpha, n_post, fit_relative_effect)
  cols = _placebo_columns(psum, origins, horizon, alpha, observed)
  end = cols.pop("horizon_end_step")
  frame = pd.DataFrame({"horizon_end": model_idx[end], **cols}, index=model_idx[origins[origins >= 0]])
  frame.index.name = "origin"
  shown = list(PLACEBO_COLUMNS) + [k for k in PLACEBO_SIMULATED_COLUMNS if k in cols]
  return frame[shown], _placebo_quality(cols, horizon, alpha, n_post, fit_relative_effect)


# `placebo_profile`: the quality entries but the horizon (the index), and the model's own statement of
# the noise at that horizon
PLACEBO_PROFILE_COLUMNS = tuple(k for k in PLACEBO_QUALITY_ENTRIES if k != "horizon") + ("relative_sd",)


def _placebo_profile_row(cols: Optional[Dict[str, np.ndarray]], horizon: int, alpha: float, n_post: int,
                         fit_relative_effect) -> Dict[str, float]:
  """One row of `placebo_profile`: `_placebo_quality` on the columns of that horizon without its
  `horizon` entry (empirical_p hence on the row horizon == n_post alone), and relative_sd, the median
  over the counted origins of predicted_sd / |predicted|."""
  quality = _placebo_quality(cols, horizon, alpha, n_post, fit_relative_effect)
  row = {k: float(quality[k]) for k in PLACEBO_PROFILE_COLUMNS[:-1]}
  row["relative_sd"] = float("nan")
  if cols is not None:
    ok = np.asarray(cols["n_counted"]) > 0
    if ok.any():
      with np.errstate(invalid="ignore", divide="ignore"):
        row["relative_sd"] = float(np.median(np.asarray(cols["predicted_sd"])[ok] / np.abs(np.asarray(cols["predicted"])[ok])))
  return row


def _placebo_horizon_columns(psum: Dict, origins, horizons, alpha: float, observed):
  """[(h, `_placebo_columns` at h)] for the used horizons of one series, from the
  `PLACEBO_HORIZON_ARRAYS` [O, K] of its placebo summary: column k read as the summary of horizon
  horizons[k]."""
  out = []
  for k, h in enumerate(int(h) for h in np.asarray(horizons).reshape(-1)):
    if h >= 1:
      at = {name: np.asarray(psum["horizons_" + name])[:, k]
            for name in ("predicted_mean", "spread_mean", "pit_mean", "n_counted", "seen_sum")}
      out.append((h, _placebo_columns(at, origins, h, alpha, observed)))
  return out


def _placebo_horizon_frames(psum: Optional[Dict], origins, horizons, alpha: float, observed,
                            model_idx: pd.Index, n_post: int, fit_relative_effect):
  """(placebo_by_horizon, placebo_profile) of one series with `Placebo(horizons=...)`: the
  `PLACEBO_COLUMNS` indexed by (origin, horizon) -- the slice at a horizon is the `placebo` frame that
  horizon alone would give, from the same origins -- and the `PLACEBO_PROFILE_COLUMNS` indexed by
  horizon.  psum None, no origin or no horizon: empty frames."""
  origins = np.asarray(origins).reshape(-1)
  per = []
  if psum is not None and horizons is not None and np.any(origins >= 0):
    per = _placebo_horizon_columns(psum, origins, horizons, alpha, observed)
  if not per:
    index = pd.MultiIndex.from_arrays([model_idx[:0], np.zeros(0, np.int64)], names=["origin", "horizon"])
    return (pd.DataFrame({k: np.zeros(0) for k in PLACEBO_COLUMNS}, index=index),
            pd.DataFrame({k: np.zeros(0) for k in PLACEBO_PROFILE_COLUMNS}, index=pd.Index([], dtype=np.int64, name="horizon")))
  frames, rows = [], []
  for h, cols in per:
    rows.append(_placebo_profile_row(cols, h, alpha, n_post, fit_relative_effect))
    end = cols.pop("horizon_end_step")
    frame = pd.DataFrame({"horizon_end": model_idx[end], **cols}, index=model_idx[origins[origins >= 0]])
    frame.index.name = "origin"
    frames.append(frame[list(PLACEBO_COLUMNS)])
  by_horizon = pd.concat(frames, keys=[h for h, _ in per], names=["horizon", "origin"]).swaplevel().sort_index()
  profile = pd.DataFrame(rows, index=pd.Index([h for h, _ in per], dtype=np.int64, name="horizon"),
                         columns=list(PLACEBO_PROFILE_COLUMNS))
  return by_horizon, profile


def _aggregate_placebo_frames(psum: Optional[Dict], actual, columns, horizon: int, alpha: float,
                              labels: pd.Index, n_post: int, fit_relative_effect):
  """(placebo, placebo_quality) of one POOLED group (`aggregates=` / `event_aggregates=` with
  `placebo=`): `_placebo_frames` for the group's pooled sums.  psum: predicted_mean, spread_mean,
  pit_mean [O] of the pooled forecast (`_native.finish_placebo_host`, or the device's), n_counted the
  member-steps every window counts and seen_sum the weighted sum of the members' `_placebo_seen`;
  actual [O]: the weighted sum of the members' `actual`; columns [O]: the origins as positions into
  `labels`, the group's own axis (-1: unused).  A simulated summary (`_simulated_placebo_means` of the
  pooled totals: pit_mean from `below`, and predicted_lower, predicted_upper) gives the columns and the
  formulas of the per-series simulated frame.  The pooled forecast treats the members as independent
  given their draws: its band adds their predictive variances.  That is the assumption these frames
  test -- shocks common to the members show as a false-positive rate above alpha."""
  columns = np.asarray(columns).reshape(-1)
  used = columns >= 0
  if psum is None or not np.any(used):
    frame = pd.DataFrame({k: np.zeros(0) for k in PLACEBO_COLUMNS}, index=labels[:0])
    return frame, _placebo_quality(None, horizon, alpha, n_post, fit_relative_effect)
  frame, cols = _aggregate_placebo_frame(psum, actual, columns, horizon, alpha, labels)
  return frame, _placebo_quality(cols, horizon, alpha, n_post, fit_relative_effect)


def _aggregate_placebo_frame(psum: Dict, actual, columns, horizon: int, alpha: float, labels: pd.Index):
  """(frame, columns) of `_aggregate_placebo_frames` for a group with an origin: `_placebo_columns` of
  the pooled sums with the pooled `actual`, indexed by the origins' labels on the group's axis."""
  used = columns >= 0
  cols = _placebo_columns(psum, columns, horizon, alpha, np.zeros(len(labels)))
  cols["actual"] = np.asarray(actual, np.float64)[used] + np.where(cols["n_counted"] > 0, 0.0, np.nan)
  end = cols.pop("horizon_end_step")
  frame = pd.DataFrame({"horizon_end": labels[end], **cols}, index=labels[columns[used]])
  frame.index.name = "origin"
  shown = list(PLACEBO_COLUMNS) + [k for k in PLACEBO_SIMULATED_COLUMNS if k in cols]
  return frame[shown], cols


def _aggregate_placebo_horizon_frames(psum: Optional[Dict], actual, columns, horizons, alpha: float,
                                      labels: pd.Index, n_post: int, fit_relative_effect):
  """(placebo_by_horizon, placebo_profile) of one POOLED group with `Placebo(horizons=...)`:
  `_placebo_horizon_frames` for the group's pooled sums.  psum: predicted_mean, spread_mean, pit_mean,
  n_counted and seen_sum, each [O, K] -- column k what `_aggregate_placebo_frames` takes for the horizon
  horizons[k]; actual [O, K]; horizons [K] (-1: unused, at the end).  The slice of the first frame at a
  horizon is the `placebo` frame of that horizon alone; the profile's row at h is its quality without
  `horizon` (empirical_p on the row h == n_post, against the aggregate's own cumulative rel_effect) and
  relative_sd, the median over the counted origins of predicted_sd / |predicted|.  psum None, no origin
  or no horizon: empty frames."""
  columns = np.asarray(columns).reshape(-1)
  marks = [] if horizons is None else [(k, int(h)) for k, h in enumerate(np.asarray(horizons).reshape(-1)) if h >= 1]
  if psum is None or not np.any(columns >= 0) or not marks:
    index = pd.MultiIndex.from_arrays([labels[:0], np.zeros(0, np.int64)], names=["origin", "horizon"])
    return (pd.DataFrame({k: np.zeros(0) for k in PLACEBO_COLUMNS}, index=index),
            pd.DataFrame({k: np.zeros(0) for k in PLACEBO_PROFILE_COLUMNS}, index=pd.Index([], dtype=np.int64, name="horizon")))
  frames, rows = [], []
  for k, h in marks:
    frame, cols = _aggregate_placebo_frame({name: np.asarray(v)[:, k] for name, v in psum.items()},
                                           np.asarray(actual)[:, k], columns, h, alpha, labels)
    frames.append(frame)
    rows.append(_placebo_profile_row(cols, h, alpha, n_post, fit_relative_effect))
  by_horizon = pd.concat(frames, keys=[h for _, h in marks], names=["horizon", "origin"]).swaplevel().sort_index()
  profile = pd.DataFrame(rows, index=pd.Index([h for _, h in marks], dtype=np.int64, name="horizon"),
                         columns=list(PLACEBO_PROFILE_COLUMNS))
  return by_horizon, profile


# --------------------------------------------------------------------------------------
# Simultaneous bands and the whole-path test (`joint_bands=True`)
# --------------------------------------------------------------------------------------
JOINT_BAND_COLUMNS = ("posterior_lower", "posterior_upper", "point_effects_lower", "point_effects_upper",
                      "cumulative_effects_lower", "cumulative_effects_upper", "outside")
JOINT_SUMMARY_COLUMNS = ("critical_value", "max_excursion", "at", "n_outside", "first_outside", "p",
                         "significant")
JOINT_PATHS = ("pointwise", "cumulative")
# (nullable integer and boolean: a window a series does not cover has missing values in every column)
_JOINT_DTYPES = dict(critical_value="float64", max_excursion="float64", at=object, n_outside="Int64",
                     first_outside=object, p="float64", significant="boolean")


def joint_table_frame(rows, index) -> pd.DataFrame:
  """The `JOINT_SUMMARY_COLUMNS` frame of `rows` (dicts; None: a row of missing values) on `index`."""
  blank = dict(critical_value=np.nan, max_excursion=np.nan, at=None, n_outside=pd.NA, first_outside=None,
               p=np.nan, significant=pd.NA)
  # (labels stay objects whatever they are: a column of dates alone would else become datetime64)
  cols = {c: pd.Series([(blank if r is None else r)[c] for r in rows], index=index, dtype=_JOINT_DTYPES[c])
          for c in JOINT_SUMMARY_COLUMNS}
  return pd.DataFrame(cols, index=index, columns=list(JOINT_SUMMARY_COLUMNS))
# what a `SummaryRecord` keeps of `summarize_paths` (inside its `windows` kind, `path_` in front)
_PATH_RECORD = ("center", "spread", "excursion_order", "observed_excursion", "at", "exceed")


def _path_ranks(num_draws: int, alpha: float) -> List[int]:
  """The order statistics the 1 - alpha quantile of the excursions needs (`_quantile_ranks`)."""
  (lo, hi, _), = _quantile_ranks(num_draws, (1.0 - alpha,))
  return sorted({lo, hi})


def joint_windows(flags, windows: Optional["Windows"] = None) -> "Windows":
  """The windows `summarize_paths` takes for a fit: window 0 is the post-period (the steps whose flag
  bit 1 is set: a contiguous run), followed by the effect windows if any.  flags [T] or [B, T];
  windows: first, count [W] or [B, W]."""
  win = (np.asarray(flags) & 2) != 0
  count = win.sum(axis=-1)
  first = np.where(count > 0, win.argmax(axis=-1), 0)
  first, count = first[..., None], count[..., None]
  if windows is not None:
    more_first, more_count = (np.asarray(a) for a in windows)
    lead = np.broadcast_shapes(first.shape[:-1], more_first.shape[:-1])
    first = np.concatenate([np.broadcast_to(first, lead + (1,)), np.broadcast_to(more_first, lead + more_first.shape[-1:])], axis=-1)
    count = np.concatenate([np.broadcast_to(count, lead + (1,)), np.broadcast_to(more_count, lead + more_count.shape[-1:])], axis=-1)
  return Windows(first.astype(np.int32), count.astype(np.int32))


def _joint_critical(psum: Dict, ranks, num_draws: int, alpha: float) -> np.ndarray:
  """c [..., W, 2]: the 1 - alpha quantile of the excursions, interpolated from the two order
  statistics of path_excursion_order [..., W, 2, R] as numpy's linear method does."""
  order = {r: psum["path_excursion_order"][..., i] for i, r in enumerate(ranks)}
  (lo, hi, gamma), = _quantile_ranks(num_draws, (1.0 - alpha,))
  return _lerp_order_stats(order, lo, hi, gamma)


def _joint_rows(psum: Dict, w: int, critical, num_draws: int, observed, label_of) -> List[Optional[Dict]]:
  """The two rows (`JOINT_PATHS`) of window w of one series for `joint_table_frame`: psum {path_*:
  [W, 2, ...]}, critical [W, 2], observed [T]; label_of(step) -> the label of a model step.  None
  where the window counts no step."""
  rows = []
  for k in range(2):
    center, spread = psum["path_center"][w, k], psum["path_spread"][w, k]
    c, seen, at = critical[w, k], psum["path_observed_excursion"][w, k], int(psum["path_at"][w, k])
    if at < 0:
      rows.append(None)
      continue
    outside = _joint_outside(center, spread, observed if k == 0 else np.where(np.isnan(observed), np.nan, 0.0), c)
    steps = np.flatnonzero(outside)
    rows.append(dict(critical_value=c, max_excursion=seen, at=label_of(at), n_outside=int(steps.size),
                     first_outside=label_of(int(steps[0])) if steps.size else None,
                     p=(1.0 + int(psum["path_exceed"][w, k])) / (1.0 + num_draws),
                     significant=bool(seen > c)))
  return rows


def _joint_outside(center, spread, target, critical) -> np.ndarray:
  """[T] bool: the counted steps (a target, spread > 0) at which the target's standardised excursion
  exceeds `critical` -- the expression of observed_excursion, so `significant` is `outside.any()`."""
  with np.errstate(invalid="ignore", divide="ignore"):
    z = np.abs(target - center) / spread
    return ~np.isnan(target) & (spread > 0.0) & (z > critical)


def _joint_frames(psum: Optional[Dict], ranks, num_draws: int, alpha: float, observed, model_idx: pd.Index,
                  full_index: pd.Index, window_names=None):
  """(joint_bands, joint_summary, window_joint_summary) of one series from the path arrays of its
  record (`psum` {path_*: [W, 2, ...]}, window 0 the post-period, then the effect windows in the
  order of `window_names`; a window the series does not cover has count 0, hence NaN rows).  observed
  [T]: the outcome on the data scale over the model steps `model_idx`."""
  critical = _joint_critical(psum, ranks, num_draws, alpha)
  center, spread = psum["path_center"][0], psum["path_spread"][0]
  with np.errstate(invalid="ignore"):
    lower = [center[k] - critical[0, k] * spread[k] for k in range(2)]
    upper = [center[k] + critical[0, k] * spread[k] for k in range(2)]
    cols = {"posterior_lower": lower[0], "posterior_upper": upper[0],
            "point_effects_lower": observed - upper[0], "point_effects_upper": observed - lower[0],
            "cumulative_effects_lower": lower[1], "cumulative_effects_upper": upper[1],
            "outside": _joint_outside(center[0], spread[0], observed, critical[0, 0])}
  bands = pd.DataFrame(cols, index=model_idx, columns=list(JOINT_BAND_COLUMNS)).reindex(full_index)
  bands["outside"] = bands["outside"].eq(True)                     # (the rows the model never sees: not outside)
  label_of = lambda step: model_idx[step]   # pylint: disable=unnecessary-lambda-assignment
  rows = [_joint_rows(psum, w, critical, num_draws, observed, label_of) for w in range(critical.shape[0])]
  summary = joint_table_frame(rows[0], list(JOINT_PATHS))
  by_window = None
  if window_names:
    by_window = joint_table_frame(
        [r for two in rows[1:] for r in two],
        pd.MultiIndex.from_product([list(window_names), list(JOINT_PATHS)], names=["window", None]))
  return bands, summary, by_window


def _paths_record(got: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
  """What `summarize_paths` / `path_excursions_host` returned as the record keeps it."""
  return {"path_" + k: got[k] for k in _PATH_RECORD}


def _sanitize_seed(seed: Optional[_SeedType]) -> Tuple[int, int]:
  """int s -> (0, s); pair -> pair; None -> fresh entropy (reference :535-543)."""
  if seed is None:
    return tuple(int(v) for v in np.random.SeedSequence().generate_state(2))
  if isinstance(seed, (int, np.integer)):
    return (0, int(seed) & 0xFFFFFFFF)
  pair = np.asarray(seed).reshape(-1)
  if pair.shape[0] != 2:
    raise ValueError(f"seed must be an int or a pair of ints, got {seed!r}")
  return (int(pair[0]) & 0xFFFFFFFF, int(pair[1]) & 0xFFFFFFFF)


def split_rhat(draws: np.ndarray) -> float:
  """Split-R-hat of [chains, draws] (Gelman et al. 2013); NaN for degenerate input."""
  return _diagnostics.split_rhat(draws)


def effective_sample_size(draws: np.ndarray, kind: str = "plain") -> float:
  """Effective sample size of [chains, draws] scalar draws: split chains, FFT autocovariances,
  Geyer's initial monotone positive sequence.  kind: "plain" (the draws as they are), "bulk"
  (rank-normalised) or "tail" (min over the 5 % / 95 % indicators) -- Vehtari et al. 2021.
  NaN for degenerate input.  (SURVEY.md 8(f) N3 -- absent upstream.)"""
  fn = {"plain": _diagnostics.ess_plain, "bulk": _diagnostics.ess_bulk,
        "tail": _diagnostics.ess_tail}[kind]
  return fn(draws)


def _train_causalimpact_sts(*,
                            ci_data: cid.CausalImpactData,
                            prior_level_sd,
                            seed: Optional[_SeedType],
                            num_results: int,
                            num_warmup_steps: int,
                            model=None,
                            dtype=np.float32,
                            seasons: Sequence[Seasons] = (),
                            experimental_tf_function_cache_key_addition: int = 0,
                            num_chains: int = 1,
                            devices: Optional[Sequence[int]] = None,
                            local_linear_trend: bool = False,
                            sampler: str = "gibbs"):
  """Runs the Gibbs sampler on the GPU(s) (reference :503-606).

  Returns (samples dict, posterior_means [T], posterior_trajectories [draws, T]); draws are
  pooled over chains, chain-major.  Chain c uses RNG stream c regardless of how chains are
  spread over `devices`, so results are invariant to the device count.
  """
  del experimental_tf_function_cache_key_addition
  return _run_sampler(ci_data=ci_data, prior_level_sd=prior_level_sd, seed=seed,
                      num_results=num_results, num_warmup_steps=num_warmup_steps, model=model,
                      dtype=dtype, seasons=seasons, num_chains=num_chains, devices=devices,
                      local_linear_trend=local_linear_trend, sampler=sampler)[:3]


def _outcome_float64(ci_data) -> np.ndarray:
  """The pre-period outcome the sampler models.  Standardised data: `outcome_ts.time_series`, i.e.
  the values rounded to DataOptions.dtype exactly as the reference hands them to its sampler
  (data.py:125-126).  Raw-scale data (`standardize_data=False`): the float64 source column -- the
  rounding to float32 must come AFTER the internal conditioning, not before it."""
  src = getattr(ci_data, "model_pre_data", None)
  if getattr(ci_data, "standardize_data", True) or src is None:
    return np.asarray(ci_data.outcome_ts.time_series, np.float64)
  return np.asarray(src[ci_data.outcome_column], np.float64)


def _internal_conditioning(ci_data) -> Tuple[float, float]:
  """(mu, s) of the affine map y -> (y - mu) / s applied to the outcome before it reaches the
  float32 kernels when the caller did NOT standardise (`standardize_data=False`); (0, 1) else.

  The default model is exactly equivariant under it: every prior and every initial value the
  reference builds is expressed in units of outcome_sd (:424-443, :467-474, :566-574), the level
  prior is centred on the first observation (:467-469), and the weights prior is conjugate (its
  covariance carries sigma^2_obs).  So with y' = (y - mu) / s the Markov chain on
  (level' = (level - mu) / s, slope / s, seasonal / s, weights / s, scales / s) driven by the SAME
  random numbers is the same chain; the draws are mapped back in float64.  What this buys: the
  float32 scans never see a large offset or a tiny scale (the reference's own TODO case,
  causalimpact_lib_test.py:679-682: no standardisation, y + 100 with noise 1e-4, where float32
  would resolve the noise with a dozen levels).  tests/test_conditioning.py checks the
  equivariance on the float64 oracle (1e-9) and the GPU tests run that TODO case."""
  if getattr(ci_data, "standardize_data", True):
    return 0.0, 1.0
  pre = _outcome_float64(ci_data)
  pre = pre[~np.isnan(pre)]
  if pre.size < 2:
    return 0.0, 1.0
  mu, sd = float(np.mean(pre)), float(np.std(pre, ddof=1))
  if not np.isfinite(sd) or sd <= 0.0:
    sd = 1.0
  return mu, sd


def map_by_device(fn, work):
  """[fn(w) for w in work], every `w` a tuple that starts with its device: the items of one device
  run in their order, the devices side by side, each on a host thread of its own -- the library
  calls are synchronous and release the GIL, and there is no collective (chains and series are
  independent).  One device: no worker thread (a fresh host thread pays the runtime's per-thread
  set-up, ~30 ms, more than the fit of 512 series takes)."""
  by_dev: Dict[Any, List[int]] = {}
  for i, w in enumerate(work):
    by_dev.setdefault(w[0], []).append(i)
  if len(by_dev) <= 1:
    return [fn(w) for w in work]
  out = [None] * len(work)

  def run(positions):
    for i in positions:
      out[i] = fn(work[i])

  import concurrent.futures  # pylint: disable=import-outside-toplevel
  with concurrent.futures.ThreadPoolExecutor(max_workers=len(by_dev)) as pool_:
    list(pool_.map(run, by_dev.values()))     # (list: a worker's exception is raised here)
  return out


# --------------------------------------------------------------------------------------
# What a fit wants summarised where its draws lie, and what it got
# --------------------------------------------------------------------------------------
class Affine(NamedTuple):
  """value = internal * scale + shift: scalars, or [B] for the series of a launch."""
  scale: Any
  shift: Any


class Windows(NamedTuple):
  """Sub-windows of the steps: first, count [W], or [B, W] for the series of a launch."""
  first: Any
  count: Any


class PlaceboPart(NamedTuple):
  """The placebo forecasts' own (scale, shift), origins [O] or [B, O] (-1: unused, at the end of a
  row) and horizon (scalar or [B])."""
  scale: Any
  shift: Any
  origins: Any
  horizon: Any
  # `Placebo(simulate=True)` only: the (lower, upper) quantiles of the totals the frame reports -- None:
  # the analytic placebo --, the `_native.LINK_*` the simulated values are formed under, and per series
  # the `placebo_stream` (key, chains) its fit's random numbers are addressed by (one pair for all:
  # a single fit).  The observed totals are taken from the request's `observed` under a link.
  quantiles: Optional[Tuple[float, float]] = None
  link: int = 0
  streams: Any = None
  # `Placebo(horizons=...)` only: the horizons [K] or [B, K] (ascending, -1: unused, at the end of a row;
  # the last used one is `horizon`) the same origins are also looked from -- the placebo kind then has
  # the `PLACEBO_HORIZON_ARRAYS` [B, O, K] too
  horizons: Any = None


@dataclasses.dataclass(frozen=True)
class SummaryRequest:
  """What one fit -- a single series, or the series of one launch -- wants summarised over its
  draws.  Whoever fills it in (`take_summaries`, `_run_sampler`) does not modify it; the answers come
  back in a `SummaryRecord`."""
  scale: Any                    # the effect summary (`_native.Session.summarize`): scalars or [B]
  shift: Any
  observed: np.ndarray          # [T] or [B, T] data-scale outcome, NaN: none
  flags: np.ndarray             # [T] or [B, T] window flags
  ranks: Sequence[int]          # the order statistics every kind returns (`_summary_ranks`)
  components: bool = False
  predictions: Optional[Affine] = None
  windows: Optional[Windows] = None
  placebo: Optional[PlaceboPart] = None
  # `joint_bands`: the windows `summarize_paths` takes (`joint_windows`: window 0 the post-period) and
  # the order statistics of the excursions (`_path_ranks`).  The answers travel in the record's
  # `windows` kind under `path_` names: they are per-window arrays.
  paths: Optional[Windows] = None
  path_ranks: Sequence[int] = ()
  # (single fits) False: the effect and its windows are left to the host arithmetic of
  # `_compute_impact`; keep_trajectories: the predictive draws are wanted on the host as well
  on_device: bool = True
  keep_trajectories: bool = False
  # `outcome_link`: the `_native.LINK_*` under which the effect, its windows and its paths form their
  # values (`Session.set_link`); the record's effect then has value_mean
  link: int = 0


@dataclasses.dataclass(frozen=True)
class SummaryRecord:
  """What a fit got: per kind {name: [B, ...]} (`of_series`: one series' own), or None for a kind that
  was not asked for or that this route leaves to the host."""
  # (under `SummaryRequest.link` the effect has value_mean [B, T] too: the mean over the draws of the
  #  linked values, which the sampler's posterior_means no longer give)
  effect: Optional[Dict[str, np.ndarray]] = None
  components: Optional[Dict[str, np.ndarray]] = None
  predictions: Optional[Dict[str, np.ndarray]] = None
  windows: Optional[Dict[str, np.ndarray]] = None
  placebo: Optional[Dict[str, np.ndarray]] = None

  def kinds(self):
    return [(f.name, getattr(self, f.name)) for f in dataclasses.fields(self)]

  def map(self, fn) -> "SummaryRecord":
    """The record of fn(kind, arrays) for every kind that is there."""
    return SummaryRecord(**{kind: None if arrays is None else fn(kind, arrays) for kind, arrays in self.kinds()})

  def of_series(self, b: int) -> "SummaryRecord":
    return self.map(lambda _, arrays: {k: v[b] for k, v in arrays.items()})


# `Placebo(horizons=...)`: the five arrays of the placebo kind at every horizon, [B, O, K]
PLACEBO_HORIZON_ARRAYS = ("horizons_predicted_mean", "horizons_spread_mean", "horizons_pit_mean",
                          "horizons_n_counted", "horizons_seen_sum")


class SummaryKind(NamedTuple):
  """How the arrays of one kind are laid out: series first and, but for the names in `whole`, time
  last -- cut to a series' length, and padded with `fill` beyond it when launches are put together."""
  whole: Tuple[str, ...]
  fill: float
  also: Tuple[str, ...] = ()    # names only some routes return, laid out like those in `whole`


SUMMARY_KINDS = {
    "effect": SummaryKind(("per_draw", "per_draw_order"), np.nan),            # [B, 2, draws | R]; value_mean [B, T]
    "components": SummaryKind(("inclusion_prob", "weight_mean", "weight_order"), np.nan),   # [B, ..., P]
    "predictions": SummaryKind(("loglik",), np.nan),                          # [B, draws]
    # [B, W, 2, draws | R]; `joint_bands`: path_center, path_spread [B, 1 + W, 2, T] over time, the rest whole
    "windows": SummaryKind(("per_draw", "per_draw_order", "path_excursion_order", "path_observed_excursion",
                            "path_at", "path_exceed"), np.nan),
    # [B, O]; predicted_lower, predicted_upper on the simulated route (`Placebo(simulate=True)`) only
    "placebo": SummaryKind(("predicted_mean", "spread_mean", "pit_mean", "n_counted", "seen_sum"),
                           np.nan, ("predicted_lower", "predicted_upper") + PLACEBO_HORIZON_ARRAYS)}
# the parameter draws the prediction errors and the placebo forecasts are filtered from on the host
_PARAMETER_DRAWS = ("observation_noise_scale", "level_scale", "slope_scale", "seasonal_drift_scales",
                    "weights")


def _to_internal_units(scale, shift, cond_mu, cond_s) -> Affine:
  """The caller's (scale, shift) as the map from the sampler's internal units
  (`_internal_conditioning`: internal = (value - cond_mu) / cond_s) to the data scale, in float64."""
  scale = np.asarray(scale, np.float64)
  return Affine(scale * cond_s, np.asarray(shift, np.float64) + cond_mu * scale)


def _request_in_internal_units(request: SummaryRequest, cond_mu, cond_s) -> SummaryRequest:
  """`request` with every part's own (scale, shift) mapped by `_to_internal_units`."""
  own = lambda part: _to_internal_units(part.scale, part.shift, cond_mu, cond_s)   # pylint: disable=unnecessary-lambda-assignment
  return dataclasses.replace(
      request, **own(request)._asdict(),
      predictions=None if request.predictions is None else own(request.predictions),
      placebo=None if request.placebo is None else request.placebo._replace(**own(request.placebo)._asdict()))


@dataclasses.dataclass(frozen=True)
class SeriesInputs:
  """One series as its sampler saw it, for the summaries taken in numpy: y, mask [T], design [T, P]
  or None (`seen`: the number format the sampler read them in), season_change [K, T], the model and
  the parameter block (`_model.series_params`)."""
  y: np.ndarray
  mask: np.ndarray
  design: Optional[np.ndarray]
  season_change: np.ndarray
  num_seasons: Sequence[int]
  has_slope: bool
  params: Dict
  seen: Any = np.float32

  def outcome(self) -> np.ndarray:
    return np.where(self.mask, 0.0, self.y).astype(self.seen)

  def filter_inputs(self):
    """(y, mask, X, season_change, num_seasons, has_slope, params) of the host filters."""
    return (self.outcome(), self.mask, None if self.design is None else self.design.astype(self.seen),
            self.season_change, self.num_seasons, self.has_slope, self.params)


def _pooled_draws(draws: Dict[str, np.ndarray], i: int) -> Dict[str, np.ndarray]:
  """{name: [C * S, ...]} of series i of {name: [n, C, S, ...]}, chain-major."""
  return {k: v[i].reshape((v.shape[1] * v.shape[2],) + v.shape[3:]) for k, v in draws.items()}


def _host_prediction_summaries(inputs: Sequence[SeriesInputs], draws, own: Affine, ranks):
  """The prediction summary {name: [n, ...]} of n series in numpy (`_prediction_summary_host`) from
  their parameter draws {name: [n, C, S, ...]} (a name the model lacks may be missing): the routes
  whose models the device filter does not take.  Over the steps of the longest series, with the
  padding convention of the device beyond a series' length."""
  n, R, num_steps = len(inputs), len(ranks), max(i.y.shape[0] for i in inputs)
  scale, shift = (np.broadcast_to(np.asarray(a, np.float64), (n,)) for a in own)
  out = None
  for i, one in enumerate(inputs):
    got = _prediction_summary_host(*one.filter_inputs(), _pooled_draws(draws, i), scale[i], shift[i], ranks)
    if out is None:
      out = dict(forecast_mean=np.zeros((n, num_steps)), forecast_order=np.zeros((n, R, num_steps)),
                 variance_mean=np.zeros((n, num_steps)), pit_mean=np.zeros((n, num_steps)),
                 loglik=np.zeros((n, got["loglik"].shape[0])))
    out["forecast_mean"][i], out["forecast_order"][i] = shift[i], shift[i]
    for k, v in got.items():
      out[k][i, ..., :v.shape[-1]] = v
  return out


def _host_placebo_summaries(inputs: Sequence[SeriesInputs], draws, part: PlaceboPart):
  """The same for the placebo summary (`_placebo_summary_host`; `part` per series: `_per_series`); a
  series without an origin stays at zero."""
  out = {k: np.zeros(part.origins.shape) for k in SUMMARY_KINDS["placebo"].whole[:3]}
  if part.horizons is not None:
    # (`Placebo(horizons=...)`: the one loop records the checkpoints; the columns at H are the summary at H)
    table = {k: np.zeros(part.origins.shape + (part.horizons.shape[1],)) for k in out}
    for i, one in enumerate(inputs):
      if np.any(part.origins[i] >= 0):
        got = _placebo_summary_host(*one.filter_inputs(), _pooled_draws(draws, i), part.scale[i],
                                    part.shift[i], part.origins[i], horizons=part.horizons[i])
        for k, v in got.items():
          table[k][i] = v
    return _placebo_with_horizons(table, part)
  for i, one in enumerate(inputs):
    if np.any(part.origins[i] >= 0):
      got = _placebo_summary_host(*one.filter_inputs(), _pooled_draws(draws, i), part.scale[i],
                                  part.shift[i], part.origins[i], part.horizon[i])
      for k, v in got.items():
        out[k][i] = v
  return out


def _placebo_with_horizons(table: Dict[str, np.ndarray], part: PlaceboPart) -> Dict[str, np.ndarray]:
  """The placebo summary {name: [n, O]} at H -- every series' LAST used column of `table` {name:
  [n, O, K]}: the checkpoint at H is the forecast at H -- and the table itself under the
  `PLACEBO_HORIZON_ARRAYS` names."""
  last = np.maximum((np.asarray(part.horizons) > 0).sum(axis=1) - 1, 0)
  out = {k: np.take_along_axis(v, last[:, None, None], axis=2)[:, :, 0] for k, v in table.items()}
  out.update({"horizons_" + k: v for k, v in table.items()})
  return out


def draws_filter_route(has_slope: bool, num_seasons: Sequence[int], on_device: bool = True) -> str:
  """Where prediction errors and placebo forecasts are filtered from parameter draws that lie on the
  host (float64 fits, HMC fits, chains pooled from several devices, the one-launch HMC batch):
  "one_lane" -- a `_native.DrawsSession` and the entries of `device_predictions_supported` --, "blocks"
  -- the same session and the `_blocks` entries (`device_block_predictions_supported`: a state of at
  most `PREDICTION_MAX_STATE` components) --, or "host": the numpy twins, with
  `InferenceOptions(summarize_on_device=False)` and for any wider state."""
  if not on_device:
    return "host"
  if device_predictions_supported(num_seasons):
    return "one_lane"
  if device_block_predictions_supported(has_slope, num_seasons):
    return "blocks"
  return "host"


def open_draws_session(inputs: Sequence[SeriesInputs], draws, *, seed, device: int = 0, series_offset: int = 0,
                       shared_streams: bool = True):
  """The `_native.DrawsSession` of the n series `inputs` -- one model, one length -- and their
  parameter draws {name: [n, C, S, ...]} (`_PARAMETER_DRAWS`; a name the model lacks may be missing)
  on `device`.  Float64 where the sampler read float64 (`SeriesInputs.seen`) or handed float64 draws,
  else float32: the values the numpy twins read, as they read them.  seed, series_offset,
  shared_streams: what keys the series' random streams (`placebo_stream`: series i of the session is
  series id series_offset + i, or the seed itself with shared_streams); the chains are the global
  chains 0 .. C - 1 in pooling order.  None where the series do not share a length."""
  one = inputs[0]
  num_steps = one.y.shape[0]
  if any(i.y.shape[0] != num_steps for i in inputs):
    return None
  used = {k: np.asarray(draws[k]) for k in _PARAMETER_DRAWS if draws.get(k) is not None}
  wide = one.seen == np.float64 or any(v.dtype == np.float64 for v in used.values())
  num_chains, num_results = used["observation_noise_scale"].shape[1:3]
  P = 0 if one.design is None else one.design.shape[1]
  if P == 0:
    used.pop("weights", None)
  if not one.num_seasons:
    used.pop("seasonal_drift_scales", None)
  pb = _native.make_problem(
      T=num_steps, P=P, has_slope=one.has_slope, num_seasons=one.num_seasons, num_warmup=0,
      num_results=num_results, num_chains=num_chains, num_series=len(inputs), seed=seed, device=device,
      flags=_native.FLAG_SHARED_SERIES_STREAMS if shared_streams else 0, series_offset=series_offset)
  return _native.DrawsSession(
      pb, np.stack([i.y.astype(i.seen) for i in inputs]), np.stack([i.mask for i in inputs]),
      None if P == 0 else np.stack([i.design.astype(i.seen) for i in inputs]), one.season_change,
      _native.make_params([i.params for i in inputs]), used, dtype=np.float64 if wide else np.float32)


def _draws_session_beside(sess, inputs: Sequence[SeriesInputs], draws, on_device: bool):
  """(`open_draws_session`, blocks) for the series of the open session `sess`, which has no filter
  entries of its own (the one-launch HMC batch), keyed as `sess` keys its series; (None, False): the
  numpy twins (`draws_filter_route`; a session that has the entries and came here all the same has
  a model they do not take, or a library without one of them)."""
  origin = getattr(sess, "problem", None) or getattr(sess, "pb", None)
  route = draws_filter_route(inputs[0].has_slope, inputs[0].num_seasons, on_device)
  if origin is None or route == "host" or {"predictions", "placebo"} <= set(getattr(sess, "summaries", ())):
    return None, False
  drawn = open_draws_session(
      inputs, draws, seed=(int(origin.seed[0]), int(origin.seed[1])), device=int(origin.device),
      series_offset=int(origin.series_offset),
      shared_streams=bool(origin.flags & _native.FLAG_SHARED_SERIES_STREAMS))
  return drawn, route == "blocks"


def pool_placebo_horizons_available(blocks: bool) -> bool:
  """Whether the loaded library has ci_session_pool_placebo_horizons (blocks: its `_blocks` form)."""
  return hasattr(_native.load(), "ci_session_pool_placebo_horizons" + ("_blocks" if blocks else ""))


def pool_placebo_horizon_columns(sess, blocks: bool, scale, shift, groups, origins, horizons, init=None,
                                 one_pass: Optional[bool] = None, max_bytes: int = 1 << 30) -> np.ndarray:
  """acc [G, O, K, 2, N] of `Session.pool_placebo_horizons` on the open session `sess` (blocks: the
  `_blocks` entry), however the library and the memory allow it: ONE filter pass where the loaded
  library has the entry (one_pass None: ask it), the horizon slots in ascending column chunks where the
  accumulators would take more than max_bytes (the limit of the C entry) -- the columns are independent,
  so no bit depends on that cut -- and K calls of `pool_placebo` (`pool_placebo_blocks`) where it lacks
  the entry: the definition, and the bit reference.  groups: one mapping per group; origins: one mapping
  {place: row} per group; horizons [G, K] (-1: unused, at the end); init: [G, O, K, 2, N] or None.  A
  group without a used slot among the columns of a call takes no part in it."""
  hz = np.asarray(horizons, np.int32)
  n_groups, width = hz.shape
  if one_pass is None:
    one_pass = pool_placebo_horizons_available(blocks)
  slots = max([np.asarray(row).size for m in origins for row in m.values()] + [1])
  num_draws = int(sess.pb.num_chains * sess.pb.num_results)
  per_column = n_groups * slots * 2 * num_draws * 8
  step = max(1, min(width, max_bytes // max(per_column, 1))) if one_pass else 1
  acc = np.zeros((n_groups, slots, width, 2, num_draws)) if init is None else np.array(init, np.float64)
  single = sess.pool_placebo_blocks if blocks else sess.pool_placebo
  for j in range(0, width, step):
    sub = hz[:, j:j + step]
    used = (sub > 0).any(axis=1)
    if not used.any():
      continue
    here = [groups[g] if used[g] else {} for g in range(n_groups)]
    rows = [origins[g] if used[g] else {} for g in range(n_groups)]
    before = np.ascontiguousarray(acc[:, :, j:j + step]) if init is not None else None
    if one_pass:
      table = np.where(used[:, None], sub, np.array([1] + [-1] * (sub.shape[1] - 1), np.int32)[None, :])
      acc[:, :, j:j + step] = sess.pool_placebo_horizons(scale, shift, here, rows, table, before, blocks=blocks)["acc"]
    else:
      acc[:, :, j] = single(scale, shift, here, rows, np.where(used, sub[:, 0], 1),
                            None if before is None else np.ascontiguousarray(before[:, :, 0]))["acc"]
  return acc


def _placebo_entry_device(drawn, blocks: bool, one: "SeriesInputs", scale, shift, observed, origins, horizon,
                          simulated=None, horizons=None) -> Dict:
  """`_placebo_entry_host` -- with simulated = (link, stream) `_placebo_entry_simulated_host` -- through
  the one-series draws session `drawn`: the group table of one group with this member at weight 1,
  whose accumulators are 0 + 1 * term, the member's own terms.  horizons [K]: the terms [O, K, N] at the
  group's horizons (`pool_placebo_horizon_columns`)."""
  origins = np.asarray(origins).reshape(-1)
  if horizons is not None:
    if simulated is not None:
      raise ValueError("the simulated pooled placebo has one horizon")
    hz = np.asarray(horizons, np.int32).reshape(1, -1)
    seen = _placebo_entry_seen(one, scale, shift, observed, origins, horizon, horizons=hz[0])
    width = int((origins >= 0).sum())
    acc = np.zeros((origins.size, hz.shape[1], 2, drawn.pb.num_chains * drawn.pb.num_results))
    if width:
      acc[:width] = pool_placebo_horizon_columns(drawn, blocks, scale, shift, [{0: 1.0}], [{0: origins[:width]}], hz)[0]
    return dict(s=acc[:, :, 0], v=acc[:, :, 1], **seen)
  link = simulated[0] if simulated is not None else 0
  seen = _placebo_entry_seen(one, scale, shift, observed, origins, horizon, link)
  num_draws = drawn.pb.num_chains * drawn.pb.num_results
  width = int((origins >= 0).sum())
  planes = 1 if simulated is not None else 2
  acc = np.zeros((origins.size, planes, num_draws))
  if width:
    if simulated is not None:
      entry = drawn.pool_simulated_placebo_blocks if blocks else drawn.pool_simulated_placebo
      got = entry(scale, shift, [{0: 1.0}], [{0: origins[:width]}], [int(horizon)], link)["acc"]
      acc[:width, 0] = got[0]
    else:
      entry = drawn.pool_placebo_blocks if blocks else drawn.pool_placebo
      acc[:width] = entry(scale, shift, [{0: 1.0}], [{0: origins[:width]}], [int(horizon)])["acc"][0]
  if simulated is not None:
    return dict(totals=acc[:, 0], **seen)
  return dict(s=acc[:, 0], v=acc[:, 1], **seen)


def _device_placebo_summaries(sess, part: PlaceboPart, blocks: bool = False):
  """The placebo summary {name: [n, O]} of an open session (`summarize_placebo`, with `blocks`
  `summarize_placebo_blocks`): the launch's own origin slots (never more than its steps), the horizon
  of a series without origin raised to the 1 the entry asks for."""
  width = max(1, int((part.origins >= 0).sum(axis=1).max()))
  entry = sess.summarize_placebo_blocks if blocks else sess.summarize_placebo
  if part.horizons is not None:
    # `Placebo(horizons=...)`: ONE filter pass for all horizons (`summarize_placebo_horizons`); for the
    # block models one call of `summarize_placebo_blocks` per horizon slot, the same origins -- the same
    # definitions, a series without that slot at its own H (not read)
    hz = np.asarray(part.horizons)
    table = {k: np.zeros(part.origins.shape + (hz.shape[1],)) for k in _native.PLACEBO_OUTPUTS}
    if blocks:
      for k in range(hz.shape[1]):
        used = hz[:, k] > 0
        if used.any():
          got = entry(part.scale, part.shift, part.origins[:, :width],
                      np.where(used, hz[:, k], np.maximum(part.horizon, 1)))
          for name, v in got.items():
            table[name][used, :width, k] = v[used]
    else:
      rows = np.where((hz > 0).any(axis=1)[:, None], hz, np.array([1] + [-1] * (hz.shape[1] - 1))[None, :])
      for name, v in sess.summarize_placebo_horizons(part.scale, part.shift, part.origins[:, :width], rows).items():
        table[name][:, :width] = v
    return _placebo_with_horizons(table, part)
  got = entry(part.scale, part.shift, part.origins[:, :width], np.maximum(part.horizon, 1))
  out = {k: np.zeros(part.origins.shape) for k in got}
  for k, v in got.items():
    out[k][:, :width] = v
  return out


def _placebo_entry_host(one: "SeriesInputs", draws, scale, shift, observed, origins, horizon, horizons=None) -> Dict:
  """What one member adds to a pooled placebo forecast, filtered in numpy: for the origins [O] (steps
  of the series; -1: unused, at the end) and the horizon of the GROUP, s and v [O, N] on the data
  scale (`_placebo_summary_host(per_draw=True)`, `_native.placebo_terms_host`), n_counted and seen_sum
  [O] (`_placebo_seen`; 0 in an unused slot) and actual [O], the observed sum of every window
  (`observed`: the series' outcome on the data scale, NaN: none).  draws: the series' pooled
  parameter draws.  horizons [K] (-1: unused, at the end; `horizon` their last one): s, v [O, K, N] and
  the rest [O, K] at the group's horizons, column k what `horizon=horizons[k]` gives, 0 in an unused slot."""
  origins = np.asarray(origins).reshape(-1)
  if horizons is not None:
    got = _placebo_summary_host(*one.filter_inputs(), draws, scale, shift, origins, horizon, per_draw=True,
                                horizons=horizons)
    s, v = _native.placebo_terms_host(got["C"], got["V"], got["cnt"], scale, shift)
    return dict(s=s, v=v, **_placebo_entry_seen(one, scale, shift, observed, origins, horizon, horizons=horizons))
  got = _placebo_summary_host(*one.filter_inputs(), draws, scale, shift, origins, horizon, per_draw=True)
  s, v = _native.placebo_terms_host(got["C"], got["V"], got["cnt"], scale, shift)
  return dict(s=s, v=v, **_placebo_entry_seen(one, scale, shift, observed, origins, horizon))


def _placebo_entry_seen(one: "SeriesInputs", scale, shift, observed, origins, horizon, link: int = 0,
                        horizons=None) -> Dict:
  """n_counted, seen_sum and actual [O] of `_placebo_entry_host`: what needs no draws.  Under an
  outcome link (the simulated pooled placebo) seen_sum is the sum of the RAW outcome `observed` over
  the counted steps (`_placebo_seen_linked`).  horizons [K] (identity link): all three [O, K], the
  prefixes of the same running sums (`_placebo_seen(horizons=...)`), 0 in an unused horizon slot."""
  origins = np.asarray(origins).reshape(-1)
  observed = np.asarray(observed, np.float64)
  if horizons is not None:
    if link:
      raise ValueError("the pooled placebo at several horizons has no outcome link")
    hz = [int(h) for h in np.asarray(horizons).reshape(-1)]
    last = max([h for h in hz if h >= 1] + [1])
    cnt, seen = _placebo_seen(one.outcome(), one.mask, origins, last, scale, shift, horizons=hz)
    steps = np.maximum(origins, 0).astype(np.int64)[:, None] + np.arange(last)[None, :]
    values = observed[np.minimum(steps, observed.shape[0] - 1)]
    values = np.where(np.isnan(values), 0.0, values)      # (what `np.nansum` adds up, replaced once)
    actual = np.zeros((origins.size, len(hz)))
    for k, h in enumerate(hz):
      if h >= 1:                                          # the sum of the window's own h steps, as at one horizon
        actual[:, k] = np.add.reduce(values[:, :h], axis=1)
    actual[origins < 0] = 0.0
    return dict(n_counted=cnt, seen_sum=np.nan_to_num(seen), actual=actual)
  if link:
    cnt, seen = _placebo_seen_linked(observed, one.mask, origins, horizon, link)
  else:
    cnt, seen = _placebo_seen(one.outcome(), one.mask, origins, horizon, scale, shift)
  # (every window's own contiguous steps, summed as `_placebo_columns` sums them; 0 in an unused slot)
  steps = np.maximum(origins, 0).astype(np.int64)[:, None] + np.arange(int(horizon))[None, :]
  actual = np.where(origins >= 0, np.nansum(observed[np.minimum(steps, observed.shape[0] - 1)], axis=1), 0.0)
  return dict(n_counted=cnt, seen_sum=np.nan_to_num(seen), actual=actual)


def _per_series(part: PlaceboPart, n: int) -> PlaceboPart:
  """`part` with one row per series: scale, shift, horizon [n], origins [n, O], streams n pairs."""
  origins = np.asarray(part.origins)
  streams = part.streams
  if streams is not None and len(streams) == 2 and not isinstance(streams[0][0], (tuple, list)):
    streams = [streams] * n              # (one (key, chains) pair for all)
  return part._replace(scale=np.broadcast_to(np.asarray(part.scale, np.float64), (n,)),
                       shift=np.broadcast_to(np.asarray(part.shift, np.float64), (n,)),
                       origins=np.broadcast_to(origins, (n, origins.shape[-1])),
                       horizon=np.broadcast_to(np.asarray(part.horizon), (n,)), streams=streams,
                       horizons=None if part.horizons is None else
                       np.broadcast_to(np.asarray(part.horizons), (n, np.shape(part.horizons)[-1])))


def _placebo_seen_linked(observed, mask, origins, horizon: int, link: int):
  """`_placebo_seen` under an outcome link: (n_counted [O], seen_sum [O]) with seen_sum the sum of the
  RAW outcome (`observed`, data scale) over the counted steps of every window, ascending in float64.
  Those steps are rows the model conditions on; ValueError if one lies outside the link's domain."""
  observed = np.asarray(observed, np.float64)
  mask = np.asarray(mask, bool)
  origins = np.asarray(origins).reshape(-1)
  n_counted, seen_sum = np.zeros(origins.size), np.full(origins.size, np.nan)
  used = origins >= 0
  if used.any():
    steps = origins[used].astype(np.int64)[:, None] + np.arange(int(horizon))[None, :]     # [O, H]
    seen = ~mask[steps]
    values = observed[steps]
    with np.errstate(invalid="ignore"):
      inside = values > (0.0 if link == _native.LINK_LOG else -1.0)
    if np.any(seen & ~inside):
      o, h = np.argwhere(seen & ~inside)[0]
      raise ValueError(f"placebo: the outcome {values[o, h]!r} at model step {int(steps[o, h])} lies outside the "
                       "domain of `outcome_link`")
    n_counted[used] = seen.sum(axis=1).astype(np.float64)
    seen_sum[used] = np.cumsum(np.where(seen, values, 0.0), axis=1)[:, -1]
  return n_counted, seen_sum


def _placebo_sim_ranks(num_draws: int, quantiles) -> List[int]:
  """The order statistics of the simulated totals the two quantiles of the frame need."""
  return sorted({r for lo, hi, _ in _quantile_ranks(num_draws, quantiles) for r in (lo, hi)})


def _simulated_placebo_summaries(inputs: Sequence[SeriesInputs], part: PlaceboPart, observed, num_draws: int,
                                 simulate) -> Dict[str, np.ndarray]:
  """The placebo kind of a record on the simulated route, {name: [n, O]}: n_counted and seen_sum of
  every series (`_placebo_seen_linked` on `observed` [T] or [n, T] under a link, `_placebo_seen`
  under the identity), then simulate(seen [n, O] with 0 in the unused slots, ranks) -> predicted_mean,
  spread_mean, below [n, O], total_order [n, R, O] of the device or the numpy twin, and from them
    pit_mean = (below + 0.5) / (N + 1)
    predicted_lower, predicted_upper: the part's quantiles of the totals, interpolated from the order
    statistics as `series` interpolates its bands."""
  n = len(inputs)
  seen = []
  for i, one in enumerate(inputs):
    if part.link:
      obs = np.broadcast_to(np.asarray(observed, np.float64), (n, np.shape(observed)[-1]))[i]
      seen.append(_placebo_seen_linked(obs, one.mask, part.origins[i], part.horizon[i], part.link))
    else:
      seen.append(_placebo_seen(one.outcome(), one.mask, part.origins[i], part.horizon[i],
                                part.scale[i], part.shift[i]))
  n_counted, seen_sum = np.stack([c for c, _ in seen]), np.stack([a for _, a in seen])
  ranks = _placebo_sim_ranks(num_draws, part.quantiles)
  got = simulate(np.nan_to_num(seen_sum), ranks)
  return dict(_simulated_placebo_means(got, ranks, num_draws, part.quantiles), n_counted=n_counted,
              seen_sum=seen_sum)


def _simulated_placebo_means(got: Dict[str, np.ndarray], ranks, num_draws: int, quantiles) -> Dict[str, np.ndarray]:
  """What the frames of a simulated placebo read, from the statistics of `simulate_placebo` or
  `pool_simulated_placebo` (predicted_mean, spread_mean, below [n, O], total_order [n, R, O] at
  `ranks` = `_placebo_sim_ranks`): predicted_mean, spread_mean, pit_mean = (below + 0.5) / (N + 1) and
  predicted_lower, predicted_upper, the two quantiles interpolated from the order statistics."""
  pos = {r: i for i, r in enumerate(ranks)}
  (lo_a, hi_a, g_a), (lo_b, hi_b, g_b) = _quantile_ranks(num_draws, quantiles)
  by_rank = {r: got["total_order"][:, pos[r]] for r in (lo_a, hi_a, lo_b, hi_b)}
  return dict(predicted_mean=got["predicted_mean"], spread_mean=got["spread_mean"],
              pit_mean=(got["below"] + 0.5) / (num_draws + 1.0),
              predicted_lower=_lerp_order_stats(by_rank, lo_a, hi_a, g_a),
              predicted_upper=_lerp_order_stats(by_rank, lo_b, hi_b, g_b))


def _placebo_entry_simulated_host(one: "SeriesInputs", draws, scale, shift, observed, origins, horizon,
                                  link: int, stream) -> Dict:
  """What one member adds to a SIMULATED pooled placebo forecast, in numpy: totals [O, N], the
  simulated totals of `_placebo_simulated_host` at the origins [O] and the horizon of the GROUP on
  the member's own stream (`placebo_stream` of its series), and n_counted, seen_sum, actual [O] of
  `_placebo_entry_seen` under `link`."""
  origins = np.asarray(origins).reshape(-1)
  got = _placebo_simulated_host(*one.filter_inputs(), draws, scale, shift, origins, horizon, link, stream)
  return dict(totals=got["totals"], **_placebo_entry_seen(one, scale, shift, observed, origins, horizon, link))


def _host_placebo_simulations(inputs: Sequence[SeriesInputs], draws, part: PlaceboPart):
  """simulate(seen, ranks) of `_simulated_placebo_summaries` in numpy (`_placebo_simulated_host`) from
  the parameter draws {name: [n, C, S, ...]}; a series without an origin stays at zero."""
  def simulate(seen, ranks):
    shape = part.origins.shape
    out = dict(predicted_mean=np.zeros(shape), spread_mean=np.zeros(shape), below=np.zeros(shape),
               total_order=np.zeros((shape[0], len(ranks), shape[1])))
    for i, one in enumerate(inputs):
      if np.any(part.origins[i] >= 0):
        got = _placebo_simulated_host(*one.filter_inputs(), _pooled_draws(draws, i), part.scale[i], part.shift[i],
                                      part.origins[i], part.horizon[i], part.link, part.streams[i], seen=seen[i],
                                      ranks=ranks)
        for k in out:
          out[k][i] = got[k]
    return out
  return simulate


def _device_placebo_simulations(sess, part: PlaceboPart, blocks: bool = False):
  """simulate(seen, ranks) of `_simulated_placebo_summaries` on an open session (`simulate_placebo`,
  with `blocks` `simulate_placebo_blocks`): the launch's own origin slots, as `_device_placebo_summaries`."""
  def simulate(seen, ranks):
    width = max(1, int((part.origins >= 0).sum(axis=1).max()))
    got = sess.simulate_placebo(part.scale, part.shift, part.origins[:, :width], np.maximum(part.horizon, 1),
                                part.link, seen[:, :width], ranks, blocks=blocks)
    out = {k: np.zeros(v.shape[:-1] + (part.origins.shape[1],)) for k, v in got.items()}
    for k, v in got.items():
      out[k][..., :width] = v
    return out
  return simulate


def _with_placebo_seen(inputs: Sequence[SeriesInputs], part: PlaceboPart, plsum):
  """`plsum` {name: [n, O]} with `_placebo_seen`'s n_counted and seen_sum of every series."""
  seen = [_placebo_seen(one.outcome(), one.mask, part.origins[i], part.horizon[i],
                        part.scale[i], part.shift[i]) for i, one in enumerate(inputs)]
  out = dict(plsum, n_counted=np.stack([c for c, _ in seen]), seen_sum=np.stack([a for _, a in seen]))
  if part.horizons is not None:        # (`Placebo(horizons=...)`: the prefixes of the same sums)
    seen = [_placebo_seen(one.outcome(), one.mask, part.origins[i], max(int(part.horizon[i]), 1),
                          part.scale[i], part.shift[i], horizons=part.horizons[i]) for i, one in enumerate(inputs)]
    out.update(horizons_n_counted=np.stack([c for c, _ in seen]), horizons_seen_sum=np.stack([a for _, a in seen]))
  return out


def take_summaries(sess, request: SummaryRequest,
                   series_inputs: Optional[Sequence[SeriesInputs]] = None) -> SummaryRecord:
  """Fills the record of `request` from the finished, still open session `sess`: `summarize`,
  `summarize_components`, `summarize_predictions`, `summarize_windows` (`summarize_paths` directly
  after it), `summarize_placebo`, in this order for every caller -- every entry uploads its own arguments and leaves nothing behind for the
  next (tests/test_gpu_summaries_together.py).  `sess.summaries` names the kinds a session has.
  Prediction errors and placebo forecasts are filtered on the device where the session has the
  entries and `device_predictions_supported` takes the model; else by the block-model entries
  (`summarize_predictions_blocks`, `summarize_placebo_blocks`) where the session has those and
  `device_block_predictions_supported` takes it; else from the parameter draws, fetched once for
  both, over `series_inputs` (one per series of the session; read for these two kinds only): a
  session without filter entries (the one-launch HMC batch) through ONE `_native.DrawsSession` over
  its series (`_draws_session_beside`), in numpy with `request.on_device` off, for a wider state and
  for a session whose library lacks an entry.  A placebo part with `quantiles` is the SIMULATED placebo (`simulate_placebo`,
  `simulate_placebo_blocks`, `_placebo_simulated_host`, chosen the same way; a session without the
  entry filters on the host).  Components a session lacks stay None: the caller's business.  The scales and shifts
  map the SESSION's units to the data scale (`_request_in_internal_units`).  With `request.link` the
  session's link is set first (`set_link`: the effect, its windows and paths then form linked values,
  and so does a pool step that follows while the session is open) and the effect gets `value_mean`
  from a last call."""
  if request.link:
    # (session state: `summarize`, `summarize_windows`, `summarize_paths` and `value_mean` honour it;
    #  the components, prediction errors and placebo forecasts describe the model and do not)
    sess.set_link(request.link)
  effect = sess.summarize(request.scale, request.shift, request.observed, request.flags, request.ranks)
  if effect["value_order"].ndim == 2:      # (`Session.summarize` drops the series axis of one series)
    effect = {k: v[None] for k, v in effect.items()}
  components = predictions = windows = placebo = draws = None
  if request.components and "components" in sess.summaries:
    components = sess.summarize_components(request.scale, request.shift, request.ranks)
  filtered = request.predictions is not None or request.placebo is not None
  has_entries = {"predictions", "placebo"} <= set(sess.summaries)
  simulated = request.placebo is not None and request.placebo.quantiles is not None
  if simulated and not hasattr(sess, "simulate_placebo"):
    has_entries = False
  one_lane = filtered and has_entries and device_predictions_supported(series_inputs[0].num_seasons)
  blocks = (filtered and has_entries and not one_lane and hasattr(sess, "summarize_predictions_blocks")
            and hasattr(sess, "summarize_placebo_blocks")
            and device_block_predictions_supported(series_inputs[0].has_slope, series_inputs[0].num_seasons))
  on_host = filtered and not (one_lane or blocks)
  flt = sess                               # the session that filters: this one, or one made from its draws
  if on_host:
    draws = sess.fetch(list(_PARAMETER_DRAWS))
    flt, blocks = _draws_session_beside(sess, series_inputs, draws, request.on_device)
    on_host = flt is None
  try:
    if request.predictions is not None:
      if on_host:
        predictions = _host_prediction_summaries(series_inputs, draws, request.predictions, request.ranks)
      else:
        entry = flt.summarize_predictions_blocks if blocks else flt.summarize_predictions
        predictions = entry(*request.predictions, request.ranks)
    if request.windows is not None:
      windows = sess.summarize_windows(request.scale, request.shift, request.observed, *request.windows,
                                       request.ranks)
    if request.paths is not None:
      windows = dict(windows or {}, **_paths_record(sess.summarize_paths(
          request.scale, request.shift, request.observed, *request.paths, request.path_ranks, want=_PATH_RECORD)))
    if simulated:
      part = _per_series(request.placebo, len(series_inputs))
      num_draws = (int(np.prod(draws["observation_noise_scale"].shape[1:3])) if on_host else
                   flt.pb.num_chains * flt.pb.num_results)
      placebo = _simulated_placebo_summaries(
          series_inputs, part, request.observed, num_draws,
          _host_placebo_simulations(series_inputs, draws, part) if on_host else
          _device_placebo_simulations(flt, part, blocks))
    elif request.placebo is not None:
      part = _per_series(request.placebo, len(series_inputs))
      placebo = _with_placebo_seen(series_inputs, part, _host_placebo_summaries(series_inputs, draws, part)
                                   if on_host else _device_placebo_summaries(flt, part, blocks))
    if request.link:
      effect = dict(effect, value_mean=sess.value_mean(request.scale, request.shift))
    return SummaryRecord(effect=effect, components=components, predictions=predictions, windows=windows,
                         placebo=placebo)
  finally:
    if flt is not None and flt is not sess:
      flt.close()


def _model_mask(ci_data) -> np.ndarray:
  """[T] bool: the steps the model does not condition on -- the missing pre-period values and, as
  missing observations, everything after the pre-period (forecasting == sampling, :548-562)."""
  return np.concatenate([np.asarray(ci_data.outcome_ts.is_missing, bool),
                         np.ones(ci_data.model_after_pre_data.shape[0], bool)])


def _run_sampler(*, ci_data, prior_level_sd, seed, num_results, num_warmup_steps, model=None,
                 dtype=np.float32, seasons=(), num_chains=1, devices=None,
                 local_linear_trend=False, sampler="gibbs", request: Optional[SummaryRequest] = None,
                 hmc_init="gibbs", hmc_prior="slab", kernel_flags=0, placebo_sink=None, sink_simulated=None):
  """_train_causalimpact_sts plus the `SummaryRecord` of `request` (on the caller's scale; None: an
  empty record), the record of ONE series (`SummaryRecord.of_series`).  On one device, with the
  float32 Gibbs sampler and unless `request.on_device` is off or it wants the trajectories kept, the
  fit stays in a session for `take_summaries`; the [draws, T] trajectories then stay in HBM and are
  returned as None.  On every other route the draws are pooled on the host: the effect and its
  windows run the same kernels on the same values (`_native.summarize_draws`,
  `_native.window_totals_host`; left out with `request.on_device` off), prediction errors and placebo
  forecasts are filtered by a session made from the pooled parameter draws (`open_draws_session` on
  the first device; in numpy with `request.on_device` off and for a state `draws_filter_route` does
  not take), and the components stay None for the caller's pooled draws."""
  if model is not None:
    raise NotImplementedError("custom tfp.sts models are not supported by the HIP path")
  seed_pair = _sanitize_seed(seed)
  np_dtype = cid._as_numpy_dtype(dtype)  # pylint: disable=protected-access
  # dtype (reference :159: the sampler runs in DataOptions.dtype).  float32 (the default): the
  # latency / time-parallel kernels, on an INTERNALLY CONDITIONED copy of a raw-scale outcome (see
  # `_internal_conditioning`: an exact reparametrisation that keeps every quantity the float32
  # scans touch O(1), mapped back in float64).  float64: the Gibbs sampler runs in float64 on the
  # sequential one-wavefront kernel (csrc/ci_gibbs64.h; draw for draw equal to the float64 oracle
  # to ~1e-9, tests/test_gpu_float64.py); slower -- it is the precision option.  The HMC
  # extension computes in float32 for either dtype.
  design = None if ci_data.feature_ts is None else np.asarray(ci_data.feature_ts.values,
                                                              dtype=np.float64)    # :545-546
  # Post-period handled as missing observations: forecasting == sampling (:548-562).
  n_after = ci_data.model_after_pre_data.shape[0]
  y = np.concatenate([_outcome_float64(ci_data), np.full(n_after, np.nan)])
  mask = _model_mask(ci_data)
  T = y.shape[0]
  cond_mu, cond_s = _internal_conditioning(ci_data)
  if (cond_mu, cond_s) != (0.0, 1.0):
    y = (y - cond_mu) / cond_s
  outcome_sd = float(np.nanstd(y[:T - n_after], ddof=1))
  num_seasons, season_change = _model.expand_seasons(seasons, T)
  params = _model.series_params(y, mask, design, prior_level_sd=prior_level_sd,
                                num_seasonal_blocks=len(num_seasons),
                                has_slope=local_linear_trend, outcome_sd=outcome_sd)
  params["weights_prior_scale"] = cond_s * cond_s     # Omega in the conditioned units (exact map)
  P = 0 if design is None else design.shape[1]
  if P > 0:
    # the spike-and-slab branch clips the VARIANCE at upper_bound = 1.2 sd, a scale (:442-443 as
    # the sampler reads it): var <= 1.2 sd  <=>  var' <= 1.2 sd / s^2 in the conditioned units
    params["obs_ub"] = params["obs_ub"] / cond_s
  K = len(num_seasons)

  if sampler not in ("gibbs", "hmc"):
    raise ValueError(f"sampler must be 'gibbs' or 'hmc', got {sampler!r}")
  devs = list(devices) if devices else [0]
  shares = np.array_split(np.arange(num_chains), len(devs))
  # the float64 Gibbs kernels read the outcome and the design in float64, every other sampler in float32
  inputs = [SeriesInputs(y, mask, design, season_change, num_seasons, local_linear_trend, params,
                         np.float64 if np_dtype == np.float64 and sampler == "gibbs" else np.float32)]
  internal = None if request is None else _request_in_internal_units(request, cond_mu, cond_s)
  record = SummaryRecord()
  def run_on(dev, chain_ids):
    """One device's share of the chains (chain ids keep their global RNG streams)."""
    nonlocal record
    if sampler == "hmc":
      from causalimpact import _hmc  # pylint: disable=import-outside-toplevel
      res = _hmc.fit_hmc(y, mask, design, params, has_slope=local_linear_trend,
                         num_results=num_results, num_warmup=num_warmup_steps,
                         num_chains=len(chain_ids), seed=seed_pair, device=dev,
                         chain_offset=int(chain_ids[0]), init=hmc_init, prior=hmc_prior,
                         horseshoe_scale=0.1 / cond_s, num_seasons=num_seasons,
                         season_change=season_change)
      return {k: v for k, v in res.items() if not k.startswith("hmc_")}
    pb = _native.make_problem(T=T, P=P, has_slope=local_linear_trend, num_seasons=num_seasons,
                              num_warmup=num_warmup_steps, num_results=num_results,
                              num_chains=len(chain_ids), chain_offset=int(chain_ids[0]),
                              seed=seed_pair, device=dev, flags=int(kernel_flags))
    if np_dtype == np.float64:
      # float64 compute (csrc/ci_gibbs64.h): the sequential kernel, every buffer float64
      return _native.fit_gibbs_f64(pb, y[None], mask[None], None if design is None else design[None],
                                   season_change, _native.make_params([params]))
    if internal is not None and internal.on_device and len(devs) == 1 and not internal.keep_trajectories:
      sess = _native.Session(pb, y[None], mask[None], None if design is None else design[None],
                             season_change, _native.make_params([params]))
      try:
        # the draws travel to (pinned) host memory while the sampler runs; the trajectories stay
        # on the device for the summary kernels
        _, part = sess.run_streamed(
            want=[k for k in _native._OUT_FIELDS  # pylint: disable=protected-access
                  if k != "posterior_trajectories" and (k != "slope" or local_linear_trend)],
            chunk_draws=32)
        record = take_summaries(sess, internal, inputs)
      finally:
        sess.close()
      return part
    return _native.fit_gibbs(pb, y[None], mask[None], None if design is None else design[None],
                             season_change, _native.make_params([params]))

  parts = map_by_device(lambda a: run_on(*a),
                        [(dev, ids) for dev, ids in zip(devs, shares) if len(ids)])
  out = ({k: v[0] for k, v in parts[0].items()} if len(parts) == 1 else              # [C, ...]
         {k: np.concatenate([p[k][0] for p in parts], axis=0) for k in parts[0]})

  if internal is not None and record.effect is None:
    # draws pooled on the host (several devices, the float64 kernels, the HMC path): the summary
    # kernels read float32 trajectories, so they get them in the INTERNAL (conditioned) units --
    # O(1) values -- with the map to the caller's scale folded into (scale, shift) in float64, as
    # on the single-device path.  Summarising the rescaled draws would round the offset back in
    # (8e-6 steps at y ~ 100).
    effect = windows = predictions = placebo = None
    tr = out["posterior_trajectories"]
    tr = tr.reshape((1, tr.shape[0] * tr.shape[1]) + tr.shape[2:])
    own = Affine(internal.scale, internal.shift)
    if internal.link and (internal.on_device or internal.paths is not None):
      # under a link: the draws on the data scale, in float64, before anything is summed or uploaded
      # (`_native.link_values_host`); what follows reads them as they are
      tr = _native.link_values_host(
          tr.astype(np.float64) * np.float64(internal.scale) + np.float64(internal.shift), internal.link)
      own = Affine(1.0, 0.0)
    if internal.on_device:
      effect = {k: v[None] for k, v in _native.summarize_draws(
          tr[0], *own, internal.observed, internal.flags, internal.ranks, device=devs[0]).items()}
      if internal.link:
        effect["value_mean"] = tr.mean(axis=1)
      if internal.windows is not None:
        # ... and the window totals from exactly these trajectories and this (scale, shift)
        windows = dict(per_draw=_native.window_totals_host(tr, *own, internal.observed, *internal.windows))
    if internal.paths is not None:
      # ... and the path excursions, also where the effect is left to `_compute_impact`
      windows = dict(windows or {}, **_paths_record(_native.path_excursions_host(
          tr, *own, internal.observed, *internal.paths, ranks=internal.path_ranks)))
    # the same definitions from the parameter draws in the sampler's units: filtered by the kernels of a
    # fit's session through a session made from the draws (`draws_filter_route`), else in numpy
    draws = {k: out[k][None] for k in _PARAMETER_DRAWS}
    route = "host"
    if internal.predictions is not None or internal.placebo is not None:
      route = draws_filter_route(local_linear_trend, num_seasons, internal.on_device)
    drawn = None if route == "host" else open_draws_session(inputs, draws, seed=seed_pair, device=devs[0])
    try:
      blocks = route == "blocks"
      if internal.predictions is not None:
        if drawn is None:
          predictions = _host_prediction_summaries(inputs, draws, internal.predictions, internal.ranks)
        else:
          entry = drawn.summarize_predictions_blocks if blocks else drawn.summarize_predictions
          predictions = entry(*internal.predictions, internal.ranks)
      if internal.placebo is not None and internal.placebo.quantiles is not None:
        part = _per_series(internal.placebo, 1)
        placebo = _simulated_placebo_summaries(
            inputs, part, internal.observed, int(np.prod(draws["observation_noise_scale"].shape[1:3])),
            _host_placebo_simulations(inputs, draws, part) if drawn is None else
            _device_placebo_simulations(drawn, part, blocks))
      elif internal.placebo is not None:
        part = _per_series(internal.placebo, 1)
        placebo = _with_placebo_seen(inputs, part, _host_placebo_summaries(inputs, draws, part)
                                     if drawn is None else _device_placebo_summaries(drawn, part, blocks))
    finally:
      if drawn is not None:
        drawn.close()
    record = SummaryRecord(effect=effect, predictions=predictions, windows=windows, placebo=placebo)
  if placebo_sink is not None:
    # (batch.py, pooled placebo forecasts: the per-draw terms from the parameter draws in the
    #  sampler's units, mapped to the caller's scale like every other summary)
    draws = {k: out[k][None] for k in _PARAMETER_DRAWS}
    pooled = _pooled_draws(draws, 0)
    route = draws_filter_route(local_linear_trend, num_seasons, internal.on_device)
    drawn = None if route == "host" else open_draws_session(inputs, draws, seed=seed_pair, device=devs[0])
    try:
      if drawn is not None:                # (the same terms through the kernels of a fit's session)
        placebo_sink(lambda origins, horizon, horizons=None: _placebo_entry_device(
            drawn, route == "blocks", inputs[0], internal.scale, internal.shift, internal.observed, origins,
            horizon, sink_simulated, horizons))
      elif sink_simulated is not None:     # (link, stream): the simulated totals in place of the moments
        placebo_sink(lambda origins, horizon: _placebo_entry_simulated_host(
            inputs[0], pooled, internal.scale, internal.shift, internal.observed, origins, horizon, *sink_simulated))
      else:
        placebo_sink(lambda origins, horizon, horizons=None: _placebo_entry_host(
            inputs[0], pooled, internal.scale, internal.shift, internal.observed, origins, horizon, horizons))
    finally:
      if drawn is not None:
        drawn.close()
  if record.components is not None and cond_s != 1.0:
    # the weights on the caller's model scale, as in `samples`
    record = dataclasses.replace(record, components={
        k: v * cond_s if k in ("weight_mean", "weight_order") else v for k, v in record.components.items()})
  if (cond_mu, cond_s) != (0.0, 1.0):
    # back to the caller's scale, in float64: locations get the offset, everything else the scale
    out = {k: np.asarray(v, np.float64) * cond_s for k, v in out.items()}
    for k in ("level", "posterior_means", "posterior_trajectories"):
      if k in out:
        out[k] += cond_mu

  def pool(a):   # [C, S, ...] -> [C*S, ...]
    return a.reshape((a.shape[0] * a.shape[1],) + a.shape[2:]).astype(np_dtype, copy=False)

  samples = dict(
      observation_noise_scale=pool(out["observation_noise_scale"]),
      level_scale=pool(out["level_scale"]), slope_scale=pool(out["slope_scale"]),
      weights=pool(out["weights"]), level=pool(out["level"]),
      slope=pool(out["slope"]) if "slope" in out else None,
      seasonal_drift_scales=pool(out["seasonal_drift_scales"]),
      seasonal_levels=pool(out["seasonal_levels"]))
  assert samples["weights"].shape[-1] == P and samples["seasonal_levels"].shape[-1] == K
  if num_chains > 1:
    scalars = {k: out[k] for k in ("observation_noise_scale", "level_scale")}
    samples["diagnostics"] = _LazyMapping(
        lambda: dict(_diagnostics.summarize(scalars), num_chains=num_chains))
  # the predictive arrays feed the data-scale summaries: with internal conditioning they carry the
  # offset again and stay float64 (float32 would round 100.0001 to 8e-6 steps)
  pred_dtype = np.float64 if (cond_mu, cond_s) != (0.0, 1.0) else np_dtype
  posterior_means = out["posterior_means"].mean(axis=0).astype(pred_dtype, copy=False)    # :627
  posterior_trajectories = None
  if "posterior_trajectories" in out:                                                     # :631
    tr = out["posterior_trajectories"]
    posterior_trajectories = tr.reshape((tr.shape[0] * tr.shape[1],) + tr.shape[2:]).astype(
        pred_dtype, copy=False)
  return samples, posterior_means, posterior_trajectories, record.of_series(0)


# --------------------------------------------------------------------------------------
# impact post-processing (reference :635-1093) -- numpy inside, the reference's frames outside
# --------------------------------------------------------------------------------------
def _compute_impact(posterior_means, posterior_trajectories, ci_data: cid.CausalImpactData,
                    alpha: float = 0.05, windows: Optional[Sequence[EffectWindow]] = None):
  """(series, summary) from the sampler's predictive draws (reference :635-705); with `windows`
  (series, summary, window_summary), the summary of every `EffectWindow` over its own rows."""
  if not 0 < alpha < 1:
    raise ValueError("`alpha` must be between 0 and 1.")
  observed_pre = ci_data.pre_data[ci_data.outcome_column]
  observed_post = ci_data.after_pre_data[ci_data.outcome_column]
  in_post = (observed_post.index >= ci_data.post_period[0]) & (observed_post.index <=
                                                              ci_data.post_period[1])
  observed_post = observed_post.loc[in_post]
  observed_full = pd.concat([observed_pre, observed_post], axis=0)
  quantiles = (alpha / 2.0, 1.0 - alpha / 2.0)
  trajectories, trajectory_summary = _sample_posterior_predictive(
      posterior_means=posterior_means, posterior_trajectories=posterior_trajectories,
      ci_data=ci_data, quantiles=quantiles)
  trajectory_dict = _compute_impact_trajectories(trajectories, observed_full,
                                                 treatment_start=ci_data.post_period[0])
  series = _compute_impact_estimates(posterior_trajectory_summary=trajectory_summary,
                                     trajectory_dict=trajectory_dict,
                                     observed_ts_full=observed_full, ci_data=ci_data,
                                     quantiles=quantiles)
  summary = _compute_summary(posterior_trajectory_summary=trajectory_summary,
                             trajectory_dict=trajectory_dict, observed_ts_post=observed_post,
                             post_period=ci_data.post_period, quantiles=quantiles, alpha=alpha)
  if windows is None:
    return series, summary
  window_summary = _window_tables(windows, lambda _, win: _compute_summary(
      posterior_trajectory_summary=trajectory_summary, trajectory_dict=trajectory_dict,
      observed_ts_post=observed_post, post_period=(win.start, win.end), quantiles=quantiles,
      alpha=alpha))
  return series, summary, window_summary


def _observed_series(ci_data: cid.CausalImpactData):
  observed_pre = ci_data.pre_data[ci_data.outcome_column]
  observed_post = ci_data.after_pre_data[ci_data.outcome_column]
  in_post = (observed_post.index >= ci_data.post_period[0]) & (observed_post.index <=
                                                              ci_data.post_period[1])
  observed_post = observed_post.loc[in_post]
  return observed_post, pd.concat([observed_pre, observed_post], axis=0)


def _quantile_ranks(num_draws: int, quantiles):
  """numpy's 'linear' quantile of n values: lerp(x_(lo), x_(lo+1), gamma) -- the order
  statistics it needs and the interpolation weight (numpy/lib/_function_base_impl.py
  _quantile: virtual index q (n - 1), previous = floor, next = previous + 1 clipped)."""
  out = []
  for q in quantiles:
    virtual = (num_draws - 1) * np.float64(q)
    lo = int(np.floor(virtual))
    if lo >= num_draws - 1:
      lo, hi, gamma = num_draws - 1, num_draws - 1, np.float64(0.0)
    else:
      hi, gamma = lo + 1, virtual - lo
    out.append((lo, hi, gamma))
  return out


def _summary_ranks(num_draws: int, quantiles) -> List[int]:
  """Order statistics the two quantiles need, and their mirror images (effect = observed - value
  reverses the order)."""
  qs = _quantile_ranks(num_draws, quantiles)
  return sorted({r for lo, hi, _ in qs for r in (lo, hi)} |
                {num_draws - 1 - r for lo, hi, _ in qs for r in (lo, hi)})


def _device_summary_request(ci_data: cid.CausalImpactData, alpha: float) -> Dict:
  """Arguments of ci_session_summarize for this analysis (see include/causalimpact_amd.h)."""
  _, observed_full = _observed_series(ci_data)
  idx = posterior_processing.model_index(ci_data)
  obs = observed_full.reindex(idx).to_numpy(dtype=np.float64)
  after_start = ~np.asarray(idx < ci_data.post_period[0])
  window = np.asarray((idx >= ci_data.post_period[0]) & (idx <= ci_data.post_period[1]))
  if ci_data.standardize_data:
    scale = float(np.ravel(ci_data.outcome_scaler.stddev_)[0])
    shift = float(np.ravel(ci_data.outcome_scaler.mean_)[0])
  else:
    scale, shift = 1.0, 0.0
  return dict(scale=scale, shift=shift, observed=obs,
              flags=after_start.astype(np.uint8) | (window.astype(np.uint8) << 1),
              quantiles=(alpha / 2.0, 1.0 - alpha / 2.0))


def _lerp_order_stats(order: Dict[int, np.ndarray], lo: int, hi: int, gamma) -> np.ndarray:
  """numpy's own interpolation of two order statistics (so results match np.quantile bit for
  bit): the quantile of the 2-point sample {x_(lo), x_(hi)} at `gamma` is lerp(x_lo, x_hi, gamma)."""
  pair = np.stack([order[lo], order[hi]])
  with np.errstate(invalid="ignore"):
    return np.quantile(pair, gamma, axis=0)


def _per_draw_means(pred_sum, point_sum, num_steps: int, num_observed: int) -> Dict[str, np.ndarray]:
  """The per-draw window means and totals `_compute_summary` takes, from the totals over a window of
  `num_steps` steps of which `num_observed` have an observation."""
  with np.errstate(invalid="ignore", divide="ignore"):
    return dict(pred_mean=pred_sum / num_steps, pred_sum=pred_sum,
                point_mean_t=point_sum / num_observed if num_observed else
                np.full_like(point_sum, np.nan),
                point_sum_t=point_sum)


def _compute_impact_device(posterior_means, device_summary: Dict, obs: np.ndarray, flags: np.ndarray,
                           ranks: Sequence[int], ci_data: cid.CausalImpactData, alpha: float,
                           windows: Optional[Sequence[EffectWindow]] = None, window_totals=None):
  """(series, summary) from the on-device summary (csrc/ci_summary.h) -- same frames as
  _compute_impact, which stays the host reference of this arithmetic.  obs, flags [T] and ranks: what
  the summary was taken with.  With `windows` (series, summary, window_summary): the summary of every
  `EffectWindow` from `window_totals` [W, 2, N], every draw's totals over it (csrc/ci_windows.h)."""
  quantiles = (alpha / 2.0, 1.0 - alpha / 2.0)
  observed_post, observed_full = _observed_series(ci_data)
  idx = posterior_processing.model_index(ci_data)
  ranks = list(ranks)
  num_draws = device_summary["per_draw"].shape[1]
  value_order = {r: device_summary["value_order"][i] for i, r in enumerate(ranks)}
  cum_order = {r: device_summary["cum_order"][i] for i, r in enumerate(ranks)}
  (lo_a, hi_a, g_a), (lo_b, hi_b, g_b) = _quantile_ranks(num_draws, quantiles)

  def frame(prefix, lower, upper):
    return pd.DataFrame({prefix + "_lower": lower, prefix + "_upper": upper}, index=idx)

  means = posterior_processing.process_posterior_quantities(ci_data, posterior_means,
                                                            ["posterior_mean"])
  trajectory_summary = means.join(frame("posterior",
                                        _lerp_order_stats(value_order, lo_a, hi_a, g_a),
                                        _lerp_order_stats(value_order, lo_b, hi_b, g_b)))
  # point effect = -(value - observed) is decreasing in the value: its k-th smallest is the
  # (N-1-k)-th smallest value, mapped
  mirrored = {k: -(value_order[num_draws - 1 - k] - obs) for k in {lo_a, hi_a, lo_b, hi_b}}
  bands = {
      "point_effects": frame("point_effects", _lerp_order_stats(mirrored, lo_a, hi_a, g_a),
                             _lerp_order_stats(mirrored, lo_b, hi_b, g_b)),
      "cumulative_effects": frame("cumulative_effects",
                                  _lerp_order_stats(cum_order, lo_a, hi_a, g_a),
                                  _lerp_order_stats(cum_order, lo_b, hi_b, g_b)),
  }
  series = _compute_impact_estimates(posterior_trajectory_summary=trajectory_summary,
                                     trajectory_dict=None, observed_ts_full=observed_full,
                                     ci_data=ci_data, quantiles=quantiles, bands=bands)
  window = (flags & 2) != 0
  n_obs_window = int(np.sum(~np.isnan(obs[window])))
  pred_sum, point_sum = device_summary["per_draw"]
  per_draw = _per_draw_means(pred_sum, point_sum, int(window.sum()), n_obs_window)
  summary = _compute_summary(posterior_trajectory_summary=trajectory_summary,
                             trajectory_dict=None, observed_ts_post=observed_post,
                             post_period=ci_data.post_period, quantiles=quantiles, alpha=alpha,
                             per_draw=per_draw)
  if windows is None:
    return series, summary

  def table_of(w, win):
    steps = slice(win.first, win.first + win.count)
    totals = window_totals[w]
    return _compute_summary(
        posterior_trajectory_summary=trajectory_summary, trajectory_dict=None,
        observed_ts_post=observed_post, post_period=(win.start, win.end), quantiles=quantiles,
        alpha=alpha, per_draw=_per_draw_means(totals[0], totals[1], win.count,
                                              int(np.sum(~np.isnan(obs[steps])))))

  return series, summary, _window_tables(windows, table_of)


def _sample_posterior_predictive(posterior_means, posterior_trajectories,
                                 ci_data: cid.CausalImpactData, quantiles: Tuple[float, float]):
  """Data-scale trajectories (T x draws) and their mean/quantile summary (reference :708-767)."""
  if any((q < 0) | (q > 1) for q in quantiles):
    raise ValueError("All elements of `quantiles` must be in (0, 1). Got %s" % (quantiles,))
  if quantiles[0] > quantiles[1]:
    raise ValueError("`quantiles` must be sorted in ascending order. Got %s" % (quantiles,))
  means = posterior_processing.process_posterior_quantities(ci_data, posterior_means,
                                                            ["posterior_mean"])
  trajectories = _package_posterior_trajectories(posterior_trajectories, ci_data)
  bands = posterior_processing.calculate_trajectory_quantiles(trajectories, "posterior", quantiles)
  return trajectories, means.join(bands)


def _package_posterior_trajectories(posterior_trajectories,
                                    ci_data: cid.CausalImpactData) -> pd.DataFrame:
  """[draws, T] -> T x draws frame named sample_1..sample_n, unscaled (reference :770-790)."""
  names = [f"sample_{i + 1}" for i in range(np.shape(posterior_trajectories)[0])]
  return posterior_processing.process_posterior_quantities(ci_data, posterior_trajectories, names)


def _compute_impact_trajectories(posterior_trajectories: pd.DataFrame,
                                 observed_ts_full: pd.Series,
                                 treatment_start: OutputDateType) -> Dict[str, pd.DataFrame]:
  """Per-draw point effects (observed - predicted) and their running sum from the treatment
  start; NaN observations give NaN effects and are skipped by the running sum
  (reference :793-837)."""
  idx, cols = posterior_trajectories.index, posterior_trajectories.columns
  pred = posterior_trajectories.to_numpy(dtype=np.float64)
  obs = observed_ts_full.reindex(idx).to_numpy(dtype=np.float64)
  point = -(pred - obs[:, None])
  base = np.where(np.asarray(idx < treatment_start)[:, None], 0.0, point)
  holes = np.isnan(base)
  cumulative = np.cumsum(np.where(holes, 0.0, base), axis=0)
  cumulative[holes] = np.nan
  return {
      "predictions": posterior_trajectories,
      "point_effects": pd.DataFrame(point, index=idx, columns=cols),
      "cumulative_effects": pd.DataFrame(cumulative, index=idx, columns=cols),
  }


def _compute_impact_estimates(posterior_trajectory_summary: pd.DataFrame,
                              trajectory_dict: Dict[str, pd.DataFrame],
                              observed_ts_full: pd.Series, ci_data: cid.CausalImpactData,
                              quantiles: Tuple[float, float],
                              bands: Optional[Dict[str, pd.DataFrame]] = None) -> pd.DataFrame:
  """The 14-column `series` frame over the full input index (reference :840-931).  `bands`:
  precomputed quantile frames of the effect trajectories (on-device summary)."""
  if bands is None:
    bands = {k: posterior_processing.calculate_trajectory_quantiles(trajectory_dict[k], k,
                                                                    quantiles)
             for k in ("point_effects", "cumulative_effects")}
  idx = posterior_trajectory_summary.index
  obs_s = observed_ts_full.reindex(idx)
  obs = obs_s.to_numpy(dtype=np.float64)
  pm = posterior_trajectory_summary["posterior_mean"]
  if not (pm.dtype == np.float64 and obs_s.dtype == np.float64 and
          all(b[c].dtype == np.float64 for b in bands.values() for c in b.columns) and
          all(b.index.equals(idx) for b in bands.values())):
    return _compute_impact_estimates_frames(posterior_trajectory_summary, observed_ts_full,
                                            ci_data, bands)
  # float64 throughout (every ordinary call): the columns as arrays, ONE frame at the end -- the same
  # IEEE operations as the frame-by-frame version below (tests/test_golden_postprocessing.py pins
  # both against the reference's output), 4 ms -> 1 ms of host time per fit
  point_mean = obs - pm.to_numpy()
  base = np.where(idx < ci_data.post_period[0], 0.0, point_mean)
  hole = np.isnan(base)
  cum_mean = np.cumsum(np.where(hole, 0.0, base))          # skips NaN like the reference
  cum_mean[hole] = np.nan
  # between pre- and post-period, and after the post-period: predictions only (:899-907);
  # no observation => no effect (NaN, not 0) (:909-915)
  blank = np.asarray(((idx > ci_data.pre_period[1]) & (idx < ci_data.post_period[0])) |
                     (idx > ci_data.post_period[1])) | np.isnan(obs)

  def effect(v):
    v = np.array(v, dtype=np.float64)
    v[blank] = np.nan
    return v

  cols = {"observed": obs}
  for c in posterior_trajectory_summary.columns:
    cols[c] = posterior_trajectory_summary[c].to_numpy()
  cols["point_effects_mean"] = effect(point_mean)
  for c in bands["point_effects"].columns:
    cols[c] = effect(bands["point_effects"][c].to_numpy())
  cols["cumulative_effects_mean"] = effect(cum_mean)
  for c in bands["cumulative_effects"].columns:
    cols[c] = effect(bands["cumulative_effects"][c].to_numpy())
  for c in posterior_trajectory_summary.columns:           # any summary column beyond the kept ones
    if c not in _KEPT_AFTER_POST:
      cols[c] = effect(cols[c])
  if idx.equals(ci_data.data.index):                        # (the usual case; the input's own index object)
    frame = pd.DataFrame(cols, index=ci_data.data.index)
  else:
    frame = pd.DataFrame(cols, index=idx).reindex(ci_data.data.index, fill_value=np.nan)
  frame["observed"] = ci_data.data[ci_data.outcome_column]
  frame["pre_period_start"] = ci_data.pre_period[0]
  frame["pre_period_end"] = ci_data.pre_period[1]
  frame["post_period_start"] = ci_data.post_period[0]
  frame["post_period_end"] = ci_data.post_period[1]
  return frame


def _compute_impact_estimates_frames(posterior_trajectory_summary, observed_ts_full, ci_data, bands):
  """_compute_impact_estimates frame by frame (any dtypes / band indices)."""
  idx = posterior_trajectory_summary.index
  obs = observed_ts_full.reindex(idx)
  point_mean = obs - posterior_trajectory_summary["posterior_mean"]
  base = point_mean.where(~(idx < ci_data.post_period[0]), 0.0)
  cum_mean = base.cumsum()                                 # skips NaN like the reference
  frame = pd.concat([
      obs.rename("observed"), posterior_trajectory_summary,
      point_mean.rename("point_effects_mean"),
      bands["point_effects"],
      cum_mean.rename("cumulative_effects_mean"),
      bands["cumulative_effects"],
  ], axis=1)
  effect_cols = frame.columns.difference(_KEPT_AFTER_POST)
  # between pre- and post-period, and after the post-period: predictions only (:899-907)
  outside = (((frame.index > ci_data.pre_period[1]) & (frame.index < ci_data.post_period[0])) |
             (frame.index > ci_data.post_period[1]))
  frame.loc[outside, effect_cols] = np.nan
  # no observation => no effect (NaN, not 0) (:909-915)
  frame.loc[np.isnan(frame["observed"].to_numpy(dtype=np.float64)), effect_cols] = np.nan
  frame = frame.reindex(ci_data.data.index, fill_value=np.nan)
  frame["observed"] = ci_data.data[ci_data.outcome_column]
  frame["pre_period_start"] = ci_data.pre_period[0]
  frame["pre_period_end"] = ci_data.pre_period[1]
  frame["post_period_start"] = ci_data.post_period[0]
  frame["post_period_end"] = ci_data.post_period[1]
  return frame


def _summary_rows(post_mean, obs, pred_mean, pred_sum, point_mean_t, point_sum_t, quantiles):
  """The numbers of the `summary` frame (reference :966-1091) from the post-period posterior
  mean [T_w], observations [T_w] and per-draw window means / totals [draws]."""
  obs_mean, obs_sum = float(np.nanmean(obs)), float(np.nansum(obs))

  def sd(v):
    return float(np.std(v, ddof=1))

  def band(v):
    lo, hi = np.quantile(v, quantiles)
    return float(lo), float(hi)

  rel = obs_sum / pred_sum - 1.0
  avg_pred, cum_pred = float(post_mean.mean()), float(post_mean.sum())
  b_pm, b_ps, b_em, b_es, b_rel = (band(pred_mean), band(pred_sum), band(point_mean_t),
                                   band(point_sum_t), band(rel))     # one selection per vector
  rows = {
      "actual": (obs_mean, obs_sum),
      "predicted": (avg_pred, cum_pred),
      "predicted_lower": (b_pm[0], b_ps[0]),
      "predicted_upper": (b_pm[1], b_ps[1]),
      "predicted_sd": (sd(pred_mean), sd(pred_sum)),
      "abs_effect": (obs_mean - avg_pred, obs_sum - cum_pred),
      "abs_effect_lower": (b_em[0], b_es[0]),
      "abs_effect_upper": (b_em[1], b_es[1]),
      "abs_effect_sd": (sd(point_mean_t), sd(point_sum_t)),
      "rel_effect": (float(rel.mean()),) * 2,
      "rel_effect_lower": (b_rel[0],) * 2,
      "rel_effect_upper": (b_rel[1],) * 2,
      "rel_effect_sd": (sd(rel),) * 2,
  }
  # one-sided tail area of the observed total among the sampled totals, the observed total
  # included so that p stays in (0, 1)   (:1077-1091)
  pool = np.append(pred_sum, obs_sum)
  p_value = min(float((obs_sum <= pool).mean()), float((obs_sum >= pool).mean()))
  return rows, p_value


def _compute_summary(posterior_trajectory_summary: pd.DataFrame,
                     trajectory_dict: Dict[str, pd.DataFrame], observed_ts_post: pd.Series,
                     post_period: OutputPeriodType, quantiles: Tuple[float, float],
                     alpha: float, per_draw: Optional[Dict[str, np.ndarray]] = None) -> pd.DataFrame:
  """The 2 x 15 `summary` frame over the post-period (reference :934-1093), or over any window
  inside it handed in as `post_period` (`effect_windows`: observed_ts_post is cut to it like the
  other frames).  `per_draw`: precomputed per-draw window means / totals (on-device summary)."""

  def window(frame):
    keep = (frame.index >= post_period[0]) & (frame.index <= post_period[1])
    return frame.loc[keep]

  post_mean = window(posterior_trajectory_summary)["posterior_mean"].to_numpy(dtype=np.float64)
  obs = window(observed_ts_post).to_numpy(dtype=np.float64)
  if per_draw is None:
    pred = window(trajectory_dict["predictions"]).to_numpy(dtype=np.float64)      # [T_post, draws]
    point = window(trajectory_dict["point_effects"]).to_numpy(dtype=np.float64)
    pred_mean, pred_sum = pred.mean(axis=0), pred.sum(axis=0)
    with np.errstate(invalid="ignore"):
      point_mean_t, point_sum_t = np.nanmean(point, axis=0), np.nansum(point, axis=0)
  else:
    pred_mean, pred_sum = per_draw["pred_mean"], per_draw["pred_sum"]
    point_mean_t, point_sum_t = per_draw["point_mean_t"], per_draw["point_sum_t"]
  rows, p_value = _summary_rows(post_mean, obs, pred_mean, pred_sum, point_mean_t, point_sum_t,
                                quantiles)
  summary = pd.DataFrame({k: {"average": v[0], "cumulative": v[1]} for k, v in rows.items()})
  summary["p_value"] = p_value
  summary["alpha"] = alpha
  return summary
