/*
 * causalimpact_amd.h -- C-ABI of the MI355X-native CausalImpact hot path.
 *
 * The reference (google/tfp-causalimpact) has no FFI: its hot path is the
 * Python call
 *     _train_causalimpact_sts(...)            causalimpact/causalimpact_lib.py:503-606
 *       -> _run_gibbs_sampler(...)            causalimpact/causalimpact_lib.py:345-395
 *            gibbs_sampler.fit_with_gibbs_sampling(...)          :365-388
 *            _get_posterior_means_and_trajectories(...)          :609-632
 * into TensorFlow-Probability.  This header is the boundary a maintainer would
 * bind instead (ctypes stub: INTEGRATION.md).  Plain pointers and sizes only;
 * the caller owns every host buffer; the library keeps no caller pointers after
 * a call returns.  All entry points return 0 on success, non-zero on error;
 * ci_last_error() then describes the failure (thread-local string).
 *
 * Shapes use the reference's names:  T = time steps handed to the sampler
 * (pre-period + everything after it, causalimpact_lib.py:548-562), P = design
 * columns incl. the trailing intercept (data.py:135), K = seasonal blocks,
 * W/S = warm-up / retained Gibbs iterations, C = chains, B = independent series.
 */
#ifndef CAUSALIMPACT_AMD_H_
#define CAUSALIMPACT_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CI_ABI_VERSION 5
#define CI_MAX_BLOCKS 8

/* Per-series priors and initial Gibbs state.  One per series because every
 * constant scales with that series' outcome_sd.
 * Replaces the prior objects built in _build_default_gibbs_model
 * (causalimpact_lib.py:424-489) and the initial GibbsSamplerState
 * (causalimpact_lib.py:566-581, :370-383). */
typedef struct ci_series_params {
  double level_conc, level_scale, level_ub;   /* IG(sigma^2_level); clip on sigma   :424-432 */
  double slope_conc, slope_scale, slope_ub;   /* IG(sigma^2_slope) (LocalLinearTrend only) */
  double obs_conc, obs_scale, obs_ub;         /* IG(sigma^2_obs); upper bound        :434-443 */
  double drift_conc, drift_scale, drift_ub;   /* IG(sigma^2_drift), all blocks       :472-474 */
  double nonzero_prob;                        /* min(1, 3/P)                         :449-450 */
  double init_level_loc, init_level_scale;    /* N(y[0], sd)                         :467-469 */
  double init_slope_scale;                    /* N(0, .)  (LocalLinearTrend only) */
  double init_seasonal_scale;                 /* N(0, sd)                            :489     */
  double obs_scale0, level_scale0, slope_scale0;  /* initial state                   :566-572 */
  double drift_scale0[CI_MAX_BLOCKS];             /*                                 :573-574 */
  /* Multiplier of the weights-prior precision Omega = 0.01 (X'X/2 + diag(X'X)/2) / T (:451-453,
   * built on the device from X); 1 = the reference's prior.  The host package conditions a raw-
   * scale outcome as y -> (y - mu) / s before the float32 kernels see it and passes s^2 here:
   * Omega is then in the conditioned units and the chain is the reference's chain, mapped
   * (causalimpact_lib._internal_conditioning).  Must be positive. */
  double weights_prior_scale;
} ci_series_params;

/* The sampler's static configuration == the non-tensor arguments of
 * _run_gibbs_sampler (causalimpact_lib.py:346-353) plus the batch extensions
 * BASELINE.json asks for (chains, series). */
typedef struct ci_problem {
  int32_t abi_version;          /* CI_ABI_VERSION */
  int32_t T, P;
  int32_t has_slope;            /* 0 LocalLevel (reference default), 1 LocalLinearTrend */
  int32_t num_blocks;           /* K seasonal blocks */
  int32_t num_seasons[CI_MAX_BLOCKS];
  int32_t num_warmup;           /* W   InferenceOptions.num_warmup_steps :215-220 */
  int32_t num_results;          /* S   InferenceOptions.num_results */
  int32_t num_chains;           /* C chains run by THIS call (per series) */
  int32_t chain_offset;         /* global id of this call's first chain: results do not
                                   depend on how chains are split over devices */
  int32_t num_series;           /* B */
  uint32_t seed[2];             /* sanitized seed pair (int s -> (0,s)) :535-543 */
  int32_t device;               /* HIP device ordinal */
  int32_t flags;                /* CI_FLAG_* (0 = let the library choose the kernel) */
  int32_t series_offset;        /* global id of this call's first series: series b draws from the
                                   random streams of series id series_offset + b, so a batch split
                                   over devices gives the same draws as one launch, and the
                                   Monte-Carlo errors of different series are independent.  Series
                                   id 0 (any single-series fit) uses the plain chain streams. */
  int32_t reserved;             /* 0 */
} ci_problem;

/* Seasonal models (and any model with more than 52 design columns): use the one-wavefront-per-chain
 * sequential kernel even where a time-parallel kernel applies.  The route of a fit is otherwise a
 * function of the model and the series alone -- never of the launch size or the device -- so this
 * flag must be given to a batch and to the single-series fit it is compared with alike.  Higher
 * throughput for batches of hundreds of short multi-block series; test / diagnostic knob. */
#define CI_FLAG_SEQUENTIAL_SEASONAL 1
/* Batches: every series consumes the random streams of series 0 (series b of the batch then
 * reproduces a single-series fit of series b draw for draw; Monte-Carlo errors are perfectly
 * correlated across the batch).  Off by default. */
#define CI_FLAG_SHARED_SERIES_STREAMS 2
/* Use the four-wavefront Gibbs kernel where the eight-wavefront latency build (four time waves,
 * a regression wave that sweeps the next iteration's matrix during the Durbin-Koopman draw, three
 * randomness waves) would be chosen.  Same sampler, random stream and roundings: the two builds
 * give bit-identical draws, so this only changes the timing; test / diagnostic knob. */
#define CI_FLAG_FOUR_WAVES 4
/* Sequential seasonal kernel: keep its arrays over time in the per-chain HBM workspace even when
 * they would fit in LDS (the library does so by itself for long series / many covariates).
 * Test / diagnostic knob. */
#define CI_FLAG_SEASONAL_WORKSPACE 8
/* Time-parallel kernels: one workgroup per chain even where the library would spread a chain over a
 * cluster of 2, 4, 8 or 16 CUs (csrc/ci_wide.h: the Durbin-Koopman draw on up to eight of them, the
 * streaming phases on all; csrc/ci_seasonal_tp.h: up to 32) because the launch leaves CUs idle.
 * Every cluster size gives the same bits; test / diagnostic knob. */
#define CI_FLAG_NO_CLUSTER 16
/* Test knob: the last workgroup of every cluster exits at once, as if it had never been
 * scheduled -- the others must notice (time-out while assembling the cluster) and the chain's
 * main workgroup must carry on alone with unchanged results. */
#define CI_FLAG_TEST_DROP_HELPER 32
/* Seasonal models: take the wave-cooperative time-parallel kernel (csrc/ci_seasonal_tp.h: chunks of
 * the series on the wavefronts of a cluster of up to 32 workgroups of 4 wavefronts, any block list with a state of at
 * most 32 components) even for "trend + one block of 2-7 seasons" and for trend models with 53+
 * design columns, which by default run on the quad-split kernel of csrc/ci_wide.h (the faster one
 * since round 6: profiles/).  Test / diagnostic knob. */
#define CI_FLAG_CLUSTER_SEASONAL 64
/* Seasonal models with a state of at most 64 components: run on the multi-wavefront build of the
 * sequential kernel (csrc/ci_seasonal_mw.h), which every state of 65-256 components takes anyway.
 * Same model, same random numbers; the sums differ from the one-wavefront kernel's only in float
 * summation order.  Test / diagnostic knob. */
#define CI_FLAG_MULTIWAVE_SEASONAL 128

/* Caller-allocated result buffers (float32, chain-major so per-device shards
 * are contiguous).  == GibbsSamplerState stack + (means, trajectories) returned
 * at causalimpact_lib.py:395.  Any pointer may be NULL to skip that output. */
typedef struct ci_outputs {
  float* observation_noise_scale;  /* [B,C,S]   */
  float* level_scale;              /* [B,C,S]   */
  float* slope_scale;              /* [B,C,S]   */
  float* seasonal_drift_scales;    /* [B,C,S,K] */
  float* weights;                  /* [B,C,S,P] */
  float* level;                    /* [B,C,S,T] */
  float* slope;                    /* [B,C,S,T] */
  float* seasonal_levels;          /* [B,C,S,T,K]  0-th latent of each block (:312-317) */
  float* posterior_means;          /* [B,C,T]   per-chain mean of the noise-free predictor (:627) */
  float* posterior_trajectories;   /* [B,C,S,T] (:629-631) */
} ci_outputs;

typedef struct ci_session ci_session;  /* device-resident fit: inputs + outputs live in HBM */

const char* ci_last_error(void);
int ci_abi_version(void);
int ci_device_count(int* count);
/* The Philox key of series `series_id` of a fit with `seed`: key = (seed[0] ^ h1(id), seed[1] ^
 * h2(id)), h1 / h2 bijective mixers that fix 0 -- series 0 (every single-series fit) keeps the
 * plain seeds, and batches under different seeds never share a stream.  A single-series fit with
 * seed = key reproduces series `series_id` of the batch (what the parity tests feed the oracle). */
void ci_series_stream_key(const uint32_t seed[2], int32_t series_id, uint32_t key[2]);
/* Waits for all work queued on `device` (bench.py brackets its timed region with it). */
int ci_device_synchronize(int device);
/* Device buffers of finished sessions are parked in a per-process pool (<= 32 GiB of the 288) for reuse by
 * the next fit, and so are their streams and events (creating and destroying a stream costs about
 * a millisecond on this runtime); this returns all of them to the driver. */
int ci_pool_trim(void);
/* Pinned (page-locked) host memory for result buffers; recycled through a pool like the device
 * buffers.  ci_host_free accepts only pointers returned by ci_host_alloc. */
int ci_host_alloc(void** ptr, size_t bytes);
int ci_host_free(void* ptr);

/* One-shot: upload, run all W+S Gibbs iterations for B*C chains, download.
 *   y     [B,T]    float32 outcome (standardised); value ignored where mask != 0
 *   mask  [B,T]    uint8, 1 = missing (NaN pre-period steps + the whole after-pre period)
 *   X     [B,T,P]  float32 row-major design, intercept last; NULL when P == 0
 *   season_change [K,T] uint8, 1 where step t is the last step of a season of block k
 *   params[B]
 * The seasonal state, 1 (+1 slope) + sum_k num_seasons[k] components, holds at most 256: states of
 * 65-256 components (e.g. an hour-of-week block of 168 seasons) run on the multi-wavefront kernel
 * (csrc/ci_seasonal_mw.h); wider ones are refused.  ci_fit_gibbs_f64 and the log-likelihood / HMC
 * sessions hold at most 64.
 * Replaces _run_gibbs_sampler (causalimpact_lib.py:345-395). */
int ci_fit_gibbs(const ci_problem* problem, const float* y, const uint8_t* mask, const float* X,
                 const uint8_t* season_change, const ci_series_params* params,
                 ci_outputs* outputs);

/* The same fit computed in FLOAT64 throughout (DataOptions.dtype = float64: the reference runs its
 * sampler in the requested dtype, causalimpact_lib.py:159; its numeric pin covers float32 and
 * float64, causalimpact_lib_test.py:655-662).  y, X and every result array are float64; any model
 * the float32 entry point takes (seasonal blocks, P up to 512, any T).  One wavefront per chain
 * (csrc/ci_gibbs64.h): trend models time-parallel over its 64 lanes, models with seasonal blocks
 * sequential in time -- the precision option, not the fast one.  Same random stream as
 * ci_fit_gibbs: the two agree draw for draw to float32 round-off. */
typedef struct ci_outputs_f64 {
  double* observation_noise_scale;  /* [B,C,S]   */
  double* level_scale;              /* [B,C,S]   */
  double* slope_scale;              /* [B,C,S]   */
  double* seasonal_drift_scales;    /* [B,C,S,K] */
  double* weights;                  /* [B,C,S,P] */
  double* level;                    /* [B,C,S,T] */
  double* slope;                    /* [B,C,S,T] */
  double* seasonal_levels;          /* [B,C,S,T,K] */
  double* posterior_means;          /* [B,C,T]   */
  double* posterior_trajectories;   /* [B,C,S,T] */
} ci_outputs_f64;
int ci_fit_gibbs_f64(const ci_problem* problem, const double* y, const uint8_t* mask,
                     const double* X, const uint8_t* season_change,
                     const ci_series_params* params, ci_outputs_f64* outputs);
/* Duration (HIP events) of the sampling kernel of the calling thread's last successful
 * ci_fit_gibbs_f64 -- the call itself also allocates, uploads and downloads. */
int ci_fit_gibbs_f64_kernel_ms(float* kernel_ms);
/* The route ci_fit_gibbs_f64 takes for `problem`, decided on the host from its shape alone (no
 * device call; the same validation and the same errors as the fit: state wider than 64, LDS limit).
 *   global_ws    1: the arrays over time in the per-chain HBM workspace, 0: in LDS
 *   reg_lds      1: the regression block's O(P^2) arrays in LDS, 0: in the workspace
 *   trend_kernel 1: the eight-wavefront trend kernel (num_blocks = 0), 0: the sequential kernel
 *   lds_bytes    the dynamic LDS of the launch
 * The tests use it to prove which kernel build and memory layout a shape reaches. */
int ci_fit_gibbs_f64_route(const ci_problem* problem, int32_t* global_ws, int32_t* reg_lds,
                           int32_t* trend_kernel, int64_t* lds_bytes);

/* Device-resident variant (what bench.py times: inputs already in HBM). */
int ci_session_create(const ci_problem* problem, const float* y, const uint8_t* mask,
                      const float* X, const uint8_t* season_change,
                      const ci_series_params* params, ci_session** session);
/* A RAGGED session: B trend models (num_blocks = 0, P <= 52, float32) whose series have their own
 * lengths, fitted in one launch.  problem->T is the ROW STRIDE of every array over time -- y and
 * mask [B,T], X [B,T,P], every [.., T] member of ci_outputs, observed / flags of
 * ci_session_summarize -- and must equal the longest series; series b has series_lengths[b] steps,
 * 3 <= series_lengths[b] <= T, and all series must run the same number of steps per thread
 * (the smallest L in {1, 2, 4, 8, 16} with 256 L >= length; hence T <= 4096).  Rows [length, T) of
 * the inputs are padding and are never read; elements [length, T) of level, slope, posterior_means
 * and posterior_trajectories read 0 after a run (the session clears those arrays when it is
 * created; the kernel never writes them).  Series b then gets, bit for bit, the draws of a
 * single-series session of its own length with the same seed and streams.
 * series_ids (int32 [B], or NULL): the series id whose random streams series b draws from, in
 * place of problem->series_offset + b -- the series of one launch need not be neighbours in their
 * panel; ignored under CI_FLAG_SHARED_SERIES_STREAMS.
 * Every argument is checked before any device call; the message names the offending series.
 * ci_session_run, _fetch, _summarize (observed = NaN and flags = 0 in the padding; order
 * statistics reported for padding steps carry no meaning), _algorithmic_bytes (counts real
 * steps), _kernel_name ("ci::gibbs_kernel<D,L,PM,false,ragged>") and _destroy take such a session;
 * ci_session_run_streamed and ci_session_profile refuse it.  It always runs the four-wavefront
 * kernel (as under CI_FLAG_FOUR_WAVES: same bits as the eight-wavefront one). */
int ci_session_create_ragged(const ci_problem* problem, const int32_t* series_lengths,
                             const int32_t* series_ids, const float* y, const uint8_t* mask,
                             const float* X, const ci_series_params* params, ci_session** session);
/* A RAGGED SEASONAL session: B models of trend plus ONE seasonal block of 2..7 seasons
 * (num_blocks = 1, P <= 52, float32) whose series have their own lengths, fitted in one launch of
 * the ragged build of the time-parallel kernel.  problem->T is the ROW STRIDE of every array over
 * time, as in ci_session_create_ragged, and of season_change [num_blocks, T] (one table for the
 * launch: the flags are positional, series b reads its first series_lengths[b] entries); seasonal_levels
 * is a [.., T] output too.  T must be a multiple of 4, at most 65536, and the longest series rounded
 * up to that multiple (max(series_lengths) > T - 4); 3 <= series_lengths[b] <= T, and all series
 * must share the chunk length of the draw's grid (4 steps up to 2048 steps, then ceil(length / 512)
 * rounded up to a multiple of 4).  CI_FLAG_SEQUENTIAL_SEASONAL, CI_FLAG_CLUSTER_SEASONAL,
 * CI_FLAG_MULTIWAVE_SEASONAL and CI_FLAG_SEASONAL_WORKSPACE are refused: a single fit would not run
 * this kernel under them.  series_ids, the padding contract (elements [length, T) of level, slope,
 * seasonal_levels, posterior_means and posterior_trajectories read 0), the checks before any device
 * call and the entry points that take or refuse the session are those of ci_session_create_ragged;
 * ci_session_kernel_name reports "ci::gibbs_wide_kernel<D,NS,ragged>".  Series b gets, bit for bit,
 * the draws of a single-series session of its own length with the same seed and streams.  It always
 * runs one workgroup per chain (the stock kernel gives the same bits for every cluster size). */
int ci_session_create_ragged_seasonal(const ci_problem* problem, const int32_t* series_lengths,
                                      const int32_t* series_ids, const float* y, const uint8_t* mask,
                                      const float* X, const uint8_t* season_change,
                                      const ci_series_params* params, ci_session** session);
/* Runs the fit on the session's stream and waits for it.  kernel_ms (optional)
 * receives the Gibbs kernel's duration measured with HIP events on that stream. */
int ci_session_run(ci_session* session, float* kernel_ms);
int ci_session_fetch(ci_session* session, ci_outputs* outputs);
/* ci_session_run + ci_session_fetch with the copies OVERLAPPED with the fit: the persistent
 * kernel publishes, every chunk_draws retained draws, how many rows of each chain are complete;
 * the host then queues the device-to-host copies of those rows ([chains, chunk, T] blocks of
 * level / slope / trajectories) on a second stream while sampling continues, and only the last
 * chunk and the small arrays remain after the kernel ends.  Give it buffers from ci_host_alloc
 * (pinned): the copies then run at PCIe rate; pageable buffers work but copy synchronously.
 * Models on the seasonal kernels are copied in the same chunks after the kernel has finished. */
int ci_session_run_streamed(ci_session* session, ci_outputs* outputs, int32_t chunk_draws,
                            float* kernel_ms);
/* Bytes the kernel must move per run (algorithmic bytes, DESIGN.md "Roofline"). */
int ci_session_algorithmic_bytes(const ci_session* session, double* bytes);
/* Name of the Gibbs kernel instantiation this session dispatches to, as a profiler shows it
 * (e.g. "ci::gibbs_kernel<2,4,1,false>"); NUL-terminated, truncated to buflen. */
int ci_session_kernel_name(const ci_session* session, char* buf, int32_t buflen);
/* Developer aid: when enabled, the next ci_session_run() accumulates shader-clock cycles of
 * the kernel's phases (block 0) into 32 counters; cycles16 (optional, 32 entries) receives the counters
 * of the previous run.  Slot meaning: DESIGN.md "Time budget". */
int ci_session_profile(ci_session* session, int enable, int64_t* cycles16);
int ci_session_destroy(ci_session* session);

/* A session MADE FROM DRAWS: what the prediction-error and placebo entries read -- the data and the
 * pooled parameter draws of B fits -- uploaded from the host, so that every route that holds its draws
 * there (float64 fits, HMC fits, fits pooled over devices, batches fitted series by series) runs the
 * filters of a fit's own session.  The filters never read the fit itself.
 *   problem   geometry (T, P, has_slope, the blocks), num_chains C, num_results S, seed, chain_offset,
 *             series_offset, flags (CI_FLAG_SHARED_SERIES_STREAMS), device, as of the fit; num_warmup is
 *             not read.  Chains pooled from several devices are ONE session with chain_offset 0.
 *   y, mask, X, season_change, params[B]   as ci_session_create takes them
 *   observation_noise_scale, level_scale, slope_scale [B,C,S], seasonal_drift_scales [B,C,S,K],
 *   weights [B,C,S,P]   the draws, chain-major, in the layout ci_session_fetch delivers; slope_scale
 *             is read only with has_slope, seasonal_drift_scales with K > 0, X and weights with P > 0
 *             (each may be NULL otherwise)
 * ci_session_create_from_draws takes float32 arrays: given the draws ci_session_fetch delivered and
 * the fit's problem record, every entry below returns the bits of the fit's own session.
 * ci_session_create_from_draws_f64 takes float64 arrays and filters them as they are, through the
 * float64-input builds of the same kernels (every value is widened to double once, where it is
 * loaded, so float32 values passed as float64 give the float32 entry's bits).
 * Checked on the host before the first device call: NULL pointers, the problem record, an unmasked y
 * that is not finite ("y[b, t] is not finite but unmasked"), and every scale draw, which must be
 * finite and not negative (the message names the array, the series and the pooled draw n = c * S + s).
 * The session is not ragged.  It holds no fit workspace, no trajectories and no latent draws.
 * It is accepted by ci_session_summarize_predictions[_blocks], ci_session_summarize_placebo[_blocks],
 * ci_session_simulate_placebo[_blocks], ci_session_pool_placebo[_blocks],
 * ci_session_pool_simulated_placebo[_blocks] (unchanged signatures and checks; the simulated entries
 * address Philox as on a fit's session: series key, chain_offset + c, draw, slot, step), their ci_test_
 * entries and ci_session_destroy.  Every entry that needs a fit -- ci_session_run, _run_streamed,
 * _fetch, _summarize, _summarize_components, _summarize_windows, _summarize_paths, _pool_trajectories,
 * _pool_event_trajectories, _value_mean, _profile, _kernel_name, _algorithmic_bytes and
 * ci_comm_session_all_gather -- refuses it before any device call: ci_last_error names the entry and
 * says that the session was made from draws. */
int ci_session_create_from_draws(const ci_problem* problem, const float* y, const uint8_t* mask,
                                 const float* X, const uint8_t* season_change,
                                 const ci_series_params* params, const float* observation_noise_scale,
                                 const float* level_scale, const float* slope_scale,
                                 const float* seasonal_drift_scales, const float* weights,
                                 ci_session** session);
int ci_session_create_from_draws_f64(const ci_problem* problem, const double* y, const uint8_t* mask,
                                     const double* X, const uint8_t* season_change,
                                     const ci_series_params* params,
                                     const double* observation_noise_scale, const double* level_scale,
                                     const double* slope_scale, const double* seasonal_drift_scales,
                                     const double* weights, ci_session** session);

/* On-device summarisation of the pooled posterior-predictive draws of a finished run, for all
 * B series of the session at once: replaces the T x (C*S) pandas/numpy work of _compute_impact
 * (causalimpact_lib.py:793-837 effect trajectories, posterior_processing.py:25-60 quantiles,
 * :966-1017 per-draw post-period totals).  All results are float64 on the data scale:
 *   value[b, n, t] = trajectory[b, n, t] * scale[b] + shift[b]   (standardize.py:60-64)
 *   point[b, n, t] = -(value[b, n, t] - observed[b, t])           NaN where observed is NaN
 *   cum[b, n, t]   = running sum of point from the treatment start (NaN steps skipped, reported NaN)
 * scale, shift [B]; observed [B,T] data-scale outcome, NaN = no observation; flags [B,T]: bit 0
 * = t >= treatment start, bit 1 = inside the post-period window.  ranks: num_ranks (<= 8)
 * 0-based order statistics over the N = C*S draws of a series (the caller interpolates
 * quantiles from them exactly as numpy does).  Outputs (host, caller-allocated, any may be NULL):
 *   value_order [B, num_ranks, T], cum_order [B, num_ranks, T],
 *   per_draw [B, 2, N]: sum over the window of value, and of point (NaN skipped),
 *   per_draw_order [B, 2, num_ranks]: the same order statistics of those two rows of totals
 *   (what the `summary` frame's bands interpolate: causalimpact_lib.py:1019-1075).
 * Any output pointer may be NULL. */
int ci_session_summarize(ci_session* session, const double* scale, const double* shift,
                         const double* observed, const uint8_t* flags, int32_t num_ranks,
                         const int32_t* ranks, double* value_order, double* cum_order,
                         double* per_draw, double* per_draw_order);
/* On-device summary of the model's COMPONENTS over the pooled draws of a finished run, for all B
 * series of the session at once.  Additive: no struct or signature changed and CI_ABI_VERSION stays 5;
 * a caller that may meet an older library looks the symbol up (dlsym) before using it.  With (scale[b], shift[b]) exactly as handed to
 * ci_session_summarize, n one of the N = C*S pooled draws (chain-major), all in float64:
 *   trend[b, n, t]       = level[b, n, t] * scale[b] + shift[b]          (two roundings)
 *   seasonal_k[b, n, t]  = seasonal_levels[b, n, t, k] * scale[b]        one per seasonal block k
 *   regression[b, n, t]  = (sum over j = 0..P-1, ascending, of X[b, t, j] * weights[b, n, j]) * scale[b]
 *                          (the products of two float32 values are exact; only the additions round)
 * and, on the model's scale, the regression weights of every design column j (the intercept
 * column included).  For every component and step, and for every column: the MEAN over the N draws
 * and the ORDER STATISTICS at `ranks` (num_ranks <= 8, 0-based; the caller interpolates quantiles
 * from them as numpy does); for every column also the share of draws with a non-zero weight.
 * Outputs (host, caller-allocated, float64; each may be NULL and is then skipped):
 *   trend_mean [B, T]            trend_order [B, num_ranks, T]
 *   seasonal_mean [B, K, T]      seasonal_order [B, K, num_ranks, T]
 *   regression_mean [B, T]       regression_order [B, num_ranks, T]
 *   inclusion_prob [B, P]        weight_mean [B, P]        weight_order [B, num_ranks, P]
 * With K = 0 the seasonal outputs, with P = 0 the regression and weight outputs are left untouched.
 * Order statistics equal a sort of the same float64 values bit for bit, inclusion counts are
 * exact, a mean is within N * 2^-52 * max|x| of any other float64 summation of its row.
 * Ordinary and both kinds of ragged sessions are taken, on every kernel route.  In a ragged
 * session T is the row stride of the outputs; beyond a series' own length every latent reads 0
 * (the padding contract), so there trend = shift[b], the seasonal and regression terms are 0, and
 * none of it carries meaning -- as for ci_session_summarize.  The components pass one after another
 * through the scratch of ci_session_summarize (allocated by whichever of the two runs first): no
 * device memory beyond it unless P > T.
 * Checked before any device call: a finished ci_session_run, num_ranks in [1, 8], ranks in [0, N). */
int ci_session_summarize_components(ci_session* session, const double* scale, const double* shift,
                                    int32_t num_ranks, const int32_t* ranks,
                                    double* trend_mean, double* trend_order,
                                    double* seasonal_mean, double* seasonal_order,
                                    double* regression_mean, double* regression_order,
                                    double* inclusion_prob, double* weight_mean,
                                    double* weight_order);
/* One-step-ahead PREDICTION ERRORS of every fit of a finished run, for all B series of the session
 * at once: for every pooled draw n (N = C*S, chain-major) the Kalman filter of that draw's model over
 * the observed series, all in float64.  Additive: CI_ABI_VERSION stays 5; look the symbol up (dlsym)
 * where an older library may be met.  The model of series b and draw n, with d = 1 + has_slope +
 * (ns - 1) state components (level, [slope], ns - 1 seasonal effects):
 *   sigma_obs, sigma_level, sigma_slope, sigma_drift: the float32 draws of ci_outputs widened to
 *     double; H = sigma_obs^2, the process variances sigma_level^2, sigma_slope^2 (separately
 *     rounded squares);
 *   a = (init_level_loc, 0, ..), P = 0 but P[0][0] = init_level_scale^2, P[1][1] =
 *     init_slope_scale^2 (with a slope) and, over the effects i, j, init_seasonal_scale^2 *
 *     ((i == j) - 1 / ns) -- the members of the ci_series_params the session was created with;
 *   transition T_t: level += slope; at a step t whose season_change[t] is set the effects x become
 *     (x_1, .., x_{ns-2}, -sum x); Q_t: sigma_level^2 on P[0][0], sigma_slope^2 on P[1][1], and at
 *     such a step (sigma_drift / ns)^2 on EVERY entry of the effects' block;
 *   Z picks the level and the first effect;
 *   reg[n, t] = sum over j = 0..P-1, ascending from 0.0, of (double)X[b, t, j] * (double)weights[b, n, j].
 * For t = 0 .. T_b - 1 (T_b = T, or the series' own length in a ragged session):
 *   m = Z a;   F = Z P Z' + H;   f = m + reg[n, t]
 *   forecast[n, t] = f * scale[b] + shift[b]                (two roundings, as ci_session_summarize)
 *   variance[n, t] = (F * scale[b]) * scale[b]
 *   if mask[b, t] == 0:  v = (double)y[b, t] - f
 *                        pit[n, t] = 0.5 * erfc(-v / sqrt(2 F))
 *                        loglik[n] += -0.5 * (log(2 pi) + log(F) + v * v / F)
 *                        a += (P Z' / F) v;   P -= (P Z') (P Z')' / F
 *   else:                pit[n, t] = 0.0                    (no observation to score)
 *   if t + 1 < T_b:      a = T_t a;   P = T_t P T_t' + Q_t
 * so forecast and variance at a masked step are those of the several-steps-ahead forecast from the
 * last observation.  Beyond T_b (padding of a ragged session) f = 0: the forecast reads shift[b],
 * variance and pit 0; none of it carries meaning there.
 * scale, shift [B] as handed to ci_session_summarize; ranks: num_ranks (1..8) 0-based order
 * statistics over the N draws.  Outputs (host, caller-allocated, float64; each may be NULL: it is
 * then skipped and its matrix is not built):
 *   forecast_mean [B, T]   forecast_order [B, num_ranks, T]   variance_mean [B, T]   pit_mean [B, T]
 *   loglik [B, N]          (per draw, on the model's scale)
 * Means and order statistics over the draws are those of ci_session_summarize_components.
 * Ordinary and both kinds of ragged sessions are taken, on every kernel route; the models: a trend
 * with or without slope, alone or with ONE block of 2 to 7 seasons.  The matrices pass one after
 * another through the scratch of ci_session_summarize: no device memory beyond it but five doubles
 * per series.  Checked before any device call: the arguments but the outputs are not NULL, the block
 * list is one of the above, a finished ci_session_run, num_ranks in [1, 8], ranks in [0, N). */
int ci_session_summarize_predictions(ci_session* session, const double* scale, const double* shift,
                                     int32_t num_ranks, const int32_t* ranks,
                                     double* forecast_mean, double* forecast_order,
                                     double* variance_mean, double* pit_mean, double* loglik);
/* PLACEBO FORECASTS of every fit of a finished run, for all B series of the session at once: the
 * treatment is pretended to begin at ORIGINS inside the observed series, and for every pooled draw n
 * the sum of the next H_b observations is forecast without any update -- how a cumulative band of
 * that length behaves where no effect exists.  Additive: CI_ABI_VERSION stays 5; look the symbol up
 * (dlsym) where an older library may be met.  This is the FIXED-PARAMETER placebo: every draw's
 * scales and weights are those of the one fit the session ran; nothing is refitted.
 * The model, the state space, Z, T_t, Q_t, reg[n, t] and the initial moments of series b and draw n
 * are those of ci_session_summarize_predictions above.  For an origin o and the horizon H_b >= 1 of
 * the series, o + H_b <= T_b:
 *   run that filter over t = 0 .. o - 1: (a, P) are the predicted moments of x_o given y[0 .. o - 1]
 *   r = 0 (d components), V = 0, C = 0, A = 0, cnt = 0
 *   for h = 0 .. H_b - 1, with t = o + h:
 *     pz = P Z';   m = Z a
 *     if mask[b, t] == 0 (sums ascending in h, from 0.0):
 *       C += m + reg[n, t];   A += (double)y[b, t];   cnt += 1
 *       V += (2 (Z r) + Z pz) + sigma_obs^2;   r += pz
 *     if h + 1 < H_b:   a = T_t a;   r = T_t r;   P = T_t P T_t' + Q_t
 * (r is Cov(S, x) of the running sum S: it transforms like a mean.)  C is the conditional mean of
 * the sum of the counted observations, V its exact predictive variance for that draw, observation
 * noise included.  Per (b, origin slot i, n):
 *   SUM    = C * scale[b] + cnt * shift[b]                  (separate roundings)
 *   SPREAD = ((V + (A - C)^2) * scale[b]) * scale[b]
 *   PIT    = 0.5 * erfc(-(A - C) / sqrt(2 V))
 * and 0 in all three where cnt == 0 or the slot is unused.
 * scale, shift [B] as handed to ci_session_summarize; max_origins: O, the slots per series, in
 * [1, T]; origins [B, O]: steps, strictly ascending, -1 = unused, the unused slots at the end of the
 * row; horizon [B].  Outputs (host, caller-allocated, float64, each [B, O]; each may be NULL: it is
 * then skipped and its matrix is not built -- what the others return does not change):
 *   predicted_mean, spread_mean, pit_mean: the means over the N draws of SUM, SPREAD and PIT, as
 *   ci_session_summarize_components takes its means.
 * The predictive variance of the sum over the draws' mixture is spread_mean - e^2 with e the
 * observed sum on the data scale minus predicted_mean.
 * Sessions and models as ci_session_summarize_predictions; a ragged session uses each series' own
 * length T_b.  The matrices [B * O, N] pass one after another through the scratch of
 * ci_session_summarize.  Checked before any device call: the arguments but the outputs are not NULL,
 * the block list, a finished ci_session_run, max_origins in [1, T], horizon >= 1, the origins
 * ascending with -1 only at the end, o + H_b <= T_b. */
int ci_session_summarize_placebo(ci_session* session, const double* scale, const double* shift,
                                 int32_t max_origins, const int32_t* origins, const int32_t* horizon,
                                 double* predicted_mean, double* spread_mean, double* pit_mean);
/* PLACEBO FORECASTS AT SEVERAL HORIZONS from one filter pass: ci_session_summarize_placebo's three
 * outputs for K horizons per series, every horizon looking from the SAME origins, so that the rows
 * are comparable (how does the check behave after 1, 2, 4 weeks; from which horizon on does the model
 * drift).  Additive: CI_ABI_VERSION stays 5; look the symbol up (dlsym) where an older library may be
 * met.  The running C, V, A and cnt of the loop above after h steps are what a window of horizon h
 * returns, so the forecast of an origin runs to the row's last horizon and SUM, SPREAD and PIT are
 * formed -- with the expressions above -- at every h == horizons[b, k]:
 *   out[b, i, k] == what ci_session_summarize_placebo returns at [b, i] with horizon[b] = horizons[b, k],
 * bit for bit, for every output.
 * max_origins, origins [B, O]: as above, with o + (the row's largest horizon) <= T_b; max_horizons: K,
 * the slots per series, in [1, 64]; horizons [B, K]: >= 1, strictly ascending, -1 = unused, the unused
 * slots at the end of the row, at least one horizon per row.  Outputs (host, caller-allocated,
 * float64, each [B, O, K]; each may be NULL): predicted_mean, spread_mean, pit_mean; 0 in the unused
 * origin and horizon slots and where the window counts no observation.
 * Sessions and models as ci_session_summarize_placebo (a trend with at most one block of 2 to 7
 * seasons; a ragged session uses each series' own length; a session made from draws in float32 or
 * float64).  The filter runs ONCE per chunk of whole series: a chunk's 3 * nb * O * K rows of N doubles
 * lie in the scratch of ci_session_summarize where one series' rows fit its B * T, else in a buffer of
 * the call's own of at most CI_PATHS_MAX_BYTES, given back when it returns; one series that does not
 * fit that is refused.  No value depends on where the chunks are cut.  Checked before any device call:
 * the arguments but the outputs are not NULL, the block list, a finished ci_session_run, max_horizons,
 * the horizon rows, then the origins as above with every row's largest horizon. */
int ci_session_summarize_placebo_horizons(ci_session* session, const double* scale, const double* shift,
                                          int32_t max_origins, const int32_t* origins /* [B, O] */,
                                          int32_t max_horizons, const int32_t* horizons /* [B, K] */,
                                          double* predicted_mean, double* spread_mean,
                                          double* pit_mean /* each [B, O, K], may be NULL */);
/* ci_session_summarize_predictions and ci_session_summarize_placebo for ANY BLOCK LIST whose state
 * has at most 64 components (the several-horizons entry has no such twin: K calls of
 * ci_session_summarize_placebo_blocks with the same origins return the same table): weekly plus
 * monthly blocks, blocks of 12, 24 or 52 seasons, blocks with several steps per season next to
 * others.  Additive: CI_ABI_VERSION stays 5; look the symbols up (dlsym) where an older library may
 * be met.  Arguments, outputs, argument checks and their messages are those of
 * ci_session_summarize_predictions and ci_session_summarize_placebo.  The model generalises theirs to
 * the K blocks of the session (hs = has_slope):
 *   block k has n_k = num_seasons[k] seasons and n_k - 1 effects at offset o_k = 1 + hs +
 *     sum_{j<k} (n_j - 1);  d = 1 + hs + sum_k (n_k - 1) <= 64;  Z has ones at 0 and at every o_k;
 *   sigma_drift: the draws [B, N, K]; season_change [K, T]; the initial moments of every block are
 *     init_seasonal_scale^2 * ((i == j) - 1 / n_k), zero across blocks;
 *   m = a[0] + a[o_0] + a[o_1] + ..;  (P Z')_i = P[i][0] + P[i][o_0] + ..;  F = Z (P Z') + H, summed
 *     in that order; Z r and Z pz of the placebo likewise;
 *   transition: level += slope, then for k ascending every block whose season_change[k, t] is set
 *     rotates, x' = (x_1, .., x_{n_k - 2}, -sum x), its rows, its columns and its covariances with
 *     every other component, the sums ascending from 0.0, and takes (sigma_drift_k / n_k)^2 on every
 *     entry of the block; last sigma_level^2 on P[0][0] and sigma_slope^2 on P[1][1].
 * Every other line is that of the entries above.  A filter is run by a group of 8, 16, 32 or 64
 * lanes (the smallest that holds d), a row of P per lane; what it computes for a (series, draw)
 * depends on nothing else in the launch.
 * Sessions: every finished ci_session of ci_session_create (float32 Gibbs), whatever kernel it runs
 * on, its state at most 64; a ragged session is refused (its models belong to the entries above).
 * Checked before any device call: as the entries above, with the state's size in place of their
 * block list. */
int ci_session_summarize_predictions_blocks(ci_session* session, const double* scale, const double* shift,
                                            int32_t num_ranks, const int32_t* ranks,
                                            double* forecast_mean, double* forecast_order,
                                            double* variance_mean, double* pit_mean, double* loglik);
int ci_session_summarize_placebo_blocks(ci_session* session, const double* scale, const double* shift,
                                        int32_t max_origins, const int32_t* origins, const int32_t* horizon,
                                        double* predicted_mean, double* spread_mean, double* pit_mean);
/* SIMULATED PLACEBO FORECASTS: the placebo check for fits under an outcome link (CI_LINK_LOG,
 * CI_LINK_LOG1P), and an independent check of the analytic one under the identity.  Additive:
 * CI_ABI_VERSION stays 5; look the symbols up (dlsym) where an older library may be met.  Under a
 * link the window's total is a sum of exp's of jointly Gaussian values and has no closed form, so
 * for every pooled draw ONE path of the window is drawn from that draw's predictive, linked step by
 * step and summed: N simulated totals per window.  Fixed parameters, as the analytic placebo.
 * Series b, pooled draw n = c * S + s (chain c of the session, kept draw s, S = num_results), origin
 * slot i with origin o, horizon H_b, o + H_b <= T_b.  The model, Z, T_t, Q_t, reg[n, t], the initial
 * moments and the filter are those of ci_session_summarize_placebo (of .._blocks for the block
 * models).  By the chain rule y_{o+h} given the simulated y_o .. y_{o+h-1} is N(f_h, F_h) of a
 * filter that is updated with the simulated values:
 *   run the filter over t = 0 .. o - 1: (a, P) are the predicted moments of x_o
 *   copy (a, P);  S = 0.0;  cnt = 0
 *   for h = 0 .. H_b - 1, u = o + h:
 *     pz = P Z';  m = Z a;  F = Z pz + sigma_obs^2;  f = m + reg[n, u]     (sums in the filters' order)
 *     if mask[b, u] == 0:
 *       z    = normal_d(key_b, chain = chain_offset + c, iter = s, site = SITE_PLACEBO_SIM, sub = i, idx = h)
 *       v    = sqrt(F) * z;   ysim = f + v                  (one rounding each)
 *       S   += link(ysim * scale[b] + shift[b])             (two roundings, no FMA, as ci_session_set_link)
 *       cnt += 1
 *       a += (pz / F) v;   P -= pz pz' / F                  (the filter's own update, with the simulated innovation)
 *     if h + 1 < H_b:  a = T_u a;  P = T_u P T_u' + Q_u
 *   TOTAL[b, i, n] = S   (0.0 where cnt == 0 or the slot is unused)
 * key_b is the Philox key the fit of series b ran on: ci_series_stream_key of the series' id (its
 * series_ids entry in a ragged session, else series_offset + b), or the seed itself under
 * CI_FLAG_SHARED_SERIES_STREAMS.  normal_d is the float64 Box-Muller normal of the specified stream
 * (Philox4x32-10, counter (idx >> 2, site | sub << 8, iter, chain), component idx & 3);
 * SITE_PLACEBO_SIM = 18 is a site of its own: the stream of every other site is untouched.  idx is h
 * whether or not the step is counted -- a masked step leaves its normal unused.  The filter outside
 * the branch goes on from the untouched (a, P).
 * link: a CI_LINK_* value, passed explicitly -- ci_session_set_link is neither read nor changed.
 * seen [B, O] (host, data scale): the observed total of every window; may be NULL when neither
 * spread_mean nor below is asked for.  ranks: num_ranks (1..8) 0-based order statistics over the N
 * draws.  Outputs (host, caller-allocated, float64; each may be NULL and is then skipped):
 *   predicted_mean [B, O]        the mean over n of TOTAL
 *   spread_mean    [B, O]        the mean over n of (TOTAL - seen)^2, one rounding per operation
 *   below          [B, O]        #{n : TOTAL <= seen}, the exact integer count as a double
 *   total_order    [B, num_ranks, O]   the order statistics of TOTAL over n
 *   totals         [B, O, N]     TOTAL itself (tests, and callers that want the draws)
 * all 0 where cnt == 0 or the slot is unused.  A mean is that of ci_session_summarize_components:
 * lane l of 64 adds the values n = l, l + 64, .. ascending from 0.0, the 64 sums are combined by a
 * butterfly (partners 32, 16, .., 1 apart), and the result is divided by N.
 * The filter runs once per call: the totals are simulated into the scratch of ci_session_summarize,
 * reduced, downloaded if wanted, and rewritten in place to the squares.  TOTAL depends on (b, i, n)
 * alone -- not on the launch geometry, nor on how a batch is cut into sessions as long as the
 * series keep their ids and the chains their global ids.
 * Checked before any device call: as ci_session_summarize_placebo (.._blocks), and link in range,
 * num_ranks in [1, 8], ranks in [0, N), seen not NULL unless only predicted_mean, total_order and
 * totals are asked for. */
int ci_session_simulate_placebo(ci_session* session, const double* scale, const double* shift,
                                int32_t max_origins, const int32_t* origins, const int32_t* horizon,
                                int32_t link, const double* seen, int32_t num_ranks, const int32_t* ranks,
                                double* predicted_mean, double* spread_mean, double* below,
                                double* total_order, double* totals);
int ci_session_simulate_placebo_blocks(ci_session* session, const double* scale, const double* shift,
                                       int32_t max_origins, const int32_t* origins, const int32_t* horizon,
                                       int32_t link, const double* seen, int32_t num_ranks,
                                       const int32_t* ranks, double* predicted_mean, double* spread_mean,
                                       double* below, double* total_order, double* totals);
/* PLACEBO FORECASTS OF POOLED SUMS: the forecasts above, added over groups of series draw by draw --
 * the placebo check of a pooled effect.  Additive: CI_ABI_VERSION stays 5; look the symbol up (dlsym)
 * where an older library may be met.
 * The group table is that of ci_session_pool_trajectories: group g has the entries k in offsets[g] ..
 * offsets[g + 1], entry k the member b_k = members[k] (a position in the session, ascending inside a
 * group) and the weight w_k.  Entry k has its own origin row origins[k, 0 .. O - 1] (steps, strictly
 * ascending, -1 = unused, at the end); group g has ONE horizon H_g = horizon[g].  For entry k, slot i
 * and pooled draw n the filter and the forecast of ci_session_summarize_placebo run for series b_k
 * from origins[k, i] with horizon H_g: C, V, cnt in the sampler's units.  On the data scale
 *   s = C * scale[b] + cnt * shift[b]          (separate roundings: SUM above)
 *   v = (V * scale[b]) * scale[b]              (the variance alone)
 * both 0 where cnt == 0 or the slot is unused.  Pooled in float64, entries ascending, one rounding
 * per operation, no fused multiply-add:
 *   S[g, i, n] = init_S[g, i, n];  for k ascending:  S = S + w_k * s_k
 *   U[g, i, n] = init_U[g, i, n];  for k ascending:  U = U + (w_k * w_k) * v_k
 * init and out: host arrays [G, O, 2, N], S then U.  init may be NULL (0.0) and may be `out` itself;
 * several sessions continue one running sum by handing `out` on as `init`, bit for bit however the
 * series are cut into sessions.
 * seen (optional, host, [G, O]): the pooled observed sum on the data scale.  With it the call also
 * returns predicted_mean, spread_mean, pit_mean [G, O] (each may be NULL), the means over the N draws,
 * as ci_session_summarize_components takes its means, of
 *   e = seen[g, i] - S;   SUM = S;   SPREAD = U + e * e;   PIT = 0.5 * erfc(-e / sqrt(2 U))
 * all 0 where U == 0 (U holds sigma_obs^2 of every counted step: it is 0 exactly when no member
 * counts a step).  Given draw n of EVERY member the pooled sum of the counted observations is
 * N(S, U) if the members are independent of each other -- the assumption a pooled band rests on,
 * and the one this check tests: shocks common to the members show as too many exceedances.
 * Sessions and models as ci_session_summarize_placebo; a ragged session uses each series' own
 * length T_b.  At most B entries at a time pass through the scratch of ci_session_summarize, a SUM
 * pass and a VAR pass each; beyond it the call holds the tables and the [G, O, 2, N] accumulators.
 * Checked before any device call, with the group, entry or slot named: the arguments but init, seen
 * and the means are not NULL, the block list, a finished ci_session_run, the group table as for
 * ci_session_pool_trajectories, max_origins in [1, T], horizon >= 1, every origin row ascending with
 * -1 only at the end, origin + H_g <= T_b, and no mean output without `seen`. */
int ci_session_pool_placebo(ci_session* session, const double* scale, const double* shift,
                            int32_t num_groups, const int32_t* offsets, const int32_t* members,
                            const double* weights, int32_t max_origins,
                            const int32_t* origins /* [K, O] */, const int32_t* horizon /* [G] */,
                            const double* init, double* out, const double* seen,
                            double* predicted_mean, double* spread_mean, double* pit_mean);
/* ci_session_pool_placebo with the filter of ci_session_summarize_placebo_blocks: the pooled placebo
 * forecasts of ANY block list whose state has at most 64 components.  Additive: CI_ABI_VERSION stays
 * 5; look the symbol up (dlsym) where an older library may be met.  The arguments, the group table,
 * s and v, the order of addition, init / out [G, O, 2, N] and their aliasing, seen and the three means
 * are those of ci_session_pool_placebo; only this differs:
 *   the model, Z, the transition and the filter of entry k are those of .._summarize_placebo_blocks
 *     (a group of 8, 16, 32 or 64 lanes per (entry, draw)), so C, V and cnt are its values;
 *   the filter runs ONCE per chunk of at most B entries: one forecast branch stores s into the
 *     scratch of ci_session_summarize and v into a buffer of the call's own, [chunk, O, N]; the two
 *     accumulates and the finishing step are the kernels of ci_session_pool_placebo.  Where the two
 *     filters agree bit for bit (the models both take) so do the accumulators and the means.
 * Sessions: those of ci_session_summarize_placebo_blocks -- a finished ci_session of
 * ci_session_create, its state at most 64; a ragged session is refused (its models belong to
 * ci_session_pool_placebo).
 * Checked before any device call: as ci_session_pool_placebo, with the state's size in place of its
 * block list. */
int ci_session_pool_placebo_blocks(ci_session* session, const double* scale, const double* shift,
                                   int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                   const double* weights, int32_t max_origins,
                                   const int32_t* origins /* [K, O] */, const int32_t* horizon /* [G] */,
                                   const double* init, double* out, const double* seen,
                                   double* predicted_mean, double* spread_mean, double* pit_mean);
/* PLACEBO FORECASTS OF POOLED SUMS AT SEVERAL HORIZONS from one filter pass: what
 * ci_session_pool_placebo[_blocks] returns, for K horizons per group, every horizon looking from the
 * SAME origins -- how the pooled check moves with the window's length.  Additive: CI_ABI_VERSION
 * stays 5; look the symbols up (dlsym) where an older library may be met.
 * The group table, the entries' origin rows origins[k, 0 .. O - 1], scale, shift, s, v and the order
 * of addition are those of ci_session_pool_placebo.  Group g has the horizon row horizons[g, 0 .. K - 1]
 * (>= 1, strictly ascending, -1 = unused, the unused slots at the end, at least one horizon per row;
 * max_horizons: K, in [1, 64]).  The running C, V and cnt of the forecast loop after h steps are what a
 * window of horizon h returns, so the forecast of an entry's origin runs to its group's largest
 * horizon and s and v are formed at every h == horizons[g, k].
 *   init, out: host arrays [G, O, K, 2, N], S then U; init may be NULL (0.0) and may be `out` itself
 *   seen (optional): [G, O, K];  predicted_mean, spread_mean, pit_mean: [G, O, K] each, may be NULL
 * CONTRACT: for every output, x[g, i, k] is, bit for bit, what ci_session_pool_placebo (for .._blocks:
 * ci_session_pool_placebo_blocks) returns at [g, i] when called with the same group table and origins,
 * horizon[g] = horizons[g, k], init[:, :, k] and seen[:, :, k].  An unused horizon slot adds terms of
 * 0, as an unused origin slot does: its accumulators keep `init` and its means are 0 (where U == 0).
 * Several sessions continue one running sum by handing `out` on as `init`, as above.
 * Sessions and models: those of ci_session_pool_placebo (ragged sessions, sessions made from draws in
 * float32 or float64) and of ci_session_pool_placebo_blocks respectively.  The filter runs ONCE per
 * chunk of whole entries, storing s and v of every checkpoint as two planes [chunk * O * K, N]; the
 * accumulate and the finishing step are the kernels of ci_session_pool_placebo with O * K slots.  A
 * chunk's planes lie in the scratch of ci_session_summarize where one entry's 2 * O * K rows fit its
 * B * T rows, else in a buffer of the call's own of at most CI_PATHS_MAX_BYTES, given back when it
 * returns; one entry that does not fit that is refused by name, and so are accumulators [G, O, K, 2, N]
 * beyond CI_PATHS_MAX_BYTES (pass the horizon slots in several calls: the columns are independent).
 * Nothing depends on where the chunks are cut.
 * Checked before any device call, with the group, entry or slot named: as ci_session_pool_placebo
 * (.._blocks), max_horizons and every group's horizon row, the origins with origin + (the group's
 * largest horizon) <= T_b, and no mean output without `seen`. */
int ci_session_pool_placebo_horizons(ci_session* session, const double* scale, const double* shift,
                                     int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                     const double* weights, int32_t max_origins,
                                     const int32_t* origins /* [E, O] */, int32_t max_horizons,
                                     const int32_t* horizons /* [G, K] */, const double* init,
                                     double* out /* [G, O, K, 2, N] */, const double* seen /* [G, O, K] */,
                                     double* predicted_mean, double* spread_mean,
                                     double* pit_mean /* each [G, O, K], may be NULL */);
int ci_session_pool_placebo_horizons_blocks(ci_session* session, const double* scale, const double* shift,
                                            int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                            const double* weights, int32_t max_origins,
                                            const int32_t* origins /* [E, O] */, int32_t max_horizons,
                                            const int32_t* horizons /* [G, K] */, const double* init,
                                            double* out /* [G, O, K, 2, N] */, const double* seen /* [G, O, K] */,
                                            double* predicted_mean, double* spread_mean,
                                            double* pit_mean /* each [G, O, K], may be NULL */);
/* SIMULATED PLACEBO FORECASTS OF POOLED SUMS: the placebo check of a pooled effect under an outcome
 * link, where the pooled total is a weighted sum of sums of exp's and N(S, U) above does not exist.
 * Additive: CI_ABI_VERSION stays 5; look the symbols up (dlsym) where an older library may be met.
 * The group table, the entries, the weights, the origin rows origins[k, 0 .. O - 1] per entry and ONE
 * horizon H_g per group are those of ci_session_pool_placebo.  For entry k (member b_k), slot i and
 * pooled draw n
 *   TOTAL_k[i, n] = TOTAL of ci_session_simulate_placebo for series b_k from origins[k, i] with
 *                   horizon H_g
 * exactly: the same filter (of .._simulate_placebo_blocks in the _blocks entry), the same explicit
 * `link`, the same two-rounding linked value and the same Philox address -- key of series b_k, chain
 * chain_offset + c, iter s, SITE_PLACEBO_SIM, sub = i, idx = h -- and 0.0 where the entry counts no
 * step or the slot is unused.  No random site is added: different members have different keys, so
 * their paths are independent of each other, the assumption the pooled check tests
 * (CI_FLAG_SHARED_SERIES_STREAMS would give all members one world and is not meant for this call); a
 * series has the same simulated world in every group it belongs to.  Pooled in float64, entries
 * ascending, one rounding per operation, no fused multiply-add:
 *   POOL[g, i, n] = init[g, i, n];  for k ascending:  POOL = POOL + w_k * TOTAL_k[i, n]
 * init and out: host arrays [G, O, N] (one plane).  init may be NULL (0.0) and may be `out` itself;
 * several sessions continue one running sum by handing `out` on as `init`, bit for bit however the
 * series are cut into sessions as long as the series keep their ids and the chains their global ids.
 * seen [G, O] (host, the pooled observed total on the data scale) and counted [G, O] (host, int32, the
 * member-steps the window counts over all members) are optional, but wanted TOGETHER by every
 * statistic.  With them the call returns the statistics of ci_session_simulate_placebo over the row
 * POOL[g, i, :] (each output may be NULL and is then skipped):
 *   predicted_mean [G, O]        the mean over n of POOL
 *   spread_mean    [G, O]        the mean over n of (POOL - seen)^2, subtraction and product rounded separately
 *   below          [G, O]        #{n : POOL <= seen}, the exact integer count as a double
 *   total_order    [G, num_ranks, O]   the order statistics of POOL over n
 * the means as ci_session_summarize_components takes its means; spread_mean and below are 0 where
 * counted == 0, and so are the others, POOL being 0.0 there.  A call with empty groups (offsets all
 * 0) and init = the finished sums only takes the statistics.
 * Sessions and models as ci_session_simulate_placebo (.._blocks: a ragged session is refused).  At most
 * B entries at a time pass through the scratch of ci_session_summarize, ONE simulation pass each;
 * beyond it the call holds the tables and the [G, O, N] accumulators, whose rows then pass through
 * the scratch, whole groups at a time, for the statistics -- `out` is downloaded before.  Nothing
 * depends on where the entries or the rows are cut.
 * Checked before any device call, with the group, entry or slot named: as ci_session_pool_placebo,
 * and link in range, num_ranks in [1, 8], ranks (not NULL) in [0, N), no statistic without both
 * `seen` and `counted`. */
int ci_session_pool_simulated_placebo(ci_session* session, const double* scale, const double* shift,
                                      int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                      const double* weights, int32_t max_origins,
                                      const int32_t* origins /* [K, O] */, const int32_t* horizon /* [G] */,
                                      int32_t link, const double* init, double* out /* [G, O, N] */,
                                      const double* seen /* [G, O] */, const int32_t* counted /* [G, O] */,
                                      int32_t num_ranks, const int32_t* ranks, double* predicted_mean,
                                      double* spread_mean, double* below, double* total_order /* [G, R, O] */);
int ci_session_pool_simulated_placebo_blocks(ci_session* session, const double* scale, const double* shift,
                                             int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                             const double* weights, int32_t max_origins,
                                             const int32_t* origins /* [K, O] */, const int32_t* horizon /* [G] */,
                                             int32_t link, const double* init, double* out /* [G, O, N] */,
                                             const double* seen /* [G, O] */, const int32_t* counted /* [G, O] */,
                                             int32_t num_ranks, const int32_t* ranks, double* predicted_mean,
                                             double* spread_mean, double* below,
                                             double* total_order /* [G, R, O] */);
/* Per-draw totals over SUB-WINDOWS of the session's steps, for all B series at once: how an effect
 * unfolds inside the post-period (week 1 against week 4, a promotion's second phase), whose bands,
 * relative effect and tail-area probability need every draw's total over the window and are not
 * combinations of the per-step bands.  Additive: CI_ABI_VERSION stays 5; look the symbol up (dlsym)
 * where an older library may be met.  The [B, N, T] float32 trajectories (N = C*S pooled draws,
 * chain-major; T the session's stride) are read where they are, in HBM, and only the columns of the
 * 64-step tiles a window intersects; no [B, T, N] matrix is built.  Series b has the num_windows
 * windows first[b, w], count[b, w] (steps of the session; windows may overlap, count may be 0).  For
 * every series b, window w and draw n, all in float64:
 *   pred_sum = 0.0; point_sum = 0.0
 *   for t = first[b, w] .. first[b, w] + count[b, w] - 1, ascending:
 *     v        = trajectory[b, n, t] * scale[b] + shift[b]     (two roundings, no fused multiply-add)
 *     pred_sum = pred_sum + v
 *     point    = -(v - observed[b, t])
 *     if point == point: point_sum = point_sum + point        (NaN, no observation: skipped)
 *   per_draw[b, w, 0, n] = pred_sum;   per_draw[b, w, 1, n] = point_sum
 * which a plain loop on the host reproduces bit for bit, and which for a window equal to the steps
 * whose flag bit 1 is set are ci_session_summarize's per_draw and per_draw_order, bit for bit.
 * per_draw_order[b, w, k, r] is the ranks[r]-th smallest of per_draw[b, w, k, :]; count = 0 gives
 * totals 0.0 and order statistics 0.0.  scale, shift [B] and observed [B, T] as handed to
 * ci_session_summarize; first, count [B, num_windows]; ranks: num_ranks 0-based order statistics
 * over the N draws.  Outputs (host, caller-allocated, float64; each may be NULL):
 *   per_draw [B, num_windows, 2, N]       per_draw_order [B, num_windows, 2, num_ranks]
 * Ordinary and both kinds of ragged sessions are taken, on every kernel route; in a ragged session
 * every series passes windows of its own.  The scratch of ci_session_summarize is neither built nor
 * touched: the device memory of a call is the tables (observed, scale, shift, first, count, ranks)
 * plus 2 * (N + 8) doubles per (series, window), given back when it returns.  No load touches
 * memory outside the trajectories, observed and the tables.
 * Checked before any device call, the error text naming the offending window: a finished run, no
 * NULL argument but the two outputs, num_windows in [1, 1024], first >= 0, count >= 0, first +
 * count <= T, num_ranks in [1, 8], ranks in [0, N). */
int ci_session_summarize_windows(ci_session* session, const double* scale, const double* shift,
                                 const double* observed, int32_t num_windows,
                                 const int32_t* first, const int32_t* count,
                                 int32_t num_ranks, const int32_t* ranks,
                                 double* per_draw, double* per_draw_order);
/* Simultaneous bands and a whole-path test of the effect: for every draw the largest standardised
 * excursion of its WHOLE path over a window, for the prediction and for the cumulative effect.  A
 * pointwise band is no statement about a path, and the total of a window misses an effect that rises
 * and then reverses; the 1 - alpha quantile c of the excursions gives the band center -+ c * spread
 * that holds the whole path with probability 1 - alpha, and the share of draws whose excursion
 * reaches the observed one a p-value for "the observed path is unlike every predictive path".
 * Additive: CI_ABI_VERSION stays 5; look the symbol up (dlsym) where an older library may be met.
 * The [B, N, T] float32 trajectories (N = C*S pooled draws, chain-major; T the session's stride) are
 * read where they are, in HBM, and only the columns of the 64-step tiles a window intersects; no
 * [B, T, N] matrix of a whole series is built.  Series b has the num_windows windows first[b, w],
 * count[b, w] (steps of the session; windows may overlap, count may be 0).  For every series b,
 * window w = (first, count) and draw n, all in float64, with
 *   v[n, t] = trajectory[b, n, t] * scale[b] + shift[b]        (two roundings, no fused multiply-add)
 * the two paths over t = first .. first + count - 1 are
 *   path 0 (prediction)         x0[n, t] = v[n, t];                        target_0[t] = observed[b, t]
 *   path 1 (cumulative effect)  x1[n, t] = the running sum over s = first .. t, ascending, of
 *                               point = -(v[n, s] - observed[b, s]), NaN points skipped;   target_1[t] = 0.0
 * (the expressions of ci_session_summarize_windows: x1 at the window's last step is its point_sum,
 * bit for bit), and for k = 0, 1
 *   center_k[t] = (sum over n of x_k[n, t]) / N
 *   spread_k[t] = sqrt((sum over n of (x_k[n, t] - center_k[t])^2) / (N - 1))
 *   counted steps of path k: the window's steps with an observation and spread_k[t] > 0
 *   z_k[n, t]      = |x_k[n, t] - center_k[t]| / spread_k[t]   (subtract, abs, divide: one rounding each)
 *   excursion_k[n] = max over the counted t of z_k[n, t];  0.0 when no step is counted
 *   observed_excursion_k = max over the counted t of |target_k[t] - center_k[t]| / spread_k[t];  NaN
 *                          when no step is counted;  at_k = the first t that attains it, else -1
 *   exceed_k       = #{n : excursion_k[n] >= observed_excursion_k}
 *   excursion_order_k[r] = the ranks[r]-th smallest of excursion_k[:]
 * ORDER OF THE ADDITIONS OVER n (both sums; a function of N alone): 256 partial sums, the i-th over
 * n = i, i + 256, i + 512, ... ascending from 0.0; each run of 64 consecutive partial sums is added
 * pairwise at distances 32, 16, 8, 4, 2, 1 (element l takes l + l', the element above); the four
 * results are added in ascending order.  A host loop in another order agrees with center to N * 2^-53
 * of the largest |x| and with spread to N * 2^-53 relative; GIVEN the returned center and spread, a
 * plain loop on the host reproduces excursion, excursion_order, observed_excursion, at and exceed bit
 * for bit.  count = 0: excursions and order statistics 0.0, observed_excursion NaN, at -1, exceed 0.
 * scale, shift [B] and observed [B, T] as handed to ci_session_summarize; first, count
 * [B, num_windows]; ranks: num_ranks 0-based order statistics over the N draws.  Outputs (host,
 * caller-allocated; each may be NULL):
 *   center, spread [B, num_windows, 2, T] float64: NaN outside the window and, for path 1, at the
 *     steps without an observation (as ci_session_summarize reports `cum`)
 *   excursion [B, num_windows, 2, N]      excursion_order [B, num_windows, 2, num_ranks]   float64
 *   observed_excursion [B, num_windows, 2] float64     at, exceed [B, num_windows, 2] int32
 * Ordinary and both kinds of ragged sessions are taken, on every kernel route; in a ragged session
 * every series passes windows of its own.  DEVICE MEMORY: the scratch of ci_session_summarize is
 * neither built nor touched.  A call takes at most CI_PATHS_MAX_BYTES (1 GiB) of its own, given back
 * when it returns: the tables (observed, scale, shift, first, count, ranks and one int64 per window)
 * and, per (series, window) of `count` steps, count * (2 N + 4) + 2 N + 20 doubles -- both paths of
 * the window's own steps, their moments and the results.  Every (series, window) is computed alone,
 * so the windows are taken in as many chunks as the limit asks for and no result depends on the
 * chunking; a window that does not fit the limit beside the tables is refused by name, a failed
 * allocation is an error.  No load touches memory outside the trajectories, observed and the tables.
 * Checked before any device call, the error text naming the offending window: a finished run, no
 * NULL argument but the outputs, num_windows in [1, 64], first >= 0, count >= 0, first + count <= T,
 * num_ranks in [1, 8], ranks in [0, N). */
#define CI_PATHS_MAX_BYTES (1ll << 30)
int ci_session_summarize_paths(ci_session* session, const double* scale, const double* shift,
                               const double* observed, int32_t num_windows,
                               const int32_t* first, const int32_t* count,
                               int32_t num_ranks, const int32_t* ranks,
                               double* center, double* spread, double* excursion,
                               double* excursion_order, double* observed_excursion,
                               int32_t* at, int32_t* exceed);
/* Weighted sums over GROUPS of series of the predictive trajectories of a finished run, draw by
 * draw: the draws of a pooled effect (all units, a region), whose quantiles are not sums of the
 * per-series quantiles.  Additive: CI_ABI_VERSION stays 5; look the symbol up (dlsym) where an older
 * library may be met.  The [B, N, T] float32 trajectories (N = C*S pooled draws, chain-major; T the
 * session's stride) are read where they are, in HBM.  The num_groups groups are the rows of a sparse
 * weight table in CSR form: group g has the members[offsets[g] .. offsets[g + 1]) (positions of
 * series in the session, strictly ascending) with the weights at the same places; members of zero
 * weight are left out, a group may be empty.  For every group, draw n and step t, all in float64:
 *   acc = init[g, n, t]                          (0.0 when init is NULL)
 *   for the members b of g, ascending:
 *     v   = trajectory[b, n, t] * scale[b] + shift[b]     (two roundings: the value of ci_session_summarize)
 *     acc = acc + weights[g, b] * v                         (two roundings, no fused multiply-add)
 *   out[g, n, t] = acc
 * which a plain loop on the host reproduces bit for bit.  init and out are host arrays
 * [num_groups, N, T] float64 (init may be NULL, and may be out itself).  A batch cut into several
 * sessions continues ONE running sum in series order by handing the `out` of a part to the next as
 * `init`: the result is bit-identical however the batch is cut.  The groups pass through the scratch
 * of ci_session_summarize (allocated by whichever call comes first), min(num_groups, B) at a time.
 * Checked before any device call: no NULL argument but init, a finished run, num_groups >= 1,
 * offsets[0] = 0 and offsets non-decreasing, members strictly ascending within a group and in
 * [0, B), weights finite. */
int ci_session_pool_trajectories(ci_session* session, const double* scale, const double* shift,
                                 int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                 const double* weights, const double* init, double* out);
/* ci_session_pool_trajectories over WINDOWS of the members' trajectories, every member shifted to a
 * start of its own: the draws of a pooled effect in EVENT TIME, for series with their own calendars
 * (a panel) aligned on each one's treatment start.  Additive: CI_ABI_VERSION stays 5; look the
 * symbol up (dlsym) where an older library may be met.  Groups, members and weights as above;
 * first[k] (per entry, parallel to members) is the step of member k that lands in column 0 of its
 * group, width[g] the number of columns of group g, out_stride the row length of init and out
 * (>= every width).  For every group g, draw n and column c < width[g], all in float64:
 *   acc = init[g, n, c]                          (0.0 when init is NULL)
 *   for the members k of g, ascending, b = members[k]:
 *     v   = trajectory[b, n, first[k] + c] * scale[b] + shift[b]     (two roundings)
 *     acc = acc + weights[k] * v                                     (two roundings, no fused multiply-add)
 *   out[g, n, c] = acc
 * which a plain loop on the host reproduces bit for bit.  Columns c >= width[g] are written as 0.0
 * and their values in init do not matter.  init and out are host arrays [num_groups, N, out_stride]
 * float64 (init may be NULL, and may be out itself); several sessions continue one running sum
 * through them as above, in the order of the calls.  With first = 0 and width = out_stride = T
 * everywhere the result is that of ci_session_pool_trajectories, bit for bit.  Ordinary and both
 * kinds of ragged sessions are taken; T is the session's stride.  The groups pass through the
 * scratch of ci_session_summarize, min(num_groups, B) at a time: no device memory beyond it but the
 * tables.  No load touches memory outside the trajectories.
 * Checked before any device call: everything ci_session_pool_trajectories checks, no NULL argument
 * but init, width[g] in [1, out_stride] and <= T, first[k] >= 0, first[k] + width[g] <= T. */
int ci_session_pool_event_trajectories(ci_session* session, const double* scale, const double* shift,
                                       int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                       const double* weights, const int32_t* first, const int32_t* width,
                                       int32_t out_stride, const double* init, double* out);
/* The OUTCOME LINK of a session's summaries: a multiplicative outcome is modelled as log y (or
 * log1p y), and its effect is wanted on the data scale.  E[exp z] != exp E[z]: the link has to be
 * applied draw by draw, before any sum or mean.  Additive: CI_ABI_VERSION stays 5; look the symbols
 * up (dlsym) where an older library may be met.  With
 *   z = (double)trajectory * scale[b] + shift[b]          two roundings, no FMA, as today
 * the `value` of the summaries below is z (CI_LINK_IDENTITY, the default: nothing changes, not a
 * bit), exp(z) (CI_LINK_LOG) or expm1(z) (CI_LINK_LOG1P), the float64 device functions, without a
 * clamp: an exp that overflows is +inf and propagates as numpy's would.  The link is session state
 * and may be set any time after create; an unknown link is an error.  It is honoured by
 *   ci_session_summarize, ci_session_summarize_windows, ci_session_summarize_paths,
 *   ci_session_pool_trajectories, ci_session_pool_event_trajectories, ci_session_value_mean
 * wherever they form `value`; point, cum, the totals, moments, excursions and pooled sums keep their
 * definitions on top of it, so given the device's own values a plain loop on the host still
 * reproduces them bit for bit, and the element-wise exp / expm1 (within 4 ulp of numpy's) is the only
 * place where device and host may differ.  ci_session_summarize_components,
 * ci_session_summarize_predictions, ci_session_summarize_placebo and ci_session_pool_placebo describe
 * the model, which is Gaussian on the transformed scale: they IGNORE the link.  So do the
 * ci_ll_session_* calls and ci_summarize_draws* (transform host draws before the upload).  No call
 * keeps values in the scratch for a later one, so a change of the link finds nothing stale.  In a
 * ragged session a padded step reads link(shift[b]) and carries no meaning, as before. */
#define CI_LINK_IDENTITY 0   /* value = z                      (today's behaviour) */
#define CI_LINK_LOG      1   /* value = exp(z)                                      */
#define CI_LINK_LOG1P    2   /* value = expm1(z)                                    */
int ci_session_set_link(ci_session* session, int32_t link);
/* value_mean [B, T] (host, float64): the mean over the N pooled draws of value[b, n, t] under the
 * session's link, taken exactly as ci_session_summarize_components takes its means (within
 * N * 2^-52 * max|x| of any other float64 summation of the row), through the scratch of
 * ci_session_summarize.  Every link, ordinary and both kinds of ragged sessions.  Under a link the
 * sampler's posterior_means mapped through (scale, shift) are not the posterior mean of the
 * prediction; this is.  Checked before any device call: no NULL argument, a finished run. */
int ci_session_value_mean(ci_session* session, const double* scale, const double* shift,
                          double* value_mean /* [B, T] */);
/* The same summary for draws that are on the host (pooled from several devices / processes, or
 * produced by the HMC path): trajectories [num_draws, T] float32 are uploaded to `device`,
 * summarised there and the (one-series) results returned as above. */
int ci_summarize_draws(int32_t device, int32_t num_draws, int32_t T, const float* trajectories,
                       double scale, double shift, const double* observed, const uint8_t* flags,
                       int32_t num_ranks, const int32_t* ranks, double* value_order,
                       double* cum_order, double* per_draw, double* per_draw_order);
/* ... for float64 trajectories (the draws of ci_fit_gibbs_f64: no rounding to float32 on the way
 * into the order statistics). */
int ci_summarize_draws_f64(int32_t device, int32_t num_draws, int32_t T, const double* trajectories,
                           double scale, double shift, const double* observed, const uint8_t* flags,
                           int32_t num_ranks, const int32_t* ranks, double* value_order,
                           double* cum_order, double* per_draw, double* per_draw_order);
/* ci_session_summarize_paths for float64 draws that are on the host and belong to no session: the
 * POOLED draws of groups of series (ci_session_pool_trajectories, ci_session_pool_event_trajectories),
 * so that a pooled effect gets simultaneous bands and a whole-path test like every series.  Additive:
 * CI_ABI_VERSION stays 5; look the symbol up (dlsym) where an older library may be met.
 * draws [num_groups, N = num_draws, T] float64 are uploaded to `device`; group g has the num_windows
 * windows first[g, w], count[g, w] (steps of its T; windows may overlap, count may be 0).  With
 *   v[n, t] = draws[g, n, t] * scale[g] + shift[g]             (two roundings, no fused multiply-add)
 * paths, targets, center, spread, counted steps, excursions, observed_excursion, at, exceed and
 * excursion_order are those of ci_session_summarize_paths, with g in place of b: the same
 * expressions in the first pass and the very same kernels after it, hence the same ORDER OF THE
 * ADDITIONS OVER n and the same roundings.  On draws that are float32 values the results are those of
 * ci_session_summarize_paths on the float32 trajectories bit for bit; given the returned center and
 * spread a plain loop on the host reproduces the rest bit for bit.  count = 0: excursions and order
 * statistics 0.0, observed_excursion NaN, at -1, exceed 0.  scale, shift [num_groups] (pooled draws are
 * on the data scale already: 1.0 and 0.0); observed [num_groups, T], NaN: no observation; ranks:
 * num_ranks 0-based order statistics over the N draws.  Outputs (host, caller-allocated; each may be
 * NULL):
 *   center, spread [num_groups, num_windows, 2, T] float64: NaN outside the window and, for path 1, at
 *     the steps without an observation
 *   excursion [num_groups, num_windows, 2, N]   excursion_order [num_groups, num_windows, 2, num_ranks]
 *   observed_excursion [num_groups, num_windows, 2] float64   at, exceed [num_groups, num_windows, 2] int32
 * DEVICE MEMORY: a call takes at most CI_PATHS_MAX_BYTES of its own, given back when it returns: the
 * tables, N * T doubles per group whose draws are on the device, and per (group, window) the doubles
 * ci_session_summarize_paths counts.  The (group, window) pairs are taken in order, in as many chunks
 * as the limit asks for; a chunk holds the draws of the groups its pairs belong to and may end inside
 * a group, whose draws then travel again.  Every pair is computed alone, so no result depends on the
 * chunking; a group whose own draws and one of its windows do not fit beside the tables is refused,
 * naming the group and the window.  No load touches memory outside draws, observed and the tables.
 * Checked before any device call, the error text naming the offender: no NULL argument but the
 * outputs, num_groups >= 1, num_draws >= 2, T >= 1, scale and shift finite, num_windows in [1, 64],
 * first >= 0, count >= 0, first + count <= T, num_ranks in [1, 8], ranks in [0, N). */
int ci_summarize_draw_paths_f64(int32_t device, int32_t num_groups, int32_t num_draws, int32_t T,
                                const double* draws, const double* scale, const double* shift,
                                const double* observed, int32_t num_windows,
                                const int32_t* first, const int32_t* count,
                                int32_t num_ranks, const int32_t* ranks,
                                double* center, double* spread, double* excursion,
                                double* excursion_order, double* observed_excursion,
                                int32_t* at, int32_t* exceed);

/* Kalman-filter log-likelihood of the trend + regression model for num_evals parameter sets
 * (the objective an HMC / VI fit would use; the reference never
 * evaluates it directly -- upstream it is LinearGaussianStateSpaceModel.log_prob).
 *   theta [num_evals, 3 + P] float64: (sigma_obs, sigma_level, sigma_slope, weights[P])
 *   loglik [num_evals] float64.   One series (num_series must be 1), no seasonal blocks. */
int ci_kalman_loglik(const ci_problem* problem, const ci_series_params* params, const float* y,
                     const uint8_t* mask, const float* X, int32_t num_evals, const double* theta,
                     double* loglik);

/* Device-resident variant for samplers that evaluate l(theta) many times (HMC leapfrogs):
 * data stay in HBM; each eval moves only theta in and (loglik, grad) out.
 *   grad [num_evals, 3 + P] float64 = dl/d(sigma_obs, sigma_level, sigma_slope, weights);
 *   NULL skips the backward pass.
 * ci_ll_session_draw_latents draws, for each theta row, one latent path (Durbin-Koopman) and
 * one posterior-predictive trajectory (what one_step_predictive, causalimpact_lib.py:620-631,
 * does with GibbsSamplerState draws): level/slope/loc/traj are [num_draws, T] float32; RNG
 * stream (seed, chain = rng_chain, iteration = iter0 + draw). */
typedef struct ci_ll_session ci_ll_session;
int ci_ll_session_create(const ci_problem* problem, const ci_series_params* params, const float* y,
                         const uint8_t* mask, const float* X, int32_t max_evals,
                         ci_ll_session** session);
/* The same for ANY model and length (season_change [K,T] as in ci_fit_gibbs): trend + one block
 * of 2-7 seasons and trend-only series of more than 4096 steps are time-parallel
 * (csrc/ci_wide_score.h), other block lists -- or CI_FLAG_SEQUENTIAL_SEASONAL -- take the
 * sequential one-wavefront route (csrc/ci_score_seq.h).  theta / grad rows are then
 * [3 + K + P]: (sigma_obs, sigma_level, sigma_slope, sigma_drift[K], weights[P]). */
int ci_ll_session_create2(const ci_problem* problem, const ci_series_params* params, const float* y,
                          const uint8_t* mask, const float* X, const uint8_t* season_change,
                          int32_t max_evals, ci_ll_session** session);
int ci_ll_session_eval(ci_ll_session* session, int32_t num_evals, const double* theta,
                       double* loglik, double* grad);
int ci_ll_session_draw_latents(ci_ll_session* session, int32_t num_draws, const double* theta,
                               const uint32_t seed[2], uint32_t rng_chain, uint32_t iter0,
                               float* level, float* slope, float* loc, float* traj);
/* Hamiltonian Monte Carlo over the model's parameters entirely on the device: one workgroup per
 * chain runs num_warmup + num_results iterations of num_leapfrog steps (log-likelihood + score by
 * the same time-parallel scans as ci_ll_session_eval).  Warm-up is the three-stage windowed scheme
 * (step size by dual averaging -> doubling windows that re-estimate the diagonal mass -> step
 * size), csrc/ci_hmc.h.  Then ONE launch draws the latent path and the posterior-predictive
 * trajectory of every retained draw (what causalimpact_lib.py:609-632 does with the Gibbs
 * states), and the fit stays resident in HBM until ci_ll_session_hmc_fetch.
 * Target: l(theta) + the reference's inverse-gamma variance priors (causalimpact_lib.py:424-443)
 * + a continuous regression prior (the spike-and-slab prior has no density):
 *   CI_HMC_PRIOR_SLAB       the Gaussian slab of the reference's prior (:451-453);
 *                           theta = (beta[P], log sigma_obs, log sigma_level[, log sigma_slope])
 *   CI_HMC_PRIOR_HORSESHOE  the horseshoe of tfp.sts.SparseLinearRegression (what BASELINE.json's
 *                           north_star names): beta_j = z_j ln_j sqrt(lv_j) gn sqrt(gv) s0;
 *                           theta = (z[P], log ln[P], log lv[P], log gn, log gv, log scales)
 * EXTENSION (upstream analogues tfp.sts.fit_with_hmc /
 * tfp.experimental.mcmc.windowed_adaptive_hmc; the reference itself has no HMC path).  RNG stream
 * (seed, chain = chain_offset + c): results do not depend on how chains are split over devices.
 * init_theta (optional): [num_chains, dim] unconstrained starting points, e.g. draws of a fitted
 * surrogate posterior; NULL starts from the Gibbs sampler's initial state.
 * kernel_ms (optional, 2 floats): HIP-event durations on the session's stream of the HMC kernel
 * and of the latent/predictive pass. */
#define CI_HMC_PRIOR_SLAB 0
#define CI_HMC_PRIOR_HORSESHOE 1
typedef struct ci_hmc_options {
  int32_t num_chains, chain_offset;
  int32_t num_warmup, num_results, num_leapfrog;
  int32_t prior;                 /* CI_HMC_PRIOR_* */
  double target_accept;          /* dual-averaging target (0.75 upstream) */
  double initial_step_size;
  double horseshoe_scale;        /* s0 = weights_prior_scale (horseshoe only) */
  uint32_t seed[2];
} ci_hmc_options;
int ci_ll_session_hmc_run(ci_ll_session* session, const ci_hmc_options* options,
                          const double* init_theta, float* kernel_ms);
/* Copies the finished fit to the host; every pointer may be NULL.  draws [num_chains,
 * num_results, 3 + P] float64 rows (sigma_obs, sigma_level, sigma_slope, beta); accept_rate,
 * step_size [num_chains]; outputs: the sample container of ci_fit_gibbs with B = 1 (seasonal
 * fields ignored). */
int ci_ll_session_hmc_fetch(ci_ll_session* session, double* draws, double* accept_rate,
                            double* step_size, ci_outputs* outputs);
/* B series in one session, for a batched HMC fit: B x num_chains workgroups of the hmc_kernel in
 * one launch (chain c of series b = workgroup b * num_chains + c).  Trend models only: no seasonal
 * blocks, T <= 4096, P <= 128; everything is validated before the first device call.
 *   params [B]; y, mask [B, T]; X [B, T, P] (row-major, NULL when P = 0).
 * Honours problem->num_series = B, series_offset and CI_FLAG_SHARED_SERIES_STREAMS as ci_fit_gibbs
 * does: series b draws from the Philox key ci_series_stream_key(seed, series_offset + b), or from
 * seed itself with shared streams -- series b then equals a one-series session with that key, and a
 * batch split into parts with matching series_offset equals the whole.
 * On such a session ci_ll_session_hmc_run's num_chains is per series and init_theta is
 * [B, num_chains, dim]; ci_ll_session_hmc_fetch returns draws [B, num_chains, num_results, 3 + P],
 * accept_rate and step_size [B, num_chains] and the ci_fit_gibbs container with this B;
 * horseshoe_scale applies to every series.  ci_ll_session_eval and ci_ll_session_draw_latents
 * refuse sessions of more than one series.  A device allocation that fails returns an error. */
int ci_ll_session_create_batch(const ci_problem* problem, const ci_series_params* params,
                               const float* y, const uint8_t* mask, const float* X,
                               int32_t max_evals, ci_ll_session** session);
/* ci_session_summarize for the posterior-predictive trajectories of the last ci_ll_session_hmc_run
 * (any session, B series): same arguments, same outputs, same kernels; the float32 [B, C, S, T]
 * trajectories are read where they are, in HBM. */
int ci_ll_session_hmc_summarize(ci_ll_session* session, const double* scale, const double* shift,
                                const double* observed, const uint8_t* flags, int32_t num_ranks,
                                const int32_t* ranks, double* value_order, double* cum_order,
                                double* per_draw, double* per_draw_order);
/* ci_session_pool_trajectories for the trajectories of the last ci_ll_session_hmc_run (any session,
 * B series, N = num_chains x num_results): same arguments, same arithmetic, same kernel. */
int ci_ll_session_pool_trajectories(ci_ll_session* session, const double* scale, const double* shift,
                                    int32_t num_groups, const int32_t* offsets,
                                    const int32_t* members, const double* weights, const double* init,
                                    double* out);
/* ci_session_summarize_windows for the trajectories of the last ci_ll_session_hmc_run (any session,
 * B series, N = num_chains x num_results): same arguments, same checks, same arithmetic, same
 * kernel; T is the session's T. */
int ci_ll_session_summarize_windows(ci_ll_session* session, const double* scale, const double* shift,
                                    const double* observed, int32_t num_windows,
                                    const int32_t* first, const int32_t* count,
                                    int32_t num_ranks, const int32_t* ranks,
                                    double* per_draw, double* per_draw_order);
/* ci_session_summarize_paths for the trajectories of the last ci_ll_session_hmc_run (any session,
 * B series, N = num_chains x num_results): same arguments, same checks, same arithmetic, same
 * kernels; T is the session's T. */
int ci_ll_session_summarize_paths(ci_ll_session* session, const double* scale, const double* shift,
                                  const double* observed, int32_t num_windows,
                                  const int32_t* first, const int32_t* count,
                                  int32_t num_ranks, const int32_t* ranks,
                                  double* center, double* spread, double* excursion,
                                  double* excursion_order, double* observed_excursion,
                                  int32_t* at, int32_t* exceed);
int ci_ll_session_kernel_name(const ci_ll_session* session, char* buf, int32_t buflen);
/* Algorithmic bytes of the last configured HMC fit (DESIGN.md "Roofline", cfg3). */
int ci_ll_session_algorithmic_bytes(const ci_ll_session* session, double* bytes);
int ci_ll_session_destroy(ci_ll_session* session);

/* ---- chain gather / diagnostics across the GPUs of one node ----
 * The reference runs one chain in one process and has no communication;
 * BASELINE.json shards independent chains over the GPUs of a node, "RCCL over xGMI only for chain
 * gather/diagnostics".  The fit itself never communicates.  One ci_comm per rank (one rank per
 * GPU); transports:
 *   CI_COMM_RCCL  librccl, loaded on first use: ncclAllGather / ncclAllReduce on device buffers.
 *   CI_COMM_HOST  a POSIX shared-memory segment on one node, for ranks that share a device (RCCL
 *                 refuses two ranks on one GPU) and GPU-less tests; same results, staged via host.
 * ci_comm_unique_id is called by ONE rank; the 128 bytes reach the others out of band (the host
 * package passes them through a file, causalimpact/_comm.py).  ci_comm_create is collective.
 * ranks_seen = ncclCommCount of the live communicator (host transport: attached ranks). */
#define CI_COMM_ID_BYTES 128
#define CI_COMM_RCCL 0
#define CI_COMM_HOST 1
#define CI_COMM_SUM 0
#define CI_COMM_MAX 1
typedef struct ci_comm ci_comm;
int ci_comm_unique_id(int32_t transport, uint8_t* id /* [CI_COMM_ID_BYTES] */);
int ci_comm_create(int32_t transport, const uint8_t* id, int32_t rank, int32_t world,
                   int32_t device, ci_comm** comm);
int ci_comm_info(const ci_comm* comm, int32_t* rank, int32_t* world, int32_t* ranks_seen);
/* Bound of ONE collective on this communicator, seconds (0: $CI_COMM_TIMEOUT_S, default 300).  A
 * collective that exceeds it returns an error; on the RCCL transport the communicator is aborted
 * (ncclCommAbort) so that its kernel leaves the GPU, and every later call on it fails at once. */
int ci_comm_set_timeout(ci_comm* comm, double seconds);
int ci_comm_barrier(ci_comm* comm);
/* values [n] float64 on the host, reduced in place over all ranks (every rank gets the same bits). */
int ci_comm_all_reduce(ci_comm* comm, double* values, int64_t n, int32_t op);
/* send [bytes] -> recv [world, bytes], host buffers, rank order. */
int ci_comm_all_gather(ci_comm* comm, const void* send, void* recv, int64_t bytes);
/* One result array of a finished fit, gathered STRAIGHT FROM HBM (no host round trip on the RCCL
 * transport): every rank's device-resident [B, C, ...] block -> recv [world, B, C, ...] on the
 * host of every rank.  All ranks must hold sessions of the same shape.  field = CI_FIELD_*, the
 * members of ci_outputs in order. */
#define CI_FIELD_OBSERVATION_NOISE_SCALE 0
#define CI_FIELD_LEVEL_SCALE 1
#define CI_FIELD_SLOPE_SCALE 2
#define CI_FIELD_SEASONAL_DRIFT_SCALES 3
#define CI_FIELD_WEIGHTS 4
#define CI_FIELD_LEVEL 5
#define CI_FIELD_SLOPE 6
#define CI_FIELD_SEASONAL_LEVELS 7
#define CI_FIELD_POSTERIOR_MEANS 8
#define CI_FIELD_POSTERIOR_TRAJECTORIES 9
int ci_comm_session_all_gather(ci_comm* comm, ci_session* session, int32_t field, float* recv);
int ci_comm_ll_session_all_gather(ci_comm* comm, ci_ll_session* session, int32_t field, float* recv);
int ci_comm_destroy(ci_comm* comm);

/* ---- component entry points used by the parity tests (tests/test_gpu_*.py) ---- */
/* normals/uniforms/gammas of the specified Philox stream, computed on device. */
int ci_test_rng(int device, const uint32_t seed[2], uint32_t chain, uint32_t iter, uint32_t site,
                uint32_t sub, int32_t n, float* uniforms, float* normals, double alpha,
                double* gamma_draw);
/* One Durbin-Koopman draw of the latent path given residuals and scales
 * (LinearGaussianStateSpaceModel.posterior_sample as reached from
 * gibbs_sampler._resample_latents).  out_latents is [T, d] float32. */
int ci_test_dk_draw(const ci_problem* problem, const ci_series_params* params,
                    const float* resid, const uint8_t* mask, const uint8_t* season_change,
                    double obs_scale, double level_scale, double slope_scale,
                    const double* drift_scales, uint32_t iter, float* out_latents);
/* ci_session_summarize_paths with the limit of its device memory handed in (max_bytes in place of
 * CI_PATHS_MAX_BYTES) and the number of chunks it took written to num_chunks (may be NULL): a test
 * can force several chunks and compare them with one. */
int ci_test_session_summarize_paths(ci_session* session, const double* scale, const double* shift,
                                    const double* observed, int32_t num_windows,
                                    const int32_t* first, const int32_t* count,
                                    int32_t num_ranks, const int32_t* ranks,
                                    double* center, double* spread, double* excursion,
                                    double* excursion_order, double* observed_excursion,
                                    int32_t* at, int32_t* exceed, int64_t max_bytes,
                                    int32_t* num_chunks);
/* ci_summarize_draw_paths_f64 with max_bytes and num_chunks, likewise. */
int ci_test_summarize_draw_paths_f64(int32_t device, int32_t num_groups, int32_t num_draws, int32_t T,
                                     const double* draws, const double* scale, const double* shift,
                                     const double* observed, int32_t num_windows,
                                     const int32_t* first, const int32_t* count,
                                     int32_t num_ranks, const int32_t* ranks,
                                     double* center, double* spread, double* excursion,
                                     double* excursion_order, double* observed_excursion,
                                     int32_t* at, int32_t* exceed, int64_t max_bytes,
                                     int32_t* num_chunks);
/* ci_session_simulate_placebo (blocks == 0) or ci_session_simulate_placebo_blocks (blocks != 0) with
 * the rows of a chunk handed in (max_rows in place of the scratch's B * T; 0: that default; at least
 * max_origins) and the number of chunks it took written to num_chunks (may be NULL), likewise. */
int ci_test_session_simulate_placebo(ci_session* session, int32_t blocks, const double* scale,
                                     const double* shift, int32_t max_origins, const int32_t* origins,
                                     const int32_t* horizon, int32_t link, const double* seen,
                                     int32_t num_ranks, const int32_t* ranks, double* predicted_mean,
                                     double* spread_mean, double* below, double* total_order,
                                     double* totals, int64_t max_rows, int32_t* num_chunks);
/* ci_session_summarize_placebo_horizons with the rows of a chunk handed in (max_rows in place of its
 * own capacity; 0: that default; at least the 3 * max_origins * max_horizons rows of one series) and
 * the number of chunks it took written to num_chunks (may be NULL), likewise. */
int ci_test_session_summarize_placebo_horizons(ci_session* session, const double* scale, const double* shift,
                                               int32_t max_origins, const int32_t* origins,
                                               int32_t max_horizons, const int32_t* horizons,
                                               double* predicted_mean, double* spread_mean, double* pit_mean,
                                               int64_t max_rows, int32_t* num_chunks);
/* ci_session_pool_placebo_blocks with the entries of a chunk handed in (chunk_entries in [1, B] in
 * place of B), likewise: the result does not depend on where the entries are cut. */
int ci_test_session_pool_placebo_blocks(ci_session* session, const double* scale, const double* shift,
                                        int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                        const double* weights, int32_t max_origins,
                                        const int32_t* origins /* [K, O] */, const int32_t* horizon /* [G] */,
                                        const double* init, double* out, const double* seen,
                                        double* predicted_mean, double* spread_mean, double* pit_mean,
                                        int32_t chunk_entries);
/* ci_session_pool_placebo_horizons (blocks == 0) or .._blocks (blocks != 0) with the entries of a
 * chunk handed in (chunk_entries >= 1; the call's own capacity where that is smaller) and the number
 * of chunks it took written to num_chunks (may be NULL), likewise. */
int ci_test_session_pool_placebo_horizons(ci_session* session, int32_t blocks, const double* scale,
                                          const double* shift, int32_t num_groups, const int32_t* offsets,
                                          const int32_t* members, const double* weights, int32_t max_origins,
                                          const int32_t* origins /* [E, O] */, int32_t max_horizons,
                                          const int32_t* horizons /* [G, K] */, const double* init,
                                          double* out /* [G, O, K, 2, N] */, const double* seen /* [G, O, K] */,
                                          double* predicted_mean, double* spread_mean, double* pit_mean,
                                          int32_t chunk_entries, int32_t* num_chunks);
/* ci_session_pool_simulated_placebo (blocks == 0) or .._blocks (blocks != 0) with the entries of a
 * chunk handed in (chunk_entries in [1, B] in place of B), likewise. */
int ci_test_session_pool_simulated_placebo(ci_session* session, int32_t blocks, const double* scale,
                                           const double* shift, int32_t num_groups, const int32_t* offsets,
                                           const int32_t* members, const double* weights, int32_t max_origins,
                                           const int32_t* origins /* [K, O] */, const int32_t* horizon /* [G] */,
                                           int32_t link, const double* init, double* out /* [G, O, N] */,
                                           const double* seen /* [G, O] */, const int32_t* counted /* [G, O] */,
                                           int32_t num_ranks, const int32_t* ranks, double* predicted_mean,
                                           double* spread_mean, double* below,
                                           double* total_order /* [G, R, O] */, int32_t chunk_entries);

#ifdef __cplusplus
}
#endif
#endif  /* CAUSALIMPACT_AMD_H_ */
