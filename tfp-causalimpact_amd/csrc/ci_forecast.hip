// ci_forecast.hip -- the Kalman-filter entries of a finished session behind the C-ABI:
// ci_session_summarize_predictions[_blocks] (kernels: ci_predict.h, ci_predict_blocks.h),
// ci_session_summarize_placebo[_blocks], ci_session_summarize_placebo_horizons, ci_session_simulate_placebo[_blocks],
// ci_session_pool_placebo[_blocks], ci_session_pool_placebo_horizons[_blocks], ci_session_pool_simulated_placebo[_blocks] (kernels: ci_placebo.h,
// ci_placebo_blocks.h) and their ci_test_ entries; and ci_session_create_from_draws[_f64], the session
// that holds what these entries read and nothing else.  A host unit: it instantiates no kernel -- the
// filters are launched through their units' launch functions, the order statistics through
// launch_select of ci_summary.hip (ci_summary_host.h).
//
// Every routine has the same shape: NULL pointers, the session (pred_check_session), the routine's own
// arguments, all before the first device call; then forecast_call, the set-up they share; then the
// routine's own tables, its filter passes through the summary's scratch, and the downloads.
#include <vector>

#include "ci_session.h"
#include "ci_components.h"
#include "ci_placebo.h"
#include "ci_placebo_blocks.h"
#include "ci_predict.h"
#include "ci_predict_blocks.h"
#include "ci_summary_host.h"

// What an entry asks of a session, and a finished run.  `entry`: its public name without _blocks.
// Without `blocks`: a trend with at most one block of 2 to 7 seasons.  With it: not ragged, and a
// state of at most 64 components.
static int pred_check_session(const ci_session* s, bool blocks, const char* entry) {
  const ci_problem& pb = s->pb;
  const std::string name = std::string(entry) + (blocks ? "_blocks" : "");
  const char* who = name.c_str();
  std::string list;
  for (int k = 0; k < pb.num_blocks; ++k) list += (k ? ", " : "") + std::to_string(pb.num_seasons[k]);
  if (!blocks) {
    if (pb.num_blocks > 1 || (pb.num_blocks == 1 && (pb.num_seasons[0] < 2 || pb.num_seasons[0] > 7)))
      return fail("%s takes a trend with at most one block of 2 to 7 seasons, "
                  "this session has the blocks (%s)", who, list.c_str());
  } else {
    if (s->ragged)
      return fail("%s takes no ragged session: their models (one block of 2 to 7 seasons at most) "
                  "belong to the entry without _blocks, %s", who, entry);
    int d = 1 + (pb.has_slope ? 1 : 0);
    for (int k = 0; k < pb.num_blocks; ++k) d += pb.num_seasons[k] - 1;
    if (d > ci::PB_MAX_STATE)
      return fail("%s takes a state of at most %d components, this session has %d with the blocks (%s)",
                  who, ci::PB_MAX_STATE, d, list.c_str());
  }
  if (!s->ran) return fail("%s needs a finished ci_session_run", who);
  return 0;
}

// The block list of a session as the block-model filters read it.
static ci::BlockModel pred_block_model(const ci_problem& pb) {
  ci::BlockModel m = {};
  m.has_slope = pb.has_slope ? 1 : 0;
  m.K = pb.num_blocks;
  m.d = 1 + m.has_slope;
  m.zmask = 1ull;
  for (int k = 0; k < m.K; ++k) {
    m.off[k] = m.d;
    m.ns[k] = pb.num_seasons[k];
    m.zmask |= 1ull << m.d;
    m.d += pb.num_seasons[k] - 1;
  }
  return m;
}

// On the device, once per session: per series the initial moments of its ci_series_params [B, 4],
// then [B] times the 1.0 the regression term is scaled by.
static int pred_init_upload(ci_session* s) {
  if (s->pred_init.p) return 0;
  const int B = s->pb.num_series;
  std::vector<double> init((size_t)5 * B, 1.0);
  for (int b = 0; b < B; ++b) {
    const ci_series_params& q = s->params[b];
    init[4 * b + 0] = q.init_level_loc;
    init[4 * b + 1] = q.init_level_scale * q.init_level_scale;
    init[4 * b + 2] = q.init_slope_scale * q.init_slope_scale;
    init[4 * b + 3] = q.init_seasonal_scale * q.init_seasonal_scale;
  }
  HIP_TRY(s->pred_init.alloc(init.size()));
  HIP_TRY(hipMemcpy(s->pred_init.p, init.data(), init.size() * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

static int check_link(int32_t link) {
  if (link < 0 || link >= ci::NUM_LINKS)
    return fail("link must be CI_LINK_IDENTITY, CI_LINK_LOG or CI_LINK_LOG1P (0 to %d), got %d", ci::NUM_LINKS - 1, link);
  return 0;
}

// What the routines below share once their arguments are checked: the session's geometry (not kpb:
// the inert block of a long trend-only series is no part of the model), its stream and scratch, and
// the filter's inputs.  The routine copies `p` into the argument struct of whichever filter it
// launches (PredArgs, PlaceboArgs::p, PlaceboSimArgs::q.p, or the _blocks structs with `m`).
namespace {
struct ForecastCall {
  int B, T, N, has_slope, NS;      // NS: the seasons of the one-lane build's block (0: none)
  bool f64;                        // the inputs are float64 (a session made from float64 draws): the _f64 launches
  hipStream_t stream;
  SummScratch* w;                  // value: p.out; cum: p.reg; obs [B * T], then scale [B], shift [B]
  ci::PredArgs p;                  // out = `value`, ll = nullptr
  ci::BlockModel m;                // (blocks)
};
}  // namespace

// The set-up of a call, the first device work of every routine: the device, the scratch and the
// initial moments (both on first use), scale and shift next to `obs`, and -- `filters`: the call has
// a row to filter -- the regression term of every draw and step in `cum`, once for all its passes.
static int forecast_call(ForecastCall& c, ci_session* s, bool blocks, const double* scale, const double* shift,
                         bool filters = true) {
  const ci_problem& pb = s->pb;
  const int B = pb.num_series, T = pb.T, P = pb.P, N = pb.num_chains * pb.num_results;
  HIP_TRY(hipSetDevice(pb.device));
  SummScratch& w = s->summ;
  if (summ_scratch_alloc(w, B, T, N)) return 1;
  if (pred_init_upload(s)) return 1;
  double* d_scale = w.obs.p + (size_t)B * T;
  double* d_shift = d_scale + B;
  HIP_TRY(hipMemcpyAsync(d_scale, scale, B * sizeof(double), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(d_shift, shift, B * sizeof(double), hipMemcpyHostToDevice, s->stream));
  const int* d_series_T = s->ragged ? s->series_T.p : nullptr;
  if (P > 0 && filters) {
    if (s->f64)
      HIP_TRY(ci::comp_launch_regression_f64(s->stream, B, N, T, P, s->Xt64.p, s->d_w64.p, d_series_T,
                                             s->pred_init.p + (size_t)4 * B, w.cum.p));
    else
      HIP_TRY(ci::comp_launch_regression(s->stream, B, N, T, P, s->Xt.p, s->o_w.p, d_series_T,
                                         s->pred_init.p + (size_t)4 * B, w.cum.p));
  }
  c.B = B; c.T = T; c.N = N; c.has_slope = pb.has_slope; c.NS = pb.num_blocks ? pb.num_seasons[0] : 0;
  c.stream = s->stream;
  c.w = &w;
  c.f64 = s->f64;
  ci::PredArgs& a = c.p;
  a.N = N; a.T = T;
  a.mask = s->mask.p; a.season_change = s->season_change.p; a.series_T = d_series_T;
  if (s->f64) {
    a.y = s->y64.p;
    a.obs = s->d_obs64.p; a.lscale = s->d_lscale64.p; a.sscale = s->d_sscale64.p; a.drift = s->d_drift64.p;
  } else {
    a.y = s->y.p;
    a.obs = s->o_obs.p; a.lscale = s->o_lscale.p; a.sscale = s->o_sscale.p; a.drift = s->o_drift.p;
  }
  a.init = s->pred_init.p; a.scales = d_scale; a.shifts = d_shift;
  a.reg = P > 0 ? w.cum.p : nullptr;
  a.out = w.value.p; a.ll = nullptr;
  c.m = blocks ? pred_block_model(pb) : ci::BlockModel{};
  return 0;
}

// ci_session_summarize_predictions and, with `blocks`, ci_session_summarize_predictions_blocks: they
// differ in the sessions they take and in the filter they launch, in nothing else.
static int summarize_predictions(ci_session* s, bool blocks, const double* scale, const double* shift,
                                 int32_t num_ranks, const int32_t* ranks, double* forecast_mean,
                                 double* forecast_order, double* variance_mean, double* pit_mean,
                                 double* loglik) {
  if (!s || !scale || !shift || !ranks) return fail("NULL argument");
  if (pred_check_session(s, blocks, "ci_session_summarize_predictions")) return 1;
  const int R = num_ranks;
  if (check_ranks(R, ranks, s->pb.num_chains * s->pb.num_results)) return 1;
  ForecastCall c;
  if (forecast_call(c, s, blocks, scale, shift)) return 1;
  const int B = c.B, T = c.T, N = c.N;
  hipStream_t stream = c.stream;
  SummScratch& w = *c.w;
  HIP_TRY(hipMemcpyAsync(w.ranks.p, ranks, R * sizeof(int), hipMemcpyHostToDevice, stream));
  // One filter pass per requested matrix through `value`, its row means in `obs`, its order
  // statistics in `order`, the per-draw log-likelihoods (with the first pass) in `draw`.
  ci::PredBlocksArgs ab;
  ab.p = c.p; ab.m = c.m;
  bool ll_pending = loglik != nullptr;
  auto pass = [&](int which, double* mean_dst, double* order_dst) -> int {
    ab.p.ll = ll_pending ? w.draw.p : nullptr;
    if (blocks) HIP_TRY((c.f64 ? ci::predict_blocks_launch_f64 : ci::predict_blocks_launch)(stream, B, which, ab));
    else HIP_TRY((c.f64 ? ci::predict_launch_f64 : ci::predict_launch)(stream, B, c.has_slope, c.NS, which, ab.p));
    if (mean_dst) HIP_TRY(ci::comp_launch_row_stats(stream, (size_t)B * T, N, w.value.p, w.obs.p, nullptr));
    if (order_dst)
      HIP_TRY(launch_select(stream, N, T, B * T, R, w.ranks.p, w.value.p, nullptr, w.order.p, nullptr));
    HIP_TRY(hipStreamSynchronize(stream));
    if (mean_dst)
      HIP_TRY(hipMemcpy(mean_dst, w.obs.p, (size_t)B * T * sizeof(double), hipMemcpyDeviceToHost));
    if (order_dst)
      HIP_TRY(hipMemcpy(order_dst, w.order.p, (size_t)B * R * T * sizeof(double), hipMemcpyDeviceToHost));
    if (ll_pending)
      HIP_TRY(hipMemcpy(loglik, w.draw.p, (size_t)B * N * sizeof(double), hipMemcpyDeviceToHost));
    ll_pending = false;
    return 0;
  };
  if ((forecast_mean || forecast_order) && pass(ci::PRED_FORECAST, forecast_mean, forecast_order)) return 1;
  if (variance_mean && pass(ci::PRED_VARIANCE, variance_mean, nullptr)) return 1;
  if ((pit_mean || ll_pending) && pass(ci::PRED_PIT, pit_mean, nullptr)) return 1;
  return 0;
}

// The origin table of ci_session_summarize_placebo and ci_session_simulate_placebo: max_origins in
// [1, T], horizon >= 1, every row ascending with -1 only at the end, o + H_b <= T_b.
static int check_placebo_plan(const ci_session* s, int O, const int32_t* origins, const int32_t* horizon) {
  const int B = s->pb.num_series, T = s->pb.T;
  if (O < 1 || O > T) return fail("max_origins must be in [1, %d], got %d", T, O);
  for (int b = 0; b < B; ++b) {
    const int Tb = s->ragged ? s->lengths[b] : T, Hb = horizon[b];
    if (Hb < 1) return fail("horizon[%d] must be at least 1, got %d", b, Hb);
    const int32_t* row = origins + (size_t)b * O;
    bool ended = false;
    for (int i = 0; i < O; ++i) {
      const int o = row[i];
      if (o == -1) { ended = true; continue; }
      if (o < 0) return fail("origins[%d, %d] must be a step or -1 (unused), got %d", b, i, o);
      if (ended || (i > 0 && o <= row[i - 1]))
        return fail("origins[%d] must be strictly ascending with the unused slots (-1) at the end "
                    "(slot %d holds %d)", b, i, o);
      if ((long long)o + Hb > Tb)
        return fail("origins[%d, %d] = %d with horizon %d reaches beyond the series' %d steps", b, i, o, Hb, Tb);
    }
  }
  return 0;
}

// ci_session_summarize_placebo and, with `blocks`, ci_session_summarize_placebo_blocks, likewise.
static int summarize_placebo(ci_session* s, bool blocks, const double* scale, const double* shift,
                             int32_t max_origins, const int32_t* origins, const int32_t* horizon,
                             double* predicted_mean, double* spread_mean, double* pit_mean) {
  if (!s || !scale || !shift || !origins || !horizon) return fail("NULL argument");
  if (pred_check_session(s, blocks, "ci_session_summarize_placebo")) return 1;
  const int O = max_origins;
  if (check_placebo_plan(s, O, origins, horizon)) return 1;
  ForecastCall c;
  if (forecast_call(c, s, blocks, scale, shift)) return 1;
  const int B = c.B, N = c.N;
  hipStream_t stream = c.stream;
  SummScratch& w = *c.w;
  DevBuf<int> d_plan;                    // origins [B, O], then horizon [B]
  HIP_TRY(d_plan.alloc((size_t)B * O + B));
  HIP_TRY(hipMemcpyAsync(d_plan.p, origins, (size_t)B * O * sizeof(int), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_plan.p + (size_t)B * O, horizon, B * sizeof(int), hipMemcpyHostToDevice, stream));
  // One pass per requested matrix [B * O, N] through `value` (O <= T: it fits), its row means in `obs`.
  ci::PlaceboBlocksArgs ab;
  ci::PlaceboArgs& a = ab.q;
  a.p = c.p; ab.m = c.m;
  a.O = O; a.origins = d_plan.p; a.horizon = d_plan.p + (size_t)B * O;
  auto pass = [&](int which, double* mean_dst) -> int {
    if (blocks) HIP_TRY((c.f64 ? ci::placebo_blocks_launch_f64 : ci::placebo_blocks_launch)(stream, B, which, ab));
    else HIP_TRY((c.f64 ? ci::placebo_launch_f64 : ci::placebo_launch)(stream, B, c.has_slope, c.NS, which, a));
    HIP_TRY(ci::comp_launch_row_stats(stream, (size_t)B * O, N, w.value.p, w.obs.p, nullptr));
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy(mean_dst, w.obs.p, (size_t)B * O * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
  };
  if (predicted_mean && pass(ci::PLACEBO_SUM, predicted_mean)) return 1;
  if (spread_mean && pass(ci::PLACEBO_SPREAD, spread_mean)) return 1;
  if (pit_mean && pass(ci::PLACEBO_PIT, pit_mean)) return 1;
  HIP_TRY(hipStreamSynchronize(stream));   // (the uploads of a call that asks for nothing)
  return 0;
}

// The horizon table of ci_session_summarize_placebo_horizons: max_horizons in [1, 64], every row with
// at least one horizon, >= 1, strictly ascending, -1 only at the end.  last [B]: the row's largest.
// ci_session_pool_placebo_horizons has one row per group (`owner`: what a row belongs to).
static int check_horizon_table(int B, int K, const int32_t* horizons, std::vector<int32_t>& last,
                               const char* owner = "series") {
  if (K < 1 || K > 64) return fail("max_horizons must be in [1, 64], got %d", K);
  last.assign(B, 0);
  for (int b = 0; b < B; ++b) {
    const int32_t* row = horizons + (size_t)b * K;
    bool ended = false;
    for (int i = 0; i < K; ++i) {
      const int h = row[i];
      if (h == -1) { ended = true; continue; }
      if (h < 1) return fail("horizons[%d, %d] must be at least 1, or -1 (unused), got %d", b, i, h);
      if (ended || (i > 0 && h <= row[i - 1]))
        return fail("horizons[%d] must be strictly ascending with the unused slots (-1) at the end "
                    "(slot %d holds %d)", b, i, h);
      last[b] = h;
    }
    if (last[b] < 1) return fail("horizons[%d] holds no horizon: every %s needs at least one", b, owner);
  }
  return 0;
}

// ci_session_summarize_placebo_horizons: summarize_placebo's three outputs at K horizons per series
// from ONE filter pass per chunk of whole series.  The chunk's three planes [nb * O * K, N] lie in
// `value` where one series' 3 * O * K rows fit the scratch's B * T, else in a buffer of the call's own
// of at most CI_PATHS_MAX_BYTES; comp_launch_row_stats then takes the wanted planes' row means.  Every
// value is a function of (b, slot, k, n) alone and every mean one of its row, so nothing depends on
// where the chunks are cut.  max_rows (tests; 0: the capacity above): the rows of a chunk; num_chunks
// (may be NULL): how many it took.
static int summarize_placebo_horizons(ci_session* s, const double* scale, const double* shift,
                                      int32_t max_origins, const int32_t* origins, int32_t max_horizons,
                                      const int32_t* horizons, double* predicted_mean, double* spread_mean,
                                      double* pit_mean, int64_t max_rows, int32_t* num_chunks) {
  if (!s || !scale || !shift || !origins || !horizons) return fail("NULL argument");
  if (pred_check_session(s, false, "ci_session_summarize_placebo_horizons")) return 1;
  const ci_problem& pb = s->pb;
  const int B = pb.num_series, T = pb.T, N = pb.num_chains * pb.num_results;
  const int O = max_origins, K = max_horizons;
  std::vector<int32_t> last;
  if (check_horizon_table(B, K, horizons, last)) return 1;
  if (check_placebo_plan(s, O, origins, last.data())) return 1;
  const size_t per = (size_t)3 * O * K;          // the rows of one series, all planes
  const size_t scratch_rows = (size_t)B * T;
  const size_t own_rows = (size_t)CI_PATHS_MAX_BYTES / sizeof(double) / N;
  const bool in_scratch = per <= scratch_rows;
  if (!in_scratch && per > own_rows)
    return fail("ci_session_summarize_placebo_horizons: the %d origins x %d horizons of one series (series 0) "
                "take %zu bytes of device memory for %d draws, the limit is %lld", O, K,
                per * N * sizeof(double), N, (long long)CI_PATHS_MAX_BYTES);
  if (max_rows < 0 || (max_rows > 0 && (size_t)max_rows < per))
    return fail("max_rows must hold the %zu rows of one series (3 x %d origins x %d horizons), got %lld", per, O,
                K, (long long)max_rows);
  size_t cap = in_scratch ? scratch_rows : own_rows;
  if (max_rows > 0 && (size_t)max_rows < cap) cap = (size_t)max_rows;
  size_t fit = cap / per;
  fit = fit > 65535 ? 65535 : fit;               // (grid.y)
  const int nb_max = fit < (size_t)B ? (int)fit : B;
  if (num_chunks) *num_chunks = (B + nb_max - 1) / nb_max;
  ForecastCall c;
  if (forecast_call(c, s, false, scale, shift)) return 1;
  hipStream_t stream = c.stream;
  SummScratch& w = *c.w;
  const size_t BO = (size_t)B * O, BK = (size_t)B * K, BOK = BO * K;
  DevBuf<int> d_plan;                    // origins [B, O], then horizons [B, K]
  DevBuf<double> d_mean, d_own;          // the three outputs [3, B, O, K]; the planes of a chunk (not in_scratch)
  HIP_TRY(d_plan.alloc(BO + BK));
  HIP_TRY(d_mean.alloc(3 * BOK));
  if (!in_scratch) HIP_TRY(d_own.alloc((size_t)nb_max * per * N));
  HIP_TRY(hipMemcpyAsync(d_plan.p, origins, BO * sizeof(int), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_plan.p + BO, horizons, BK * sizeof(int), hipMemcpyHostToDevice, stream));
  double* const dst[3] = {predicted_mean, spread_mean, pit_mean};
  ci::PlaceboHorizonsArgs a;
  a.p = c.p;
  a.p.out = in_scratch ? w.value.p : d_own.p;
  a.O = O; a.origins = d_plan.p; a.K = K; a.horizons = d_plan.p + BO;
  for (int b0 = 0; b0 < B; b0 += nb_max) {
    const int nb = B - b0 < nb_max ? B - b0 : nb_max;
    a.b0 = b0;
    a.rows = (size_t)nb * O * K;
    HIP_TRY((c.f64 ? ci::placebo_horizons_launch_f64 : ci::placebo_horizons_launch)(stream, nb, c.has_slope, c.NS, a));
    for (int plane = 0; plane < 3; ++plane)
      if (dst[plane])
        HIP_TRY(ci::comp_launch_row_stats(stream, a.rows, N, a.p.out + (size_t)plane * a.rows * N,
                                          d_mean.p + (size_t)plane * BOK + (size_t)b0 * O * K, nullptr));
  }
  HIP_TRY(hipStreamSynchronize(stream));
  for (int plane = 0; plane < 3; ++plane)
    if (dst[plane])
      HIP_TRY(hipMemcpy(dst[plane], d_mean.p + (size_t)plane * BOK, BOK * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// The Philox key every series' fit ran on (ci_series_stream_key of its id, or the seed itself), [B, 2]:
// what the simulated routines draw their normals from.  `keys` is the caller's: it outlives the copy.
static int stream_keys_upload(const ci_session* s, std::vector<uint32_t>& keys, DevBuf<uint32_t>& d_keys) {
  const ci_problem& pb = s->pb;
  const int B = pb.num_series;
  keys.resize((size_t)2 * B);
  const int shared = (pb.flags & CI_FLAG_SHARED_SERIES_STREAMS) ? -1 : 0;
  for (int b = 0; b < B; ++b) {
    const int sid = s->ids.empty() ? pb.series_offset + b : s->ids[b];
    keys[2 * b] = ci::stream_key0(pb.seed[0], shared, sid);
    keys[2 * b + 1] = ci::stream_key1(pb.seed[1], shared, sid);
  }
  HIP_TRY(d_keys.alloc(keys.size()));
  HIP_TRY(hipMemcpyAsync(d_keys.p, keys.data(), keys.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
  return 0;
}

// The statistics of `rows` rows of simulated totals in `value`, O rows per series or group; every
// destination is on the device and may be NULL (not asked for): the row means, the order statistics
// [rows / O, R, O], the rows' download when `totals` (host) is wanted, the count below `seen`, the
// rewrite to (x - seen)^2 in place and its row means.  `value` holds the squares afterwards.
static int sim_total_stats(hipStream_t stream, SummScratch& w, size_t rows, int N, int O, int R,
                           const double* d_seen, const int* d_counted, double* d_mean, double* d_order,
                           double* d_below, double* d_spread, double* totals = nullptr) {
  if (d_mean) HIP_TRY(ci::comp_launch_row_stats(stream, rows, N, w.value.p, d_mean, nullptr));
  if (d_order)
    HIP_TRY(launch_select(stream, N, O, (int)rows, R, w.ranks.p, w.value.p, nullptr, d_order, nullptr));
  if (totals) {
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipMemcpy(totals, w.value.p, rows * N * sizeof(double), hipMemcpyDeviceToHost));
  }
  if (d_spread || d_below) {
    HIP_TRY(ci::placebo_sim_seen_launch(stream, rows, N, w.value.p, d_seen, d_counted, d_below, d_spread != nullptr));
    if (d_spread) HIP_TRY(ci::comp_launch_row_stats(stream, rows, N, w.value.p, d_spread, nullptr));
  }
  return 0;
}

// ci_session_simulate_placebo and, with `blocks`, ci_session_simulate_placebo_blocks: the filter runs
// ONCE per chunk of series whose rows [nb * O, N] fit the scratch -- simulate into `value`, then
// sim_total_stats.  TOTAL is a function of (b, slot, n) alone and every statistic one of its row, so
// nothing depends on where the chunks are cut.  max_rows (tests; 0: the scratch's B * T rows, which
// hold every call's B * O): the rows of a chunk; num_chunks (may be NULL): how many it took.
static int simulate_placebo(ci_session* s, bool blocks, const double* scale, const double* shift,
                            int32_t max_origins, const int32_t* origins, const int32_t* horizon, int32_t link,
                            const double* seen, int32_t num_ranks, const int32_t* ranks, double* predicted_mean,
                            double* spread_mean, double* below, double* total_order, double* totals,
                            int64_t max_rows, int32_t* num_chunks) {
  if (!s || !scale || !shift || !origins || !horizon || !ranks) return fail("NULL argument");
  if (pred_check_session(s, blocks, "ci_session_simulate_placebo")) return 1;
  const ci_problem& pb = s->pb;
  const int B = pb.num_series, T = pb.T, N = pb.num_chains * pb.num_results;
  const int O = max_origins, R = num_ranks;
  if (check_placebo_plan(s, O, origins, horizon)) return 1;
  if (check_link(link)) return 1;
  if (check_ranks(R, ranks, N)) return 1;
  if (!seen && (spread_mean || below)) return fail("spread_mean and below need `seen`, which is NULL");
  const size_t BO = (size_t)B * O;
  if (max_rows < 0 || (max_rows > 0 && max_rows < O))
    return fail("max_rows must hold the %d rows of one series, got %lld", O, (long long)max_rows);
  const size_t cap = max_rows > 0 && (size_t)max_rows < (size_t)B * T ? (size_t)max_rows : (size_t)B * T;
  const int nb_max = (int)(cap / O);     // (O <= T: at least one series)
  if (num_chunks) *num_chunks = (B + nb_max - 1) / nb_max;
  ForecastCall c;
  if (forecast_call(c, s, blocks, scale, shift)) return 1;
  hipStream_t stream = c.stream;
  SummScratch& w = *c.w;
  std::vector<uint32_t> keys;
  DevBuf<int> d_plan;                    // origins [B, O], horizon [B], counted [B, O]
  DevBuf<uint32_t> d_keys;               // [B, 2]
  DevBuf<double> d_stat;                 // seen, mean, spread, below: [B, O] each
  HIP_TRY(d_plan.alloc(2 * BO + B));
  HIP_TRY(d_stat.alloc(4 * BO));
  int* d_counted = d_plan.p + BO + B;
  double *d_seen = d_stat.p, *d_mean = d_stat.p + BO, *d_spread = d_stat.p + 2 * BO, *d_below = d_stat.p + 3 * BO;
  HIP_TRY(hipMemcpyAsync(d_plan.p, origins, BO * sizeof(int), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_plan.p + BO, horizon, B * sizeof(int), hipMemcpyHostToDevice, stream));
  if (stream_keys_upload(s, keys, d_keys)) return 1;
  if (seen) HIP_TRY(hipMemcpyAsync(d_seen, seen, BO * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(w.ranks.p, ranks, R * sizeof(int), hipMemcpyHostToDevice, stream));
  ci::PlaceboBlocksSimArgs ab;
  ci::PlaceboSimArgs& a = ab.s;
  a.q.p = c.p; ab.m = c.m;
  a.q.O = O; a.q.origins = d_plan.p; a.q.horizon = d_plan.p + BO;
  a.kept = pb.num_results; a.chain_offset = (uint32_t)pb.chain_offset; a.keys = d_keys.p;
  for (int b0 = 0; b0 < B; b0 += nb_max) {
    const int nb = B - b0 < nb_max ? B - b0 : nb_max;
    const size_t rows = (size_t)nb * O, off = (size_t)b0 * O;
    a.b0 = b0;
    a.counted = d_counted + off;
    if (blocks) HIP_TRY((c.f64 ? ci::placebo_blocks_sim_launch_f64 : ci::placebo_blocks_sim_launch)(stream, nb, link, ab));
    else HIP_TRY((c.f64 ? ci::placebo_sim_launch_f64 : ci::placebo_sim_launch)(stream, nb, c.has_slope, c.NS, link, a));
    if (sim_total_stats(stream, w, rows, N, O, R, d_seen + off, d_counted + off,
                        predicted_mean ? d_mean + off : nullptr,
                        total_order ? w.order.p + (size_t)b0 * R * O : nullptr, below ? d_below + off : nullptr,
                        spread_mean ? d_spread + off : nullptr, totals ? totals + off * N : nullptr))
      return 1;
  }
  HIP_TRY(hipStreamSynchronize(stream));
  if (predicted_mean) HIP_TRY(hipMemcpy(predicted_mean, d_mean, BO * sizeof(double), hipMemcpyDeviceToHost));
  if (spread_mean) HIP_TRY(hipMemcpy(spread_mean, d_spread, BO * sizeof(double), hipMemcpyDeviceToHost));
  if (below) HIP_TRY(hipMemcpy(below, d_below, BO * sizeof(double), hipMemcpyDeviceToHost));
  if (total_order)
    HIP_TRY(hipMemcpy(total_order, w.order.p, BO * R * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// The plan of a pooled placebo call (ci_session_pool_placebo, ci_session_pool_simulated_placebo):
// one horizon >= 1 per group, every entry's origin row ascending with -1 only at the end and
// o + H_g <= T_b of its member; entry_horizon [K] is the group's horizon per entry.
static int check_pool_plan(const ci_session* s, int G, const int32_t* offsets, const int32_t* members, int O,
                           const int32_t* origins, const int32_t* horizon, std::vector<int>& entry_horizon) {
  const int T = s->pb.T, K = offsets[G];
  entry_horizon.assign((size_t)(K ? K : 1), 0);
  for (int g = 0; g < G; ++g) {
    const int Hg = horizon[g];
    if (Hg < 1) return fail("group %d: the horizon must be at least 1, got %d", g, Hg);
    for (int k = offsets[g]; k < offsets[g + 1]; ++k) {
      const int b = members[k], Tb = s->ragged ? s->lengths[b] : T;
      const int32_t* row = origins + (size_t)k * O;
      entry_horizon[k] = Hg;
      bool ended = false;
      for (int i = 0; i < O; ++i) {
        const int o = row[i];
        if (o == -1) { ended = true; continue; }
        if (o < 0)
          return fail("group %d, entry %d (member %d): slot %d must hold a step or -1 (unused), got %d", g, k, b, i, o);
        if (ended || (i > 0 && o <= row[i - 1]))
          return fail("group %d, entry %d (member %d): the origins must be strictly ascending with the unused "
                      "slots (-1) at the end (slot %d holds %d)", g, k, b, i, o);
        if ((long long)o + Hg > Tb)
          return fail("group %d, entry %d (member %d): the origin %d of slot %d with horizon %d reaches beyond "
                      "the series' %d steps", g, k, b, o, i, Hg, Tb);
      }
    }
  }
  return 0;
}

// The device copy of a pooled call's group table, the call's own: the K entries (an empty table
// keeps one slot: Ka = 1) and the groups' accumulators [G, O, planes, N] holding `init` or zeros.
// tail_ints, tail_doubles: room behind them for what the routine keeps per row besides.
namespace {
struct PoolTables {
  DevBuf<int> ints;                // offsets [G + 1], members [Ka], horizon [Ka], origins [Ka, O], tail
  DevBuf<double> doubles;          // acc, weights [Ka], tail
  int *offsets, *members, *horizon, *origins, *tail_ints;
  double *acc, *weights, *tail_doubles;
  size_t acc_n;
};
}  // namespace

static int pool_tables_upload(PoolTables& t, hipStream_t stream, int G, int O, int N, int planes,
                              const int32_t* offsets, const int32_t* members, const double* weights,
                              const int32_t* origins, const std::vector<int>& entry_horizon, const double* init,
                              size_t tail_ints, size_t tail_doubles) {
  const size_t K = (size_t)offsets[G], Ka = K ? K : 1;
  t.acc_n = (size_t)G * O * planes * N;
  HIP_TRY(t.ints.alloc((size_t)G + 1 + 2 * Ka + Ka * O + tail_ints));
  HIP_TRY(t.doubles.alloc(t.acc_n + Ka + tail_doubles));
  t.offsets = t.ints.p;
  t.members = t.offsets + G + 1;
  t.horizon = t.members + Ka;
  t.origins = t.horizon + Ka;
  t.tail_ints = t.origins + Ka * O;
  t.acc = t.doubles.p;
  t.weights = t.acc + t.acc_n;
  t.tail_doubles = t.weights + Ka;
  HIP_TRY(hipMemcpyAsync(t.offsets, offsets, ((size_t)G + 1) * sizeof(int), hipMemcpyHostToDevice, stream));
  if (K > 0) {
    HIP_TRY(hipMemcpyAsync(t.members, members, K * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(t.horizon, entry_horizon.data(), K * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(t.origins, origins, K * O * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(t.weights, weights, K * sizeof(double), hipMemcpyHostToDevice, stream));
  }
  if (init)
    HIP_TRY(hipMemcpyAsync(t.acc, init, t.acc_n * sizeof(double), hipMemcpyHostToDevice, stream));
  else
    HIP_TRY(hipMemsetAsync(t.acc, 0, t.acc_n * sizeof(double), stream));
  return 0;
}

// The placebo forecasts of POOLED sums: per group, slot and draw the weighted sum S of the members'
// forecasts and the sum U of their predictive variances (include/causalimpact_amd.h).  The entries
// of the group table pass through `value` at most B at a time, a SUM pass and its accumulate, then a
// VAR pass and its accumulate; the accumulators [G, O, 2, N] and the tables are the call's own.
// With `blocks` ci_session_pool_placebo_blocks: the sessions and the filter of the block models, ONE
// pass per chunk that stores SUM into `value` and VAR into a buffer of the call's own, then the same
// two accumulates.  chunk_entries (tests; 0: B): the entries of a chunk, in [1, B].
static int pool_placebo(ci_session* s, bool blocks, const double* scale, const double* shift,
                        int32_t num_groups, const int32_t* offsets, const int32_t* members,
                        const double* weights, int32_t max_origins, const int32_t* origins,
                        const int32_t* horizon, const double* init, double* out,
                        const double* seen, double* predicted_mean, double* spread_mean,
                        double* pit_mean, int32_t chunk_entries) {
  if (!s || !scale || !shift || !offsets || !members || !weights || !origins || !horizon || !out)
    return fail("NULL argument");
  if (pred_check_session(s, blocks, "ci_session_pool_placebo")) return 1;
  const int B = s->pb.num_series, T = s->pb.T, O = max_origins, G = num_groups;
  if (chunk_entries < 0 || chunk_entries > B)
    return fail("chunk_entries must be in [1, %d] (the session's series), got %d", B, chunk_entries);
  const int chunk = chunk_entries ? chunk_entries : B;
  if (check_groups(B, G, offsets, members, weights)) return 1;
  if (O < 1 || O > T) return fail("max_origins must be in [1, %d], got %d", T, O);
  if (!seen && (predicted_mean || spread_mean || pit_mean))
    return fail("predicted_mean, spread_mean and pit_mean need `seen`, the pooled observed sums");
  const int K = offsets[G];
  std::vector<int> entry_horizon;
  if (check_pool_plan(s, G, offsets, members, O, origins, horizon, entry_horizon)) return 1;
  ForecastCall c;
  if (forecast_call(c, s, blocks, scale, shift, K > 0)) return 1;
  const int N = c.N;
  hipStream_t stream = c.stream;
  SummScratch& w = *c.w;
  const size_t rows = (size_t)G * O;
  PoolTables t;                          // tail: seen [G, O]
  DevBuf<double> d_var;                  // (blocks) VAR of a chunk [chunk, O, N]
  if (pool_tables_upload(t, stream, G, O, N, 2, offsets, members, weights, origins, entry_horizon, init, 0, rows))
    return 1;
  if (blocks && K > 0) HIP_TRY(d_var.alloc((size_t)(K < chunk ? K : chunk) * O * N));
  double* d_seen = t.tail_doubles;
  if (seen) HIP_TRY(hipMemcpyAsync(d_seen, seen, rows * sizeof(double), hipMemcpyHostToDevice, stream));
  ci::PlaceboBlocksPoolArgs ab;
  ci::PlaceboArgs& a = ab.q;
  a.p = c.p; ab.m = c.m; ab.var = d_var.p;
  a.O = O;
  // at most B entries at a time: [B * O, N] with O <= T fits `value`
  for (int c0 = 0; c0 < K; c0 += chunk) {
    const int c1 = K - c0 < chunk ? K : c0 + chunk;
    a.series_of = t.members + c0; a.origins = t.origins + (size_t)c0 * O; a.horizon = t.horizon + c0;
    if (blocks) {
      HIP_TRY((c.f64 ? ci::placebo_blocks_pool_launch_f64 : ci::placebo_blocks_pool_launch)(stream, c1 - c0, ab));
      HIP_TRY(ci::placebo_pool_launch(stream, N, O, G, 0, c0, c1, t.offsets, t.weights, w.value.p, t.acc));
      HIP_TRY(ci::placebo_pool_launch(stream, N, O, G, 1, c0, c1, t.offsets, t.weights, d_var.p, t.acc));
      continue;
    }
    for (int which = 0; which < 2; ++which) {
      HIP_TRY((c.f64 ? ci::placebo_launch_f64 : ci::placebo_launch)(stream, c1 - c0, c.has_slope, c.NS,
                                                                    which ? ci::PLACEBO_VAR : ci::PLACEBO_SUM, a));
      HIP_TRY(ci::placebo_pool_launch(stream, N, O, G, which, c0, c1, t.offsets, t.weights, w.value.p, t.acc));
    }
  }
  HIP_TRY(hipMemcpyAsync(out, t.acc, t.acc_n * sizeof(double), hipMemcpyDeviceToHost, stream));
  // the means over the draws, one matrix at a time and as many rows as `value` and `obs` hold
  const size_t per_pass = (size_t)B * T;
  auto finish = [&](int which, double* mean_dst) -> int {
    for (size_t r0 = 0; r0 < rows; r0 += per_pass) {
      const size_t nr = rows - r0 < per_pass ? rows - r0 : per_pass;
      HIP_TRY(ci::placebo_finish_launch(stream, N, r0, nr, which, t.acc, d_seen, w.value.p));
      HIP_TRY(ci::comp_launch_row_stats(stream, nr, N, w.value.p, w.obs.p, nullptr));
      HIP_TRY(hipMemcpyAsync(mean_dst + r0, w.obs.p, nr * sizeof(double), hipMemcpyDeviceToHost, stream));
    }
    return 0;
  };
  if (predicted_mean && finish(ci::PLACEBO_SUM, predicted_mean)) return 1;
  if (spread_mean && finish(ci::PLACEBO_SPREAD, spread_mean)) return 1;
  if (pit_mean && finish(ci::PLACEBO_PIT, pit_mean)) return 1;
  HIP_TRY(hipStreamSynchronize(stream));
  return 0;
}

// ci_session_pool_placebo_horizons and, with `blocks`, .._blocks: pool_placebo's accumulators and means
// at K horizons per group from ONE filter pass per chunk of whole entries.  A chunk's two planes
// (SUM, VAR) [ne * O * K, N] lie in `value` where one entry's 2 * O * K rows fit the scratch's B * T,
// else in a buffer of the call's own of at most CI_PATHS_MAX_BYTES; placebo_pool_kernel then adds them
// to the accumulators [G, O * K, 2, N] and placebo_finish_kernel finishes them, both with O * K in the
// place of O.  Every term is a function of (entry, slot, k, n) alone and the accumulate takes a
// group's entries in ascending order whatever the cut, so nothing depends on where the chunks are
// cut.  chunk_entries (tests; 0: the capacity above): the entries of a chunk, at most that capacity;
// num_chunks (may be NULL): how many it took.
static int pool_placebo_horizons(ci_session* s, bool blocks, const double* scale, const double* shift,
                                 int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                 const double* weights, int32_t max_origins, const int32_t* origins,
                                 int32_t max_horizons, const int32_t* horizons, const double* init, double* out,
                                 const double* seen, double* predicted_mean, double* spread_mean,
                                 double* pit_mean, int32_t chunk_entries, int32_t* num_chunks) {
  if (!s || !scale || !shift || !offsets || !members || !weights || !origins || !horizons || !out)
    return fail("NULL argument");
  if (pred_check_session(s, blocks, "ci_session_pool_placebo_horizons")) return 1;
  const char* who = blocks ? "ci_session_pool_placebo_horizons_blocks" : "ci_session_pool_placebo_horizons";
  const ci_problem& pb = s->pb;
  const int B = pb.num_series, T = pb.T, N = pb.num_chains * pb.num_results;
  const int O = max_origins, K = max_horizons, G = num_groups;
  if (chunk_entries < 0) return fail("chunk_entries must be at least 1, got %d", chunk_entries);
  if (check_groups(B, G, offsets, members, weights)) return 1;
  if (O < 1 || O > T) return fail("max_origins must be in [1, %d], got %d", T, O);
  if (!seen && (predicted_mean || spread_mean || pit_mean))
    return fail("predicted_mean, spread_mean and pit_mean need `seen`, the pooled observed sums");
  std::vector<int32_t> last;             // [G] every group's largest horizon
  if (check_horizon_table(G, K, horizons, last, "group")) return 1;
  const int E = offsets[G];
  std::vector<int> entry_horizon;
  if (check_pool_plan(s, G, offsets, members, O, origins, last.data(), entry_horizon)) return 1;
  const size_t OK = (size_t)O * K, rows = (size_t)G * OK;
  const size_t max_doubles = (size_t)CI_PATHS_MAX_BYTES / sizeof(double);
  if (rows * 2 > max_doubles / N)
    return fail("%s: the accumulators of %d groups x %d origins x %d horizons take %zu bytes of device memory "
                "for %d draws, the limit is %lld: pass the horizon slots in several calls", who, G, O, K,
                rows * 2 * N * sizeof(double), N, (long long)CI_PATHS_MAX_BYTES);
  const size_t per = 2 * OK;                     // the rows of one entry, both planes
  const size_t scratch_rows = (size_t)B * T, own_rows = max_doubles / N;
  const bool in_scratch = per <= scratch_rows;
  if (!in_scratch && per > own_rows)
    return fail("%s: the %d origins x %d horizons of one entry (entry 0) take %zu bytes of device memory for "
                "%d draws, the limit is %lld", who, O, K, per * N * sizeof(double), N, (long long)CI_PATHS_MAX_BYTES);
  size_t fit = (in_scratch ? scratch_rows : own_rows) / per;
  fit = fit > 65535 ? 65535 : fit;               // (grid.y)
  if (chunk_entries > 0 && (size_t)chunk_entries < fit) fit = (size_t)chunk_entries;
  const int chunk = (int)fit;
  if (num_chunks) *num_chunks = (E + chunk - 1) / chunk;
  ForecastCall c;
  if (forecast_call(c, s, blocks, scale, shift, E > 0)) return 1;
  hipStream_t stream = c.stream;
  SummScratch& w = *c.w;
  // the horizon row of every entry: its group's
  const size_t Ea = E ? E : 1;
  std::vector<int32_t> entry_rows(Ea * K, -1);
  for (int g = 0; g < G; ++g)
    for (int k = offsets[g]; k < offsets[g + 1]; ++k)
      std::copy(horizons + (size_t)g * K, horizons + (size_t)(g + 1) * K, entry_rows.begin() + (size_t)k * K);
  PoolTables t;                          // acc [G, O, K, 2, N]; tails: the entries' horizon rows [Ea, K]; seen [G, O, K]
  DevBuf<double> d_own;                  // the planes of a chunk (not in_scratch)
  if (pool_tables_upload(t, stream, G, O, N, 2 * K, offsets, members, weights, origins, entry_horizon, init,
                         Ea * K, rows))
    return 1;
  int* d_rows = t.tail_ints;
  HIP_TRY(hipMemcpyAsync(d_rows, entry_rows.data(), Ea * K * sizeof(int), hipMemcpyHostToDevice, stream));
  const int ne_max = E < chunk ? E : chunk;
  if (!in_scratch && E > 0) HIP_TRY(d_own.alloc((size_t)ne_max * per * N));
  double* d_seen = t.tail_doubles;
  if (seen) HIP_TRY(hipMemcpyAsync(d_seen, seen, rows * sizeof(double), hipMemcpyHostToDevice, stream));
  double* planes = in_scratch ? w.value.p : d_own.p;
  ci::PlaceboPoolHorizonsArgs a;
  a.p = c.p; a.p.out = planes;
  a.O = O; a.K = K;
  ci::PlaceboBlocksPoolHorizonsArgs ab;
  ab.q.p = a.p; ab.m = c.m; ab.q.O = O; ab.K = K; ab.q.horizon = nullptr;
  for (int c0 = 0; c0 < E; c0 += chunk) {
    const int c1 = E - c0 < chunk ? E : c0 + chunk;
    const size_t plane = (size_t)(c1 - c0) * OK * N;   // the doubles of one plane of this chunk
    if (blocks) {
      ab.q.series_of = t.members + c0; ab.q.origins = t.origins + (size_t)c0 * O;
      ab.horizons = d_rows + (size_t)c0 * K; ab.var = planes + plane;
      HIP_TRY((c.f64 ? ci::placebo_blocks_pool_horizons_launch_f64 : ci::placebo_blocks_pool_horizons_launch)(stream, c1 - c0, ab));
    } else {
      a.series_of = t.members + c0; a.origins = t.origins + (size_t)c0 * O;
      a.horizons = d_rows + (size_t)c0 * K; a.rows = (size_t)(c1 - c0) * OK;
      HIP_TRY((c.f64 ? ci::placebo_pool_horizons_launch_f64 : ci::placebo_pool_horizons_launch)(stream, c1 - c0, c.has_slope, c.NS, a));
    }
    HIP_TRY(ci::placebo_pool_launch(stream, N, (int)OK, G, 0, c0, c1, t.offsets, t.weights, planes, t.acc));
    HIP_TRY(ci::placebo_pool_launch(stream, N, (int)OK, G, 1, c0, c1, t.offsets, t.weights, planes + plane, t.acc));
  }
  HIP_TRY(hipMemcpyAsync(out, t.acc, t.acc_n * sizeof(double), hipMemcpyDeviceToHost, stream));
  // the means over the draws, one matrix at a time and as many rows as `value` and `obs` hold
  const size_t per_pass = scratch_rows;
  auto finish = [&](int which, double* mean_dst) -> int {
    for (size_t r0 = 0; r0 < rows; r0 += per_pass) {
      const size_t nr = rows - r0 < per_pass ? rows - r0 : per_pass;
      HIP_TRY(ci::placebo_finish_launch(stream, N, r0, nr, which, t.acc, d_seen, w.value.p));
      HIP_TRY(ci::comp_launch_row_stats(stream, nr, N, w.value.p, w.obs.p, nullptr));
      HIP_TRY(hipMemcpyAsync(mean_dst + r0, w.obs.p, nr * sizeof(double), hipMemcpyDeviceToHost, stream));
    }
    return 0;
  };
  if (predicted_mean && finish(ci::PLACEBO_SUM, predicted_mean)) return 1;
  if (spread_mean && finish(ci::PLACEBO_SPREAD, spread_mean)) return 1;
  if (pit_mean && finish(ci::PLACEBO_PIT, pit_mean)) return 1;
  HIP_TRY(hipStreamSynchronize(stream));
  return 0;
}

// The SIMULATED placebo forecasts of pooled sums (include/causalimpact_amd.h): the entries of the group
// table pass through `value` at most `chunk` at a time -- ONE simulation pass (the entry-table build
// of simulate_placebo's kernel; TOTAL is a function of (series, origin, slot, horizon, n) alone) and
// its accumulate into POOL [G, O, N], the call's own.  `out` is downloaded, then sim_total_stats is
// taken over the accumulators' rows, copied through `value` at most B * T rows at a time (whole
// groups, so that the selection's [G, R, O] layout holds per chunk).  Nothing depends on where either
// kind of chunk is cut.  chunk_entries (tests; 0: B): in [1, B].
static int pool_simulated_placebo(ci_session* s, bool blocks, const double* scale, const double* shift,
                                  int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                  const double* weights, int32_t max_origins, const int32_t* origins,
                                  const int32_t* horizon, int32_t link, const double* init, double* out,
                                  const double* seen, const int32_t* counted, int32_t num_ranks,
                                  const int32_t* ranks, double* predicted_mean, double* spread_mean,
                                  double* below, double* total_order, int32_t chunk_entries) {
  if (!s || !scale || !shift || !offsets || !members || !weights || !origins || !horizon || !out || !ranks)
    return fail("NULL argument");
  if (pred_check_session(s, blocks, "ci_session_pool_simulated_placebo")) return 1;
  const ci_problem& pb = s->pb;
  const int B = pb.num_series, T = pb.T, N = pb.num_chains * pb.num_results;
  const int O = max_origins, G = num_groups, R = num_ranks;
  if (chunk_entries < 0 || chunk_entries > B)
    return fail("chunk_entries must be in [1, %d] (the session's series), got %d", B, chunk_entries);
  const int chunk = chunk_entries ? chunk_entries : B;
  if (check_groups(B, G, offsets, members, weights)) return 1;
  if (O < 1 || O > T) return fail("max_origins must be in [1, %d], got %d", T, O);
  if (check_link(link)) return 1;
  if (check_ranks(R, ranks, N)) return 1;
  const bool stats = predicted_mean || spread_mean || below || total_order;
  if (stats && (!seen || !counted))
    return fail("predicted_mean, spread_mean, below and total_order need `seen` and `counted`, the pooled "
                "observed totals and the member-steps they count");
  const int K = offsets[G];
  std::vector<int> entry_horizon;
  if (check_pool_plan(s, G, offsets, members, O, origins, horizon, entry_horizon)) return 1;
  ForecastCall c;
  if (forecast_call(c, s, blocks, scale, shift, K > 0)) return 1;
  hipStream_t stream = c.stream;
  SummScratch& w = *c.w;
  const size_t rows = (size_t)G * O;
  const size_t chunk_rows = (size_t)(K < chunk ? (K ? K : 1) : chunk) * O;
  std::vector<uint32_t> keys;
  PoolTables t;                          // tails: cnt of a chunk's rows [chunk, O], counted [G, O];
                                         // seen, mean, spread, below [G, O] each, order [G, R, O]
  DevBuf<uint32_t> d_keys;               // [B, 2]
  if (pool_tables_upload(t, stream, G, O, N, 1, offsets, members, weights, origins, entry_horizon, init,
                         chunk_rows + rows, 4 * rows + rows * R))
    return 1;
  int* d_cnt = t.tail_ints;
  int* d_counted = d_cnt + chunk_rows;
  double* d_seen = t.tail_doubles;
  double *d_mean = d_seen + rows, *d_spread = d_mean + rows, *d_below = d_spread + rows;
  double* d_order = d_below + rows;
  if (stats) {
    HIP_TRY(hipMemcpyAsync(d_seen, seen, rows * sizeof(double), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_counted, counted, rows * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(w.ranks.p, ranks, R * sizeof(int), hipMemcpyHostToDevice, stream));
  }
  if (stream_keys_upload(s, keys, d_keys)) return 1;
  ci::PlaceboBlocksSimArgs ab;
  ci::PlaceboSimArgs& a = ab.s;
  a.q.p = c.p; ab.m = c.m;
  a.q.O = O;
  a.b0 = 0; a.kept = pb.num_results; a.chain_offset = (uint32_t)pb.chain_offset; a.keys = d_keys.p;
  a.counted = d_cnt;
  // at most B entries at a time: [B * O, N] with O <= T fits `value`
  for (int c0 = 0; c0 < K; c0 += chunk) {
    const int c1 = K - c0 < chunk ? K : c0 + chunk;
    a.q.series_of = t.members + c0; a.q.origins = t.origins + (size_t)c0 * O; a.q.horizon = t.horizon + c0;
    if (blocks)
      HIP_TRY((c.f64 ? ci::placebo_blocks_sim_entries_launch_f64 : ci::placebo_blocks_sim_entries_launch)(stream, c1 - c0, link, ab));
    else
      HIP_TRY((c.f64 ? ci::placebo_sim_entries_launch_f64 : ci::placebo_sim_entries_launch)(stream, c1 - c0, c.has_slope, c.NS,
                                                                                            link, a));
    HIP_TRY(ci::placebo_pool_totals_launch(stream, N, O, G, c0, c1, t.offsets, t.weights, w.value.p, t.acc));
  }
  HIP_TRY(hipMemcpyAsync(out, t.acc, t.acc_n * sizeof(double), hipMemcpyDeviceToHost, stream));
  if (stats) {
    // whole groups, as many as `value` holds: (B * T / O) * O rows, at least O
    const size_t per_pass = ((size_t)B * T / O) * O;
    for (size_t r0 = 0; r0 < rows; r0 += per_pass) {
      const size_t nr = rows - r0 < per_pass ? rows - r0 : per_pass;
      HIP_TRY(hipMemcpyAsync(w.value.p, t.acc + r0 * N, nr * N * sizeof(double), hipMemcpyDeviceToDevice, stream));
      if (sim_total_stats(stream, w, nr, N, O, R, d_seen + r0, d_counted + r0, predicted_mean ? d_mean + r0 : nullptr,
                          total_order ? d_order + r0 * R : nullptr, below ? d_below + r0 : nullptr,
                          spread_mean ? d_spread + r0 : nullptr))
        return 1;
    }
  }
  HIP_TRY(hipStreamSynchronize(stream));
  if (predicted_mean) HIP_TRY(hipMemcpy(predicted_mean, d_mean, rows * sizeof(double), hipMemcpyDeviceToHost));
  if (spread_mean) HIP_TRY(hipMemcpy(spread_mean, d_spread, rows * sizeof(double), hipMemcpyDeviceToHost));
  if (below) HIP_TRY(hipMemcpy(below, d_below, rows * sizeof(double), hipMemcpyDeviceToHost));
  if (total_order) HIP_TRY(hipMemcpy(total_order, d_order, rows * R * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// ---- A session made from draws (include/causalimpact_amd.h) --------------------------------------
// The filters read the data and the parameter draws, never the fit: this session holds y (masked
// steps zeroed, as a fit's), mask, the design feature-major, season_change, the parameter blocks
// (pred_init_upload) and the five draw arrays -- where a fit leaves them (F = float) or, float64, in
// the session's *64 buffers, which the float64-input builds of the filters read.  No workspace, no
// trajectories, no latents, no kernel pointer, no copy stream.
namespace {
struct DrawsSessionGuard {
  ci_session* s;
  ~DrawsSessionGuard() { if (s) ci_session_destroy(s); }
};

// A scale draw must be finite and not negative: array [B, N], or with `per_block` [B, N, width].
template <class F>
int check_scale_draws(const char* name, const F* x, int B, int N, int width = 1, bool per_block = false) {
  for (int b = 0; b < B; ++b)
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < width; ++k) {
        const double v = (double)x[((size_t)b * N + n) * width + k];
        if (std::isfinite(v) && v >= 0.0) continue;
        if (per_block)
          return fail("%s of series %d, draw %d, block %d must be finite and not negative, got %g", name, b, n, k, v);
        return fail("%s of series %d, draw %d must be finite and not negative, got %g", name, b, n, v);
      }
  return 0;
}

template <class F> int upload(DevBuf<F>& dst, const F* src, size_t n) {
  HIP_TRY(dst.alloc(n));
  if (n) HIP_TRY(hipMemcpy(dst.p, src, n * sizeof(F), hipMemcpyHostToDevice));
  return 0;
}
}  // namespace

template <class F>
static int session_from_draws(const ci_problem* pb, const F* y, const uint8_t* mask, const F* X,
                              const uint8_t* season_change, const ci_series_params* params, const F* obs,
                              const F* lscale, const F* sscale, const F* drift, const F* weights,
                              ci_session** out) {
  constexpr bool F64 = sizeof(F) == sizeof(double);
  if (validate(pb)) return 1;
  if (!y || !mask || !params || !obs || !lscale || !out) return fail("NULL argument");
  if (pb->has_slope && !sscale) return fail("slope_scale is NULL but has_slope is set");
  if (pb->num_blocks > 0 && !season_change) return fail("season_change is NULL but num_blocks > 0");
  if (pb->num_blocks > 0 && !drift) return fail("seasonal_drift_scales is NULL but num_blocks > 0");
  if (pb->P > 0 && !X) return fail("X is NULL but P=%d", pb->P);
  if (pb->P > 0 && !weights) return fail("weights is NULL but P=%d", pb->P);
  const int B = pb->num_series, T = pb->T, P = pb->P, K = pb->num_blocks;
  const int N = pb->num_chains * pb->num_results;
  std::vector<F> yh;
  std::vector<double> n_obs;
  if (stage_outcomes<F>(B, T, nullptr, y, mask, yh, n_obs)) return 1;
  if (check_scale_draws("observation_noise_scale", obs, B, N)) return 1;
  if (check_scale_draws("level_scale", lscale, B, N)) return 1;
  if (pb->has_slope && check_scale_draws("slope_scale", sscale, B, N)) return 1;
  if (K > 0 && check_scale_draws("seasonal_drift_scales", drift, B, N, K, true)) return 1;
  HIP_TRY(hipSetDevice(pb->device));
  ci_session* s = new ci_session();
  DrawsSessionGuard guard{s};
  s->pb = *pb;
  s->kpb = *pb;
  s->from_draws = true;
  s->f64 = F64;
  s->ran = true;
  s->kernel_name = "(made from draws)";
  s->params.assign(params, params + B);
  HIP_TRY(pool_stream_get(&s->stream));
  const size_t BN = (size_t)B * N;
  HIP_TRY(s->mask.alloc((size_t)B * T));
  HIP_TRY(hipMemcpy(s->mask.p, mask, (size_t)B * T, hipMemcpyHostToDevice));
  if (K > 0) {
    HIP_TRY(s->season_change.alloc((size_t)K * T));
    HIP_TRY(hipMemcpy(s->season_change.p, season_change, (size_t)K * T, hipMemcpyHostToDevice));
  }
  const std::vector<F> xt = P > 0 ? transpose_design<F>(B, T, P, X) : std::vector<F>();
  // (no slope: the filters never read sscale; no block: never drift; no design: never Xt and w)
  const size_t n_ss = pb->has_slope ? BN : 0, n_dr = K > 0 ? BN * K : 0, n_w = P > 0 ? BN * P : 0;
  if constexpr (F64) {
    if (upload(s->y64, yh.data(), yh.size()) || upload(s->Xt64, xt.data(), xt.size()) ||
        upload(s->d_obs64, obs, BN) || upload(s->d_lscale64, lscale, BN) || upload(s->d_sscale64, sscale, n_ss) ||
        upload(s->d_drift64, drift, n_dr) || upload(s->d_w64, weights, n_w))
      return 1;
  } else {
    if (upload(s->y, yh.data(), yh.size()) || upload(s->Xt, xt.data(), xt.size()) ||
        upload(s->o_obs, obs, BN) || upload(s->o_lscale, lscale, BN) || upload(s->o_sscale, sscale, n_ss) ||
        upload(s->o_drift, drift, n_dr) || upload(s->o_w, weights, n_w))
      return 1;
  }
  guard.s = nullptr;
  *out = s;
  return 0;
}

extern "C" {

int ci_session_create_from_draws(const ci_problem* pb, const float* y, const uint8_t* mask, const float* X,
                                 const uint8_t* season_change, const ci_series_params* params,
                                 const float* observation_noise_scale, const float* level_scale,
                                 const float* slope_scale, const float* seasonal_drift_scales,
                                 const float* weights, ci_session** out) {
  return session_from_draws<float>(pb, y, mask, X, season_change, params, observation_noise_scale, level_scale,
                                   slope_scale, seasonal_drift_scales, weights, out);
}

int ci_session_create_from_draws_f64(const ci_problem* pb, const double* y, const uint8_t* mask, const double* X,
                                     const uint8_t* season_change, const ci_series_params* params,
                                     const double* observation_noise_scale, const double* level_scale,
                                     const double* slope_scale, const double* seasonal_drift_scales,
                                     const double* weights, ci_session** out) {
  return session_from_draws<double>(pb, y, mask, X, season_change, params, observation_noise_scale, level_scale,
                                    slope_scale, seasonal_drift_scales, weights, out);
}

int ci_session_summarize_predictions(ci_session* s, const double* scale, const double* shift,
                                     int32_t num_ranks, const int32_t* ranks, double* forecast_mean,
                                     double* forecast_order, double* variance_mean, double* pit_mean,
                                     double* loglik) {
  return summarize_predictions(s, false, scale, shift, num_ranks, ranks, forecast_mean, forecast_order,
                               variance_mean, pit_mean, loglik);
}

int ci_session_summarize_predictions_blocks(ci_session* s, const double* scale, const double* shift,
                                            int32_t num_ranks, const int32_t* ranks, double* forecast_mean,
                                            double* forecast_order, double* variance_mean, double* pit_mean,
                                            double* loglik) {
  return summarize_predictions(s, true, scale, shift, num_ranks, ranks, forecast_mean, forecast_order,
                               variance_mean, pit_mean, loglik);
}

int ci_session_summarize_placebo(ci_session* s, const double* scale, const double* shift,
                                 int32_t max_origins, const int32_t* origins, const int32_t* horizon,
                                 double* predicted_mean, double* spread_mean, double* pit_mean) {
  return summarize_placebo(s, false, scale, shift, max_origins, origins, horizon, predicted_mean, spread_mean,
                           pit_mean);
}

int ci_session_summarize_placebo_blocks(ci_session* s, const double* scale, const double* shift,
                                        int32_t max_origins, const int32_t* origins, const int32_t* horizon,
                                        double* predicted_mean, double* spread_mean, double* pit_mean) {
  return summarize_placebo(s, true, scale, shift, max_origins, origins, horizon, predicted_mean, spread_mean,
                           pit_mean);
}

int ci_session_summarize_placebo_horizons(ci_session* s, const double* scale, const double* shift,
                                          int32_t max_origins, const int32_t* origins, int32_t max_horizons,
                                          const int32_t* horizons, double* predicted_mean, double* spread_mean,
                                          double* pit_mean) {
  return summarize_placebo_horizons(s, scale, shift, max_origins, origins, max_horizons, horizons, predicted_mean,
                                    spread_mean, pit_mean, 0, nullptr);
}

int ci_test_session_summarize_placebo_horizons(ci_session* s, const double* scale, const double* shift,
                                               int32_t max_origins, const int32_t* origins, int32_t max_horizons,
                                               const int32_t* horizons, double* predicted_mean,
                                               double* spread_mean, double* pit_mean, int64_t max_rows,
                                               int32_t* num_chunks) {
  return summarize_placebo_horizons(s, scale, shift, max_origins, origins, max_horizons, horizons, predicted_mean,
                                    spread_mean, pit_mean, max_rows, num_chunks);
}

int ci_session_simulate_placebo(ci_session* s, const double* scale, const double* shift, int32_t max_origins,
                                const int32_t* origins, const int32_t* horizon, int32_t link, const double* seen,
                                int32_t num_ranks, const int32_t* ranks, double* predicted_mean,
                                double* spread_mean, double* below, double* total_order, double* totals) {
  return simulate_placebo(s, false, scale, shift, max_origins, origins, horizon, link, seen, num_ranks, ranks,
                          predicted_mean, spread_mean, below, total_order, totals, 0, nullptr);
}

int ci_session_simulate_placebo_blocks(ci_session* s, const double* scale, const double* shift,
                                       int32_t max_origins, const int32_t* origins, const int32_t* horizon,
                                       int32_t link, const double* seen, int32_t num_ranks, const int32_t* ranks,
                                       double* predicted_mean, double* spread_mean, double* below,
                                       double* total_order, double* totals) {
  return simulate_placebo(s, true, scale, shift, max_origins, origins, horizon, link, seen, num_ranks, ranks,
                          predicted_mean, spread_mean, below, total_order, totals, 0, nullptr);
}

int ci_test_session_simulate_placebo(ci_session* s, int32_t blocks, const double* scale, const double* shift,
                                     int32_t max_origins, const int32_t* origins, const int32_t* horizon,
                                     int32_t link, const double* seen, int32_t num_ranks, const int32_t* ranks,
                                     double* predicted_mean, double* spread_mean, double* below,
                                     double* total_order, double* totals, int64_t max_rows, int32_t* num_chunks) {
  return simulate_placebo(s, blocks != 0, scale, shift, max_origins, origins, horizon, link, seen, num_ranks, ranks,
                          predicted_mean, spread_mean, below, total_order, totals, max_rows, num_chunks);
}

int ci_session_pool_placebo(ci_session* s, const double* scale, const double* shift,
                            int32_t num_groups, const int32_t* offsets, const int32_t* members,
                            const double* weights, int32_t max_origins, const int32_t* origins,
                            const int32_t* horizon, const double* init, double* out,
                            const double* seen, double* predicted_mean, double* spread_mean,
                            double* pit_mean) {
  return pool_placebo(s, false, scale, shift, num_groups, offsets, members, weights, max_origins, origins,
                      horizon, init, out, seen, predicted_mean, spread_mean, pit_mean, 0);
}

int ci_session_pool_placebo_blocks(ci_session* s, const double* scale, const double* shift,
                                   int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                   const double* weights, int32_t max_origins, const int32_t* origins,
                                   const int32_t* horizon, const double* init, double* out,
                                   const double* seen, double* predicted_mean, double* spread_mean,
                                   double* pit_mean) {
  return pool_placebo(s, true, scale, shift, num_groups, offsets, members, weights, max_origins, origins,
                      horizon, init, out, seen, predicted_mean, spread_mean, pit_mean, 0);
}

int ci_test_session_pool_placebo_blocks(ci_session* s, const double* scale, const double* shift,
                                        int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                        const double* weights, int32_t max_origins, const int32_t* origins,
                                        const int32_t* horizon, const double* init, double* out,
                                        const double* seen, double* predicted_mean, double* spread_mean,
                                        double* pit_mean, int32_t chunk_entries) {
  if (!s) return fail("NULL argument");
  if (chunk_entries < 1)
    return fail("chunk_entries must be in [1, %d] (the session's series), got %d", s->pb.num_series, chunk_entries);
  return pool_placebo(s, true, scale, shift, num_groups, offsets, members, weights, max_origins, origins,
                      horizon, init, out, seen, predicted_mean, spread_mean, pit_mean, chunk_entries);
}

int ci_session_pool_placebo_horizons(ci_session* s, const double* scale, const double* shift,
                                     int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                     const double* weights, int32_t max_origins, const int32_t* origins,
                                     int32_t max_horizons, const int32_t* horizons, const double* init,
                                     double* out, const double* seen, double* predicted_mean,
                                     double* spread_mean, double* pit_mean) {
  return pool_placebo_horizons(s, false, scale, shift, num_groups, offsets, members, weights, max_origins, origins,
                               max_horizons, horizons, init, out, seen, predicted_mean, spread_mean, pit_mean, 0,
                               nullptr);
}

int ci_session_pool_placebo_horizons_blocks(ci_session* s, const double* scale, const double* shift,
                                            int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                            const double* weights, int32_t max_origins, const int32_t* origins,
                                            int32_t max_horizons, const int32_t* horizons, const double* init,
                                            double* out, const double* seen, double* predicted_mean,
                                            double* spread_mean, double* pit_mean) {
  return pool_placebo_horizons(s, true, scale, shift, num_groups, offsets, members, weights, max_origins, origins,
                               max_horizons, horizons, init, out, seen, predicted_mean, spread_mean, pit_mean, 0,
                               nullptr);
}

int ci_test_session_pool_placebo_horizons(ci_session* s, int32_t blocks, const double* scale, const double* shift,
                                          int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                          const double* weights, int32_t max_origins, const int32_t* origins,
                                          int32_t max_horizons, const int32_t* horizons, const double* init,
                                          double* out, const double* seen, double* predicted_mean,
                                          double* spread_mean, double* pit_mean, int32_t chunk_entries,
                                          int32_t* num_chunks) {
  if (chunk_entries < 1) return fail("chunk_entries must be at least 1, got %d", chunk_entries);
  return pool_placebo_horizons(s, blocks != 0, scale, shift, num_groups, offsets, members, weights, max_origins,
                               origins, max_horizons, horizons, init, out, seen, predicted_mean, spread_mean,
                               pit_mean, chunk_entries, num_chunks);
}

int ci_session_pool_simulated_placebo(ci_session* s, const double* scale, const double* shift,
                                      int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                      const double* weights, int32_t max_origins, const int32_t* origins,
                                      const int32_t* horizon, int32_t link, const double* init, double* out,
                                      const double* seen, const int32_t* counted, int32_t num_ranks,
                                      const int32_t* ranks, double* predicted_mean, double* spread_mean,
                                      double* below, double* total_order) {
  return pool_simulated_placebo(s, false, scale, shift, num_groups, offsets, members, weights, max_origins,
                                origins, horizon, link, init, out, seen, counted, num_ranks, ranks,
                                predicted_mean, spread_mean, below, total_order, 0);
}

int ci_session_pool_simulated_placebo_blocks(ci_session* s, const double* scale, const double* shift,
                                             int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                             const double* weights, int32_t max_origins, const int32_t* origins,
                                             const int32_t* horizon, int32_t link, const double* init, double* out,
                                             const double* seen, const int32_t* counted, int32_t num_ranks,
                                             const int32_t* ranks, double* predicted_mean, double* spread_mean,
                                             double* below, double* total_order) {
  return pool_simulated_placebo(s, true, scale, shift, num_groups, offsets, members, weights, max_origins,
                                origins, horizon, link, init, out, seen, counted, num_ranks, ranks,
                                predicted_mean, spread_mean, below, total_order, 0);
}

int ci_test_session_pool_simulated_placebo(ci_session* s, int32_t blocks, const double* scale, const double* shift,
                                           int32_t num_groups, const int32_t* offsets, const int32_t* members,
                                           const double* weights, int32_t max_origins, const int32_t* origins,
                                           const int32_t* horizon, int32_t link, const double* init, double* out,
                                           const double* seen, const int32_t* counted, int32_t num_ranks,
                                           const int32_t* ranks, double* predicted_mean, double* spread_mean,
                                           double* below, double* total_order, int32_t chunk_entries) {
  if (!s) return fail("NULL argument");
  if (chunk_entries < 1)
    return fail("chunk_entries must be in [1, %d] (the session's series), got %d", s->pb.num_series, chunk_entries);
  return pool_simulated_placebo(s, blocks != 0, scale, shift, num_groups, offsets, members, weights, max_origins,
                                origins, horizon, link, init, out, seen, counted, num_ranks, ranks,
                                predicted_mean, spread_mean, below, total_order, chunk_entries);
}

}  // extern "C"
