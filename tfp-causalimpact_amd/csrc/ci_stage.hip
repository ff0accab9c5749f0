// ci_stage.hip -- what the sessions and the stand-alone fits check and prepare on the host
// (ci_session.h): problem validation, the routing predicates it shares with the Gibbs session,
// and the per-series parameter blocks.  No device call in this unit.
#include "ci_session.h"
#include "ci_wide.h"

bool wide_bigp_ok(const ci_problem* pb) {
  if (pb->P <= ci::MAXP || pb->T < 64) return false;
  if (pb->flags & (CI_FLAG_SEQUENTIAL_SEASONAL | CI_FLAG_CLUSTER_SEASONAL | CI_FLAG_SEASONAL_WORKSPACE |
                   CI_FLAG_MULTIWAVE_SEASONAL))
    return false;
  if (!(pb->num_blocks == 0 || (pb->num_blocks == 1 && pb->num_seasons[0] >= 2 && pb->num_seasons[0] <= 7)))
    return false;
  const int d = (pb->has_slope ? 2 : 1) + (pb->num_blocks == 1 ? pb->num_seasons[0] - 1 : 1);
  return ci::make_wlayout(pb->P, d).total <= 160 * 1024 - 512;
}
bool use_wide(const ci_problem* pb) {
  if (pb->num_blocks == 1 && pb->P > ci::MAXP) return wide_bigp_ok(pb);
  return pb->num_blocks == 1 && pb->P <= ci::MAXP && !(pb->flags & CI_FLAG_SEQUENTIAL_SEASONAL) &&
         !(pb->flags & CI_FLAG_CLUSTER_SEASONAL) && !(pb->flags & CI_FLAG_MULTIWAVE_SEASONAL) &&
         ci_wide_inst(pb->has_slope ? 2 : 1, pb->num_seasons[0]) != nullptr;
}
int wide_steps_per_thread(int T) {
  int lc = (T + ci::NT - 1) / ci::NT;
  return (lc + 3) & ~3;
}

int steps_per_thread(int T) {
  for (int L = 1; L <= 16; L *= 2)
    if (ci::NT * L >= T) return L;
  return 0;
}

int validate(const ci_problem* pb) {
  if (!pb) return fail("problem is NULL");
  if (pb->abi_version != CI_ABI_VERSION)
    return fail("ABI mismatch: caller %d, library %d", pb->abi_version, CI_ABI_VERSION);
  if (pb->T < 3) return fail("T must be >= 3, got %d", pb->T);
  if (pb->P < 0 || pb->P > ci::MAXP_BIG)
    return fail("P must be in [0, %d], got %d", ci::MAXP_BIG, pb->P);
  if (pb->num_blocks < 0 || pb->num_blocks > CI_MAX_BLOCKS)
    return fail("num_blocks must be in [0, %d], got %d", CI_MAX_BLOCKS, pb->num_blocks);
  if (pb->num_blocks > 0) {
    int dfull = pb->has_slope ? 2 : 1;
    for (int k = 0; k < pb->num_blocks; ++k) {
      if (pb->num_seasons[k] < 2) return fail("num_seasons[%d] must be >= 2", k);
      dfull += pb->num_seasons[k];
    }
    if (use_wide(pb)) {
      if (wide_steps_per_thread(pb->T) > ci::WIDE_MAX_LC)
        return fail("T=%d exceeds the time-parallel seasonal path (max %d)", pb->T, ci::NT * ci::WIDE_MAX_LC);
    } else {
      // (65-256 components: the multi-wavefront build of the sequential kernel, ci_seasonal_mw.h)
      if (dfull > ci::MW_MAXD)
        return fail("seasonal state too wide: %d > %d components (the limit of the multi-wavefront "
                    "seasonal kernel)", dfull, ci::MW_MAXD);
    }
  }
  if (pb->num_warmup < 0 || pb->num_results < 1) return fail("need num_warmup >= 0, num_results >= 1");
  if (pb->num_chains < 1 || pb->num_series < 1) return fail("need num_chains >= 1, num_series >= 1");
  if (pb->series_offset < 0 || pb->chain_offset < 0) return fail("series_offset and chain_offset must be >= 0");
  // (series ids enter the Philox key, chain ids the counter: no packing limit on either)
  if (pb->num_blocks == 0 && steps_per_thread(pb->T) == 0 &&
      wide_steps_per_thread(pb->T) > ci::WIDE_MAX_LC)
    return fail("T=%d exceeds the longest supported series (%d)", pb->T, ci::NT * ci::WIDE_MAX_LC);
  return 0;
}

int check_weights_prior_scale(const ci_series_params* params, int B) {
  for (int b = 0; b < B; ++b)
    if (!(params[b].weights_prior_scale > 0.0) || !std::isfinite(params[b].weights_prior_scale))
      return fail("params[%d].weights_prior_scale must be positive and finite (1 = the reference's "
                  "prior), got %g", b, params[b].weights_prior_scale);
  return 0;
}

int copy_name(const std::string& name, char* buf, int32_t buflen) {
  if (!buf || buflen < 1) return fail("NULL / empty name buffer");
  snprintf(buf, (size_t)buflen, "%s", name.c_str());
  return 0;
}

// Lower Cholesky factor of the prior covariance of x_0 in the (n-1)-effect coordinates:
// diag(level, [slope]) (+) sd^2 (I - 11'/n) per block   (SURVEY.md Appendix F); row-major [dr, dr].
std::vector<double> prior_chol_reduced_d(const ci_problem* pb, const ci_series_params& q, int dr,
                                         bool inert_blocks) {
  const int K = pb->num_blocks;
  std::vector<double> A((size_t)dr * dr, 0.0);
  A[0] = q.init_level_scale * q.init_level_scale;
  int o = 1;
  if (pb->has_slope) { A[(size_t)1 * dr + 1] = q.init_slope_scale * q.init_slope_scale; o = 2; }
  for (int k = 0; k < K; ++k) {
    const int n = pb->num_seasons[k];
    const double v = inert_blocks ? 0.0 : q.init_seasonal_scale * q.init_seasonal_scale;
    for (int i = 0; i < n - 1; ++i)
      for (int j = 0; j < n - 1; ++j)
        A[(size_t)(o + i) * dr + o + j] = v * ((i == j ? 1.0 : 0.0) - 1.0 / n);
    o += n - 1;
  }
  for (int j = 0; j < dr; ++j) {
    double sdiag = A[(size_t)j * dr + j];
    for (int k2 = 0; k2 < j; ++k2) sdiag -= A[(size_t)j * dr + k2] * A[(size_t)j * dr + k2];
    const double ljj = sdiag > 0.0 ? std::sqrt(sdiag) : 0.0;
    A[(size_t)j * dr + j] = ljj;
    for (int i = j + 1; i < dr; ++i) {
      double t2 = A[(size_t)i * dr + j];
      for (int k2 = 0; k2 < j; ++k2) t2 -= A[(size_t)i * dr + k2] * A[(size_t)j * dr + k2];
      A[(size_t)i * dr + j] = ljj > 0.0 ? t2 / ljj : 0.0;
    }
    for (int i = 0; i < j; ++i) A[(size_t)i * dr + j] = 0.0;
  }
  return A;
}
std::vector<float> prior_chol_reduced(const ci_problem* pb, const ci_series_params& q, int dr,
                                      bool inert_blocks) {
  const std::vector<double> A = prior_chol_reduced_d(pb, q, dr, inert_blocks);
  std::vector<float> out(A.size());
  for (size_t e = 0; e < A.size(); ++e) out[e] = (float)A[e];
  return out;
}

ci::DevSeriesParams dev_series_params(const ci_series_params& q, double n_obs) {
  ci::DevSeriesParams d;
  d.level_conc = q.level_conc; d.level_scale = q.level_scale; d.level_ub = q.level_ub;
  d.slope_conc = q.slope_conc; d.slope_scale = q.slope_scale; d.slope_ub = q.slope_ub;
  d.obs_conc = q.obs_conc; d.obs_scale = q.obs_scale; d.obs_ub = q.obs_ub;
  d.nonzero_prob = q.nonzero_prob;
  d.init_level_loc = q.init_level_loc; d.init_level_scale = q.init_level_scale;
  d.init_slope_scale = q.init_slope_scale;
  d.obs_scale0 = q.obs_scale0; d.level_scale0 = q.level_scale0; d.slope_scale0 = q.slope_scale0;
  d.n_obs = n_obs;
  return d;
}

ci::DevSeasonalParams dev_seasonal_params(const ci_series_params& q, bool inert) {
  ci::DevSeasonalParams d;
  d.drift_conc = inert ? 1.0 : q.drift_conc;
  d.drift_scale = inert ? 1.0 : q.drift_scale;
  d.drift_ub = inert ? 1.0 : q.drift_ub;
  d.init_seasonal_scale = inert ? 0.0 : q.init_seasonal_scale;
  for (int k = 0; k < CI_MAX_BLOCKS; ++k) d.drift_scale0[k] = inert ? 0.0 : q.drift_scale0[k];
  return d;
}
