// ci_predict.h -- one-step-ahead prediction errors of every fit of a finished session: for every
// series b and pooled draw n (chain-major, n = c*S + s) the Kalman filter of that draw's model over
// the observed series, in float64 (ci_session_summarize_predictions; DESIGN.md "Prediction errors").
//
// One lane per (series, draw), sequential over time.  A wavefront holds 64 consecutive draws of one
// series: every load and store over the draw axis is coalesced, everything that depends on the step
// alone (y, mask, season change) is uniform over the wavefront.  The kernel is templated on the
// state's shape -- HAS_SLOPE in {0, 1}, NS in {0, 2..7}: d = 1 + HAS_SLOPE + (NS - 1) <= 8 -- so the
// state mean a[d] and the upper triangle of the symmetric covariance P (<= 36 entries) are fully
// unrolled register arrays; no array is indexed at run time (that would go to scratch).
//
// The model of series b, draw n (the state space of oracle/ci_oracle.c):
//   sigma_obs, sigma_level, sigma_slope, sigma_drift: the session's draws widened to double, once, where
//     they are loaded -- float32 (IN = float: a fit's session, or one made from float32 draws) or float64
//     (IN = double: ci_session_create_from_draws_f64); y likewise; everything downstream is float64;
//     H = sigma_obs^2, Q_level = sigma_level^2, Q_slope = sigma_slope^2, q = (sigma_drift / NS)^2
//   a_0 = (init_level_loc, 0, ..), P_0 = diag(init_level_scale^2, init_slope_scale^2) and, in the
//     NS - 1 effect coordinates, init_seasonal_scale^2 (I - 1/NS)        (init [B, 4] holds them)
//   transition t -> t + 1: level += slope; at a step whose season_change flag is set the block's
//     companion rotation x' = (x_1, .., x_{NS-2}, -sum x), with q added to every entry of the block
//   Z picks component 0 and the first effect of the block
//   reg[n, t] = sum over j ascending from 0.0 of double(X[t, j]) * double(w[n, j]):
//     comp_regression_kernel with scale 1, read from the [T, N] matrix `reg` (nullptr: no design)
// and for t = 0 .. T_b - 1 (T_b: the series' own length in a ragged session):
//   m = Z a;  F = Z P Z' + H;  f = m + reg[n, t]
//   forecast[n, t] = f * scale[b] + shift[b]       (two roundings)
//   variance[n, t] = (F * scale[b]) * scale[b]
//   not masked:  v = double(y[t]) - f;  pit[n, t] = 0.5 erfc(-v / sqrt(2 F));
//                ll[n] += -0.5 (log 2 pi + log F + v^2 / F);  a += (P Z' / F) v;  P -= (P Z')(P Z')' / F
//   masked:      pit[n, t] = 0
//   t + 1 < T_b: a <- T_t a;  P <- T_t P T_t' + Q_t
// Beyond T_b (padding) f = 0: the forecast reads shift[b], variance and pit 0.
//
// Layout of the results: the filter runs ONCE PER REQUESTED MATRIX, selected by the template
// argument OUT; it writes that [T, N] matrix (time-major, draws contiguous: what the select and
// row-statistics kernels read) and nothing else but, when `ll` is given, the per-draw
// log-likelihood.  The regression matrix is only read and serves every pass.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ci {

enum PredOut { PRED_FORECAST = 0, PRED_VARIANCE = 1, PRED_PIT = 2 };

struct PredArgs {
  int N, T;                        // pooled draws; steps (the row stride of a ragged session)
  const void* y;                   // [B, T] of IN, the input type (float or double) the kernel is built for
  const uint8_t* mask;             // [B, T]
  const uint8_t* season_change;    // [T] (NS > 0)
  const int* series_T;             // [B] or nullptr
  const void *obs, *lscale, *sscale, *drift;   // [B, N] of IN
  const double* init;              // [B, 4]: level loc, level var, slope var, seasonal var
  const double *scales, *shifts;   // [B]
  const double* reg;               // [B, T, N] or nullptr
  double* out;                     // [B, T, N]
  double* ll;                      // [B, N] or nullptr
};

// The launch (ci_predict.hip): predict_kernel<has_slope, num_seasons, out> over B series.  The filter
// units are built twice: as they stand for F = float, the inputs of a fit's session, and with
// -DCI_FILTER_F64 for F = double, the inputs of a float64 session made from draws
// (ci_session_create_from_draws_f64); the launches of that build carry the suffix _f64.
hipError_t predict_launch(hipStream_t stream, int B, int has_slope, int num_seasons, int out,
                          const PredArgs& args);
hipError_t predict_launch_f64(hipStream_t stream, int B, int has_slope, int num_seasons, int out,
                              const PredArgs& args);
#ifdef CI_FILTER_F64
#define CI_FILTER_F double
#define CI_FILTER_NAME(name) name##_f64
#else
#define CI_FILTER_F float
#define CI_FILTER_NAME(name) name
#endif

// Position of (i, j) in the row-major upper triangle of a symmetric D x D matrix.
template <int D> __host__ __device__ constexpr int pred_sym(int i, int j) {
  return i <= j ? i * D - i * (i - 1) / 2 + (j - i) : j * D - j * (j - 1) / 2 + (i - j);
}

// The block's companion rotation x' = (x_1, .., x_{N1-1}, -sum x) of the N1 effects at offset O on a
// vector that transforms like the state mean (the mean itself; the covariance of the state with a
// running sum, ci_placebo.h).  The sum runs ascending from 0.0.
template <int O, int N1, int D>
__device__ __forceinline__ void pred_season_rotate(double (&a)[D]) {
  constexpr int L = N1 - 1;                  // the block's last effect
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < N1; ++i) s += a[O + i];
#pragma unroll
  for (int i = 0; i < L; ++i) a[O + i] = a[O + i + 1];
  a[O + L] = -s;
}

// The block's step at a season change, on the mean and the upper triangle of the covariance: the
// companion rotation x' = (x_1, .., x_{N1-1}, -sum x) of the N1 effects at offset O, then q on every
// entry of the block.  Sums run ascending from 0.0.
template <int O, int N1, int D>
__device__ __forceinline__ void pred_season_step(double (&a)[D], double (&P)[D * (D + 1) / 2], double q_drift) {
#define PM(i, j) P[pred_sym<D>(i, j)]
  constexpr int L = N1 - 1;                  // the block's last effect
  pred_season_rotate<O, N1, D>(a);
#pragma unroll
  for (int c = 0; c < O; ++c) {              // the trend's rows of the block's columns
    double sc = 0.0;
#pragma unroll
    for (int i = 0; i < N1; ++i) sc += PM(c, O + i);
#pragma unroll
    for (int i = 0; i < L; ++i) PM(c, O + i) = PM(c, O + i + 1);
    PM(c, O + L) = -sc;
  }
  double rs[N1], tot = 0.0;                  // row sums of the block and their sum
#pragma unroll
  for (int i = 0; i < N1; ++i) {
    double r = 0.0;
#pragma unroll
    for (int j = 0; j < N1; ++j) r += PM(O + i, O + j);
    rs[i] = r;
  }
#pragma unroll
  for (int i = 0; i < N1; ++i) tot += rs[i];
#pragma unroll
  for (int i = 0; i < L; ++i)
#pragma unroll
    for (int j = i; j < L; ++j) PM(O + i, O + j) = PM(O + i + 1, O + j + 1);
#pragma unroll
  for (int i = 0; i < L; ++i) PM(O + i, O + L) = -rs[i + 1];
  PM(O + L, O + L) = tot;
#pragma unroll
  for (int i = 0; i < N1; ++i)
#pragma unroll
    for (int j = i; j < N1; ++j) PM(O + i, O + j) += q_drift;
#undef PM
}

// grid (ceil(N / 64), B), block 64.
template <int HAS_SLOPE, int NS, int OUT, class IN = float>
__global__ __launch_bounds__(64) void predict_kernel(PredArgs k) {
  constexpr int N1 = NS ? NS - 1 : 0, O = 1 + HAS_SLOPE, D = O + N1, NP = D * (D + 1) / 2;
  constexpr double LOG_2PI = 1.8378770664093454835606594728112;
  const int n = blockIdx.x * 64 + threadIdx.x, N = k.N, T = k.T;
  const size_t b = blockIdx.y;
  if (n >= N) return;
  const int Tb = k.series_T ? k.series_T[b] : T;
  const size_t bn = b * N + n;
  const double so = (double)((const IN*)k.obs)[bn], H = so * so;
  const double sl = (double)((const IN*)k.lscale)[bn], q_level = sl * sl;
  double q_slope = 0.0, q_drift = 0.0;
  if (HAS_SLOPE) {
    const double ss = (double)((const IN*)k.sscale)[bn];
    q_slope = ss * ss;
  }
  if (NS) {
    const double q = (double)((const IN*)k.drift)[bn] / (double)NS;
    q_drift = q * q;
  }
  const double scale = k.scales[b], shift = k.shifts[b];
  const double* init = k.init + 4 * b;
  const IN* y = (const IN*)k.y + b * T;
  const uint8_t* mask = k.mask + b * T;
  const double* reg = k.reg ? k.reg + b * T * N + n : nullptr;
  double* out = k.out + b * T * N + n;

  double a[D], P[NP];
#define PM(i, j) P[pred_sym<D>(i, j)]
#pragma unroll
  for (int i = 0; i < D; ++i) a[i] = 0.0;
#pragma unroll
  for (int i = 0; i < NP; ++i) P[i] = 0.0;
  a[0] = init[0];
  PM(0, 0) = init[1];
  if (HAS_SLOPE) PM(1, 1) = init[2];
  if (NS) {
    const double v = init[3];
#pragma unroll
    for (int i = 0; i < N1; ++i)
#pragma unroll
      for (int j = i; j < N1; ++j) PM(O + i, O + j) = v * ((i == j ? 1.0 : 0.0) - 1.0 / (double)NS);
  }

  double ll = 0.0;
  for (int t = 0; t < Tb; ++t) {
    double pz[D];
#pragma unroll
    for (int i = 0; i < D; ++i) pz[i] = NS ? PM(i, 0) + PM(i, O < D ? O : 0) : PM(i, 0);
    const double m = NS ? a[0] + a[O < D ? O : 0] : a[0];
    const double F = (NS ? pz[0] + pz[O < D ? O : 0] : pz[0]) + H;
    const double f = m + (reg ? reg[(size_t)t * N] : 0.0);
    const bool seen = mask[t] == 0;              // uniform over the wavefront
    const double v = seen ? (double)y[t] - f : 0.0;
    double res;
    if (OUT == PRED_FORECAST) res = __dadd_rn(__dmul_rn(f, scale), shift);
    else if (OUT == PRED_VARIANCE) res = __dmul_rn(__dmul_rn(F, scale), scale);
    else res = seen ? 0.5 * erfc(-v / sqrt(2.0 * F)) : 0.0;
    out[(size_t)t * N] = res;
    if (seen) {
      if (k.ll) ll += -0.5 * (LOG_2PI + log(F) + v * v / F);
#pragma unroll
      for (int i = 0; i < D; ++i) a[i] += (pz[i] / F) * v;
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = i; j < D; ++j) PM(i, j) -= pz[i] * pz[j] / F;
    }
    if (t + 1 >= Tb) break;
    // a <- T a, P <- T P T' + Q: the trend's part, then the block's (they act on disjoint components)
    if (HAS_SLOPE) {
      a[0] += a[1];
      const double p01 = PM(0, 1) + PM(1, 1);
      PM(0, 0) = (PM(0, 0) + PM(0, 1)) + p01;
      PM(0, 1) = p01;
#pragma unroll
      for (int j = 2; j < D; ++j) PM(0, j) += PM(1, j);
    }
    if constexpr (NS > 0) {
      if (k.season_change[t]) pred_season_step<O, N1, D>(a, P, q_drift);   // uniform over the grid
    }
    PM(0, 0) += q_level;
    if (HAS_SLOPE) PM(1, 1) += q_slope;
  }
#undef PM
  const double pad = OUT == PRED_FORECAST ? __dadd_rn(__dmul_rn(0.0, scale), shift) : 0.0;
  for (int t = Tb; t < T; ++t) out[(size_t)t * N] = pad;
  if (k.ll) k.ll[bn] = ll;
}

}  // namespace ci
