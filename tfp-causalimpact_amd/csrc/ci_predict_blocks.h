// ci_predict_blocks.h -- the prediction-error filter of ci_predict.h for ANY block list with a state
// of at most 64 components, cooperative over lanes (ci_session_summarize_predictions_blocks;
// DESIGN.md "Block-model filters").
//
// THE MODEL is that of ci_predict.h, generalised to K blocks.  Let hs = has_slope.
//   Block k has n_k seasons and n_k - 1 effect coordinates at offset o_k = 1 + hs + sum_{j<k} (n_j - 1);
//   d = 1 + hs + sum_k (n_k - 1) <= 64.  Z has ones at 0 and at every o_k.
//   sigma_obs, sigma_level, sigma_slope as there; sigma_drift: the session's draws [B, N, K], of the
//   input type IN (float or double, as there) widened to double; season_change [K, T].  a_0 = (init_level_loc, 0, ..), P_0 = diag(init_level_scale^2,
//   init_slope_scale^2) and init_seasonal_scale^2 (I - 1/n_k) in every block, zero across blocks.
// Per step t = 0 .. T - 1:
//   m = a[0] + a[o_0] + a[o_1] + ..        (added in that order)
//   pz_i = P[i, 0] + P[i, o_0] + ..        (the same order);   F = (pz[0] + pz[o_0] + ..) + H
//   f = m + reg[n, t];  forecast, variance, pit, ll, the masked branch and the two-rounding maps to
//   the data scale: lines 22-30 of ci_predict.h, expression by expression
//   not masked:  a_i += (pz_i / F) v;   P_ij -= pz_i pz_j / F
// Transition t -> t + 1, t + 1 < T:
//   the trend's part as in predict_kernel (level += slope);
//   then, k ascending, every block whose season_change[k, t] is set takes the companion rotation of
//   pred_season_step -- x' = (x_1, .., x_{n_k - 2}, -sum x) -- on its own rows and columns AND on its
//   cross-covariances with every component outside it (the trend's rows and the other blocks' rows),
//   sums ascending from 0.0, then q_k = (sigma_drift_k / n_k)^2 on every entry of block k;
//   last q_level on P[0, 0] and q_slope on P[1, 1].
//
// LAYOUT.  A group of G lanes runs one filter, G the smallest of 8, 16, 32, 64 that is >= d (the
// template argument); a wavefront (one workgroup) holds 64 / G filters of consecutive draws of one
// series.  Lane i of the group owns a_i and ROW i of P as the register array P[G], indexed by
// unrolled loops only: the block offsets, sizes and change flags are run-time values, uniform over
// the grid, kept in LDS and in 64-bit masks (Z, a block's columns) whose bit j is tested against the
// unrolled index j; they never index registers.
// Rows and columns from d on stay zero.  The FULL matrix is stored, both triangles: P[i][j] and
// P[j][i] are produced by mirrored expressions whose operands are bitwise equal (a product commutes,
// the sums below run over the same values in the same order), so the matrix stays bitwise symmetric
// and an entry has one value however it is reached:
//   update     lane i, column j: P[i][j] - pz_i * pz_j / F, pz_j read from LDS
//   trend      row 0 += row 1 (lane 0 reads P[j][1] = P[1][j] of lane j from LDS), then in every
//              lane column 0 += column 1: P[0][0] = (P00 + P01) + (P01 + P11) as predict_kernel
//   rotation   columns first, in every lane: s_i = sum of row i over the block's columns, the block's
//              columns move down by one, the last becomes -s_i; then rows: the block's lanes take the
//              row of the lane above them (__shfl_down), the block's last lane builds its row from
//              the s of all lanes (LDS): -s_c outside the block, -s_{c+1} inside it, and sum_i s_i
//              (ascending from 0.0) on the diagonal -- what the mirrored sums over rows would give.
// Cross-lane traffic is three 64-double LDS vectors per wavefront (a, pz or s, and the placebo's r)
// and the row shift.  Nothing of one filter's arithmetic depends on what shares its wavefront, on N,
// B, the grid or the output requested; lanes of a group beyond N repeat draw N - 1 and store nothing.
//
// Results as ci_predict.h: one pass per requested matrix (OUT), [T, N] per series, the group's lane 0
// stores -- consecutive draws of a wavefront's filters are neighbours.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ci_predict.h"

namespace ci {

constexpr int PB_MAX_BLOCKS = 8;   // == CI_MAX_BLOCKS
constexpr int PB_MAX_STATE = 64;

struct BlockModel {                // uniform over the grid
  int has_slope, K, d;
  int off[PB_MAX_BLOCKS];          // o_k
  int ns[PB_MAX_BLOCKS];           // n_k
  unsigned long long zmask;        // bit 0 and the bits o_k: Z
};

struct PredBlocksArgs {
  PredArgs p;                      // season_change [K, T], drift [B, N, K]; series_T unused (not ragged)
  BlockModel m;
};

// The launch (ci_predict_blocks.hip): predict_blocks_kernel<G, out> over B series, G from m.d.
hipError_t predict_blocks_launch(hipStream_t stream, int B, int out, const PredBlocksArgs& args);
hipError_t predict_blocks_launch_f64(hipStream_t stream, int B, int out, const PredBlocksArgs& args);

// What a group's lanes share: the model in LDS, the exchange vectors, the lane's place.
struct PbCtx {
  int lane, i, gb, g;              // lane of the wavefront, row, the group's first lane, group
  int hs, K, T;
  unsigned long long zmask;
  const uint8_t* season_change;    // [K, T]
  const int *off, *n1;             // LDS [K]: o_k, n_k - 1
  const double* q;                 // LDS [K] of this group: q_k
  double *xa, *xb, *xc;            // LDS [64]
  double q_level, q_slope;
};

// sum over Z of a vector lying in LDS at the group's base: x[0] + x[o_0] + x[o_1] + ..
__device__ __forceinline__ double pb_zsum(const PbCtx& c, const double* x) {
  double m = x[c.gb];
  for (int k = 0; k < c.K; ++k) m += x[c.gb + c.off[k]];
  return m;
}

// pz_i of the lane's row: P[i][0] + P[i][o_0] + ..
template <int G> __device__ __forceinline__ double pb_pz(const PbCtx& c, const double (&P)[G]) {
  double pz = P[0];
#pragma unroll
  for (int j = 1; j < G; ++j)
    if ((c.zmask >> j) & 1ull) pz += P[j];
  return pz;
}

// a += (pz / F) v, P -= pz pz' / F; xb holds the group's pz.
template <int G>
__device__ __forceinline__ void pb_update(const PbCtx& c, double& a, double (&P)[G], double pz, double F, double v) {
  a += (pz / F) * v;
#pragma unroll
  for (int j = 0; j < G; ++j) P[j] -= pz * c.xb[c.gb + j] / F;
}

// The companion rotation of block k on a vector that transforms like the mean, lying in LDS (x):
// the lane's new component.
__device__ __forceinline__ double pb_rotate_mean(const PbCtx& c, const double* x, double mine, int o, int last) {
  double s = 0.0;
  for (int j = o; j <= last; ++j) s += x[c.gb + j];
  if (c.i >= o && c.i < last) return x[c.lane + 1];
  if (c.i == last) return -s;
  return mine;
}

// a <- T a, [r <- T r,] P <- T P T' + Q of step t -> t + 1.
template <int G, bool WITH_R>
__device__ __forceinline__ void pb_transition(const PbCtx& c, int t, double& a, double& r, double (&P)[G]) {
  if (c.hs) {
    __syncthreads();
    c.xa[c.lane] = a;
    c.xb[c.lane] = P[1];
    if (WITH_R) c.xc[c.lane] = r;
    __syncthreads();
    if (c.i == 0) {
      a += c.xa[c.gb + 1];
      if (WITH_R) r += c.xc[c.gb + 1];
#pragma unroll
      for (int j = 0; j < G; ++j) P[j] += c.xb[c.gb + j];
    }
    P[0] += P[1];
  }
  for (int k = 0; k < c.K; ++k) {
    if (!c.season_change[(size_t)k * c.T + t]) continue;      // uniform over the grid
    const int o = c.off[k], last = o + c.n1[k] - 1;
    // the block's columns, its columns but the last, its last column: bit j of a uniform mask each,
    // tested against the unrolled index
    const unsigned long long in_last = 1ull << last;
    const unsigned long long in_block = (in_last | (in_last - 1ull)) & ~((1ull << o) - 1ull);
    const unsigned long long in_head = in_block & ~in_last;
    // columns: s = the row's sum over the block, the block's columns move down, the last is -s
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < G; ++j)
      if ((in_block >> j) & 1ull) s += P[j];
#pragma unroll
    for (int j = 0; j + 1 < G; ++j)
      if ((in_head >> j) & 1ull) P[j] = P[j + 1];
#pragma unroll
    for (int j = 0; j < G; ++j)
      if ((in_last >> j) & 1ull) P[j] = -s;
    __syncthreads();
    c.xa[c.lane] = a;
    c.xb[c.lane] = s;
    if (WITH_R) c.xc[c.lane] = r;
    __syncthreads();
    // rows: the block's lanes but the last take the row above them
    const bool up = c.i >= o && c.i < last;
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const double above = __shfl_down(P[j], 1, G);
      if (up) P[j] = above;
    }
    a = pb_rotate_mean(c, c.xa, a, o, last);
    if (WITH_R) r = pb_rotate_mean(c, c.xc, r, o, last);
    double tot = 0.0;
    for (int j = o; j <= last; ++j) tot += c.xb[c.gb + j];
    if (c.i == last) {
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const int src = j + (int)((in_head >> j) & 1ull);
        const double sj = c.xb[c.gb + src];
        P[j] = ((in_last >> j) & 1ull) ? tot : -sj;
      }
    }
    if (c.i >= o && c.i <= last) {
      const double qk = c.q[k];
#pragma unroll
      for (int j = 0; j < G; ++j)
        if ((in_block >> j) & 1ull) P[j] += qk;
    }
  }
  if (c.i == 0) P[0] += c.q_level;
  if (c.hs && c.i == 1) P[1] += c.q_slope;
}

// The LDS of one wavefront's filters.
struct PbShared {
  double xa[64], xb[64], xc[64];
  double q[8][PB_MAX_BLOCKS];      // [group][k]
  int off[PB_MAX_BLOCKS], n1[PB_MAX_BLOCKS];
};

// Sets the context up, loads the draw's scales and the initial moments (a, P) of the lane's row.
// n: the group's draw (clamped to N - 1), bn = b * N + n.
template <int G, class IN>
__device__ __forceinline__ void pb_begin(const PredArgs& p, const BlockModel& m, PbShared& sh, size_t b, size_t bn,
                                         PbCtx& c, double& H, double& a, double (&P)[G]) {
  c.lane = threadIdx.x; c.i = c.lane % G; c.g = c.lane / G; c.gb = c.g * G;
  c.hs = m.has_slope; c.K = m.K; c.T = p.T; c.zmask = m.zmask;
  c.season_change = p.season_change;
  c.off = sh.off; c.n1 = sh.n1; c.q = sh.q[c.g];
  c.xa = sh.xa; c.xb = sh.xb; c.xc = sh.xc;
#pragma unroll
  for (int kk = 0; kk < PB_MAX_BLOCKS; ++kk)     // (unrolled: the argument arrays are not indexed at run time)
    if (c.lane == kk) {
      sh.off[kk] = kk < m.K ? m.off[kk] : 0;
      sh.n1[kk] = kk < m.K ? m.ns[kk] - 1 : 0;
    }
  __syncthreads();
  if (c.i < m.K) {
    const double q = (double)((const IN*)p.drift)[bn * m.K + c.i] / (double)(sh.n1[c.i] + 1);
    sh.q[c.g][c.i] = q * q;
  }
  const double so = (double)((const IN*)p.obs)[bn];
  H = so * so;
  const double sl = (double)((const IN*)p.lscale)[bn];
  c.q_level = sl * sl;
  c.q_slope = 0.0;
  if (m.has_slope) {
    const double ss = (double)((const IN*)p.sscale)[bn];
    c.q_slope = ss * ss;
  }
  __syncthreads();
  const double* init = p.init + 4 * b;
  a = c.i == 0 ? init[0] : 0.0;
#pragma unroll
  for (int j = 0; j < G; ++j) P[j] = 0.0;
  if (c.i == 0) P[0] = init[1];
  if (m.has_slope && c.i == 1) P[1] = init[2];
  const double v = init[3];
  for (int k = 0; k < m.K; ++k) {
    const int o = sh.off[k], last = o + sh.n1[k] - 1;
    if (c.i < o || c.i > last) continue;
    const double inv = 1.0 / (double)(sh.n1[k] + 1);
#pragma unroll
    for (int j = 0; j < G; ++j)
      if (j >= o && j <= last) P[j] = v * ((c.i == j ? 1.0 : 0.0) - inv);
  }
}

// The filter's moments of a step: pz of the lane's row, and through LDS m = Z a, zpz = Z pz
// (xb keeps the group's pz for pb_update).
template <int G>
__device__ __forceinline__ void pb_moments(const PbCtx& c, double a, const double (&P)[G], double& pz, double& m,
                                           double& zpz) {
  pz = pb_pz<G>(c, P);
  __syncthreads();
  c.xa[c.lane] = a;
  c.xb[c.lane] = pz;
  __syncthreads();
  m = pb_zsum(c, c.xa);
  zpz = pb_zsum(c, c.xb);
}

// grid (ceil(N / (64 / G)), B), block 64.
template <int G, int OUT, class IN = float>
__global__ __launch_bounds__(64) void predict_blocks_kernel(PredBlocksArgs k) {
  constexpr double LOG_2PI = 1.8378770664093454835606594728112;
  constexpr int FPW = 64 / G;
  __shared__ PbShared sh;
  const int N = k.p.N, T = k.p.T;
  const int n_own = blockIdx.x * FPW + (int)threadIdx.x / G;
  const bool active = n_own < N;
  const int n = active ? n_own : N - 1;
  const size_t b = blockIdx.y, bn = b * N + n;
  PbCtx c;
  double H, a, P[G];
  pb_begin<G, IN>(k.p, k.m, sh, b, bn, c, H, a, P);
  const bool writer = active && c.i == 0;
  const double scale = k.p.scales[b], shift = k.p.shifts[b];
  const IN* y = (const IN*)k.p.y + b * T;
  const uint8_t* mask = k.p.mask + b * T;
  const double* reg = k.p.reg ? k.p.reg + b * T * N + n : nullptr;
  double* out = k.p.out + b * T * N + n;

  double ll = 0.0, unused = 0.0;
  for (int t = 0; t < T; ++t) {
    double pz, m, zpz;
    pb_moments<G>(c, a, P, pz, m, zpz);
    const double F = zpz + H;
    const double f = m + (reg ? reg[(size_t)t * N] : 0.0);
    const bool seen = mask[t] == 0;              // uniform over the wavefront
    const double v = seen ? (double)y[t] - f : 0.0;
    double res;
    if (OUT == PRED_FORECAST) res = __dadd_rn(__dmul_rn(f, scale), shift);
    else if (OUT == PRED_VARIANCE) res = __dmul_rn(__dmul_rn(F, scale), scale);
    else res = seen ? 0.5 * erfc(-v / sqrt(2.0 * F)) : 0.0;
    if (writer) out[(size_t)t * N] = res;
    if (seen) {
      if (k.p.ll) ll += -0.5 * (LOG_2PI + log(F) + v * v / F);
      pb_update<G>(c, a, P, pz, F, v);
    }
    if (t + 1 >= T) break;
    pb_transition<G, false>(c, t, a, unused, P);
  }
  if (writer && k.p.ll) k.p.ll[bn] = ll;
}

}  // namespace ci
