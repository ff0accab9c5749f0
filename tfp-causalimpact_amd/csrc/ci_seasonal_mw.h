// ci_seasonal_mw.h -- the multi-wavefront build of the sequential seasonal Gibbs kernel
// (gibbs_seasonal_kernel<GWS, BIGP, MW_NWV> of ci_seasonal.h): states of 65-256 components, such
// as an hour-of-week block Seasons(168) on hourly data.
//
// Same model form, same smoother, same random numbers as the one-wavefront build: slot
// coordinates, the observation row e_0 + sum_k e_{off[k]+c_k(t)}, rank-1 drift noise
// sigma eta (e_slot - 1/n), de Jong / Koopman fast smoothing.  Thread i (of MW_NWV wavefronts) owns
// component i of every state-sized vector and ROW i of the covariance.  What changes:
//   * the covariance lives in LDS as a packed COLUMN-MAJOR lower triangle (tri() below: D (D + 1) / 2
//     floats, 131.6 KB at D = 256): thread i walks its row j = 0..i, and at any j the threads of a
//     wavefront touch consecutive words -- conflict-free, no register array indexed at run time;
//   * the step's cross-component sums (F, Z a, K'r) go through LDS and workgroup barriers: the
//     1 + K observed components publish P z and a, everyone reads them back (two barriers per
//     filter step), the backward pass reduces per wavefront and then over MW_NWV partials;
//   * wavefront 0 alone runs what the one-wave kernel runs outside the four passes (regression
//     block, scale draws, emission, random normals) through the very same code; the others wait.
// The arrays over time stay where the one-wave kernel keeps them (LDS or the HBM workspace).
// With D <= 64 (CI_FLAG_MULTIWAVE_SEASONAL) the sums are those of the one-wave kernel up to float
// summation order, and every random number is the same.
#pragma once
#include "ci_kernels.h"

namespace ci {

// float offsets in the multi-wave step area (SLayout::pzv, MW_LDS_FLOATS floats)
constexpr int MW_PZ = 0;                 // [MW_MAXD] P z of the step; after pass 3 the drift statistics
constexpr int MW_OZ = MW_MAXD;           // [1 + SMAXK] P z of the observed components (level, blocks)
constexpr int MW_OA = MW_MAXD + 16;      // [1 + SMAXK] filtered mean of the observed components
constexpr int MW_RED = MW_MAXD + 32;     // [2][8] per-wavefront partial sums, by step parity
constexpr int MW_SC = MW_MAXD + 48;      // [8] scale draws of the iteration: sigma_obs, level, slope
constexpr int MW_DSD = MW_MAXD + 56;     // [SMAXK] drift scale of each block
constexpr int MW_DST = MW_MAXD + 64;     // [SMAXK] drift statistic of each block
constexpr int MW_ZC = MW_MAXD + 72;      // [SMAXK] int: observed column of each block
static_assert(MW_ZC + SMAXK <= MW_LDS_FLOATS, "multi-wave step area");

// packed column-major lower triangle: column j holds rows j..D-1
__device__ __forceinline__ int mw_tri(int i, int j, int D) { return j * D - ((j * (j - 1)) >> 1) + (i - j); }
__device__ __forceinline__ int mw_sym(int i, int j, int D) { return i >= j ? mw_tri(i, j, D) : mw_tri(j, i, D); }

// Pass 1 (Kalman filter in slot coordinates, storing K_t and v_t / F_t), one workgroup of NWV
// wavefronts.  Per step: P z of the own row from the 1 + K observed columns; the observed
// components publish (P z)_c and a_c; F and v from those; then the own row of
//   P' = T (P - (P z)(P z)' / F) T' + Q_t,   Q_t = diag(ql, qs) + sigma_k^2 g g' (changing blocks)
// in place.
template <bool GWS, int NWV>
__device__ __forceinline__ void seasonal_filter_pass_mw(const SeasFilterArgs& p, int K) {
  const int T = p.T, D = p.D, tid = p.lane, blk = p.blk, pos = p.pos, nb = p.nb, boff = p.boff;
  const bool slope = p.has_slope != 0;
  const bool comp = tid < D;
  const float H = p.H, ql = p.ql, qs = p.qs, myd2 = p.myd2, rnb = p.rnb;
  CI_LDS float* Pm = (CI_LDS float*)p.Pm;
  CI_LDS float* mw = (CI_LDS float*)p.pzv;
  CI_LDS float* pzv = mw + MW_PZ;
  CI_LDS float* oz = mw + MW_OZ;
  CI_LDS float* oa = mw + MW_OA;
  CI_LDS int* zc = (CI_LDS int*)(mw + MW_ZC);
  using TF = typename std::conditional<GWS, CI_GLB float, CI_LDS float>::type;
  using TB = typename std::conditional<GWS, CI_GLB const uint8_t, CI_LDS const uint8_t>::type;
  using TF4 = typename std::conditional<GWS, CI_GLB ci_f4v, CI_LDS ci_f4v>::type;
  using TU = typename std::conditional<GWS, CI_GLB const uint32_t, CI_LDS const uint32_t>::type;
  TF* kfw = (TF*)p.kf + tid;
  TF* vfp = (TF*)p.vf;
  TF* ytil = (TF*)p.ytil;
  TB* cbv = (TB*)p.cbv;
  TB* msk = (TB*)p.msk;
  TB* cidb = (TB*)p.cidb;
  auto at4 = [](const ci_f4v& v, int q) { return q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w; };
  if (blk >= 0 && pos == 0) zc[blk] = p.boff;
  __syncthreads();
  float am = p.a1e;
  const int rbase = comp ? mw_tri(tid, 0, D) : 0;   // = tid: the row's first entry
  for (int t4 = 0; t4 < T; t4 += 4) {
    const ci_f4v yt4 = *(TF4*)(ytil + t4);
    const uint32_t cb4 = *(TU*)(cbv + t4), mk4 = *(TU*)(msk + t4), cw4 = *(TU*)(cidb + t4);
    float vfq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int t = t4 + q;
      vfq[q] = 0.f;
      if (t >= T) continue;
      const bool obs = ((mk4 >> (8 * q)) & 0xFFu) == 0u;
      const bool last = t + 1 == T;
      const unsigned cb = last ? 0u : ((cb4 >> (8 * q)) & 0xFFu);
      const int mycur = (int)((cw4 >> (8 * q)) & 0xFFu);
      const bool mych = blk >= 0 && ((cb >> blk) & 1u) != 0u;
      // a full time update (else at most level += ql, which touches thread 0's own entry only)
      const bool upd = !last && (obs || cb != 0u || slope);
      float pz = 0.f, p10 = 0.f, p11 = 0.f;
      if (obs && comp) {
        pz = Pm[rbase];
        for (int k = 0; k < K; ++k) pz += Pm[mw_sym(tid, zc[k], D)];
        if (tid == 0) { oz[0] = pz; oa[0] = am; }
        if (blk >= 0 && pos == mycur) { oz[1 + blk] = pz; oa[1 + blk] = am; }
        pzv[tid] = pz;
      }
      if (upd && slope && tid == 0) { p10 = Pm[1]; p11 = Pm[D]; }   // row 1 before thread 1 rewrites it
      if (obs || (upd && slope)) __syncthreads();
      float kfi = 0.f, rF = 0.f;
      if (obs) {
        float F = oz[0], za = oa[0];
        for (int k = 0; k < K; ++k) { F += oz[1 + k]; za += oa[1 + k]; }
        F += H;
        rF = __builtin_amdgcn_rcpf(F);
        rF = fmaf(fmaf(-F, rF, 1.0f), rF, rF);
        const float v = at4(yt4, q) - za;
        kfi = pz * rF;
        vfq[q] = v * rF;
        am = fmaf(kfi, v, am);
      }
      if (comp) *kfw = kfi;
      kfw += D;
      if (last) continue;
      if (!upd) {
        if (tid == 0) Pm[0] += ql;
        continue;
      }
      if (slope) {
        const float m1 = readlane_f(am, 1);
        if (tid == 0) am += m1;
      }
      if (comp) {
        // the own row, j = 0..tid:  P[i][j] - (Pz)_i (Pz)_j / F  (+ sigma_k^2 g_i g_j in the own block)
        const float gi = mych ? ((pos == mycur ? 1.f : 0.f) - rnb) : 0.f;
        float u0 = 0.f, u1 = 0.f;
        int a = rbase, j = 0;
        // batches of MW_RB entries: every load of a batch is issued before the first store (the
        // loop is bound by LDS latency, not bandwidth)
        constexpr int MW_RB = 16;
        for (; j + MW_RB <= tid + 1; j += MW_RB) {
          int ad[MW_RB];
          float pv[MW_RB], pj[MW_RB];
#pragma unroll
          for (int u = 0; u < MW_RB; ++u) { ad[u] = a; a += D - (j + u) - 1; }
#pragma unroll
          for (int u = 0; u < MW_RB; ++u) pv[u] = Pm[ad[u]];
#pragma unroll
          for (int u = 0; u < MW_RB; u += 4) {
            const ci_f4v q4 = obs ? *(CI_LDS const ci_f4v*)(pzv + j + u) : ci_f4v{0.f, 0.f, 0.f, 0.f};
            pj[u] = q4.x; pj[u + 1] = q4.y; pj[u + 2] = q4.z; pj[u + 3] = q4.w;
          }
#pragma unroll
          for (int u = 0; u < MW_RB; ++u) {
            float v = fmaf(-(pz * pj[u]), rF, pv[u]);
            if (mych && j + u >= boff) v = fmaf(myd2, gi * ((j + u - boff == mycur ? 1.f : 0.f) - rnb), v);
            pv[u] = v;
          }
          if (j == 0) { u0 = pv[0]; u1 = pv[1]; }
#pragma unroll
          for (int u = 0; u < MW_RB; ++u) Pm[ad[u]] = pv[u];
        }
        for (; j <= tid; ++j) {
          const float pj = obs ? pzv[j] : 0.f;
          float u = fmaf(-(pz * pj), rF, Pm[a]);
          if (mych && j >= boff) u = fmaf(myd2, gi * ((j - boff == mycur ? 1.f : 0.f) - rnb), u);
          if (j == 0) u0 = u;
          if (j == 1) u1 = u;
          Pm[a] = u;
          a += D - j - 1;
        }
        // trend: level += slope on rows and columns (T . T'), then Q
        if (slope) {
          if (tid == 0) {
            const float pz1 = obs ? pzv[1] : 0.f;
            const float u10 = fmaf(-(pz1 * pz), rF, p10), u11 = fmaf(-(pz1 * pz1), rF, p11);
            Pm[0] = ((u0 + u10) + (u10 + u11)) + ql;
          } else {
            Pm[rbase] = u0 + u1;
            if (tid == 1) Pm[D] = u1 + qs;
          }
        } else if (tid == 0) {
          Pm[0] = u0 + ql;
        }
      }
      // the changing blocks observe their next slot from t + 1 on
      if (mych && pos == 0) zc[blk] = boff + ((mycur + 1 == nb) ? 0 : mycur + 1);
      __syncthreads();
    }
    if (tid == 0) *(TF4*)(vfp + t4) = ci_f4v{vfq[0], vfq[1], vfq[2], vfq[3]};
  }
}

}  // namespace ci
