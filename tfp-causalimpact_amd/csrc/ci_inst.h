// ci_inst.h -- what the instantiation objects export, shared by the units that define it and the
// host units that call it: one table of function pointers per kind of object, one getter per
// object, one lookup per kind.  The (D, L) and (TR, NS) lists are written here and nowhere else.
// Host declarations only: including it changes no kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace ci {
struct HmcArgs;
struct HmcSeries;
struct WideScoreArgs;
struct HmcWideArgs;
struct SeqScoreArgs;
struct HmcSeqArgs;
struct G64Args;
}  // namespace ci

// ci_inst.hip, one (D, L) per object.
struct CiInst {
  // gibbs_kernel<D, L, pm[, profiled]>: pm + 8 selects the instrumented variant; null if not built
  void* (*gibbs)(int pm);
  // gibbs_kernel8<D, L>: xg = 0 the design in LDS (*lds_base = LDS bytes without it), xg = 1 read from L2
  void* (*gibbs8)(int profiled, int xg, size_t* lds_base);
  void (*launch_dk)(int T, const float* resid, const uint8_t* mask, float H, float sig0, float sig1,
                    float a1, float p10, float p11, uint32_t k0, uint32_t k1, uint32_t chain,
                    uint32_t iter, float* out);
  void (*launch_loglik)(int T, int P, int E, const float* y, const uint8_t* mask, const float* Xt,
                        const double* theta, float a1, float p10, float p11, double* out,
                        hipStream_t stream);
  void (*launch_llgrad)(int T, int P, int E, const float* y, const uint8_t* mask, const float* Xt,
                        const double* theta, float a1, float p10, float p11, double* out_ll,
                        double* out_grad, hipStream_t stream);
  void (*launch_latents)(int T, int P, int E, const float* y, const uint8_t* mask, const float* Xt,
                         const double* theta, float a1, float p10, float p11, uint32_t k0, uint32_t k1,
                         uint32_t rng_chain, uint32_t iter0, int per_chain, int group,
                         int chains_per_series, int series_stream_base, const ci::HmcSeries* ser,
                         float* level, float* slope, float* loc, float* traj, float* loc_sum,
                         hipStream_t stream);
  void (*launch_hmc)(const ci::HmcArgs* args, hipStream_t stream);
};
// ci_ragged.hip, one (D, L) per object: gibbs_kernel<D, L, pm, false, ragged>.
struct CiRaggedInst {
  void* (*gibbs)(int pm);
};
// ci_wide.hip, one (TR, NS) per object.
struct CiWideInst {
  void* gibbs;                                  // gibbs_wide_kernel<TR, NS>
  void (*launch_score)(const ci::WideScoreArgs* a, hipStream_t stream);
  void (*launch_hmc)(const ci::HmcWideArgs* a, hipStream_t stream);
};
// ci_wide_ragged.hip, ci_wide_bigp.hip (one (TR, NS) each) and ci_seasonal_tp.hip (one NQ each).
struct CiKernelInst {
  void* gibbs;
};

// The lists: X(table type, getter stem, a, b) for every object of a kind.
#define CI_DL_LIST(X, T, s)                                                                         \
  X(T, s, 1, 1) X(T, s, 1, 2) X(T, s, 1, 4) X(T, s, 1, 8) X(T, s, 1, 16) X(T, s, 2, 1) X(T, s, 2, 2) \
  X(T, s, 2, 4) X(T, s, 2, 8) X(T, s, 2, 16)
#define CI_TRNS_LIST(X, T, s)                                                                       \
  X(T, s, 1, 2) X(T, s, 1, 3) X(T, s, 1, 4) X(T, s, 1, 5) X(T, s, 1, 6) X(T, s, 1, 7) X(T, s, 2, 2) \
  X(T, s, 2, 3) X(T, s, 2, 4) X(T, s, 2, 5) X(T, s, 2, 6) X(T, s, 2, 7)
#define CI_NQ_LIST(X, T, s) X(T, s, 2, 0) X(T, s, 3, 0) X(T, s, 4, 0) X(T, s, 5, 0) X(T, s, 6, 0) X(T, s, 7, 0) X(T, s, 8, 0)
// one getter per object (ci_inst_d1_l1, ci_wide_inst_tr2_ns7, ci_seasonal_tp_inst_nq4, ...)
#define CI_GET_DL(T, s, D, L) const T* ci_##s##_d##D##_l##L(void);
#define CI_GET_TRNS(T, s, TR, NS) const T* ci_##s##_tr##TR##_ns##NS(void);
#define CI_GET_NQ(T, s, NQ, _) const T* ci_##s##_nq##NQ(void);

extern "C" {
CI_DL_LIST(CI_GET_DL, CiInst, inst) CI_DL_LIST(CI_GET_DL, CiRaggedInst, ragged_inst)
CI_TRNS_LIST(CI_GET_TRNS, CiWideInst, wide_inst) CI_TRNS_LIST(CI_GET_TRNS, CiKernelInst, wide_ragged_inst)
CI_TRNS_LIST(CI_GET_TRNS, CiKernelInst, wide_bigp_inst) CI_NQ_LIST(CI_GET_NQ, CiKernelInst, seasonal_tp_inst)

// ci_seasonal.hip, ci_seasonal_mw.hip: one object each.  `which`: bit 0 the arrays over time in the
// HBM workspace, bit 1 P > MAXP.
void* ci_gibbs_seasonal_fn(int which);
void* ci_gibbs_seasonal_mw_fn(int which);
void ci_launch_seq_score(const ci::SeqScoreArgs* args, int D, hipStream_t stream);
void ci_launch_hmc_seq(const ci::HmcSeqArgs* args, int D, hipStream_t stream);
void ci_launch_gibbs64(const ci::G64Args* args, int grid, size_t lds, int global_ws, hipStream_t stream);
}  // extern "C"

// The lookups, one per kind: null when no such object is built.
#define CI_PICK_DL(T, s, D, L) if (a == D && b == L) return ci_##s##_d##D##_l##L();
#define CI_PICK_TRNS(T, s, TR, NS) if (a == TR && b == NS) return ci_##s##_tr##TR##_ns##NS();
#define CI_PICK_NQ(T, s, NQ, _) if (a == NQ) return ci_##s##_nq##NQ();
#define CI_LOOKUP(T, s, LIST, PICK) inline const T* ci_##s(int a, int b = 0) { LIST(PICK, T, s) (void)b; return nullptr; }
CI_LOOKUP(CiInst, inst, CI_DL_LIST, CI_PICK_DL)                           // ci_inst(D, L)
CI_LOOKUP(CiRaggedInst, ragged_inst, CI_DL_LIST, CI_PICK_DL)              // ci_ragged_inst(D, L)
CI_LOOKUP(CiWideInst, wide_inst, CI_TRNS_LIST, CI_PICK_TRNS)              // ci_wide_inst(TR, NS)
CI_LOOKUP(CiKernelInst, wide_ragged_inst, CI_TRNS_LIST, CI_PICK_TRNS)     // ci_wide_ragged_inst(TR, NS)
CI_LOOKUP(CiKernelInst, wide_bigp_inst, CI_TRNS_LIST, CI_PICK_TRNS)       // ci_wide_bigp_inst(TR, NS)
CI_LOOKUP(CiKernelInst, seasonal_tp_inst, CI_NQ_LIST, CI_PICK_NQ)         // ci_seasonal_tp_inst(NQ)
