// Instantiations of the time-parallel general seasonal kernel (ci_seasonal_tp.h): one per width of
// the register rows (4 NQ = 8, 12, ..., 32 columns).  CI_TP_NQ selects ONE of them so that the seven
// builds compile in parallel (csrc/Makefile).
#include <hip/hip_runtime.h>

#include "ci_seasonal_tp.h"
#include "ci_inst.h"

#ifndef CI_TP_NQ
#error "compile with -DCI_TP_NQ=2..8"
#endif

#define CI_TP_CAT2(a, b) a##b
#define CI_TP_CAT(a, b) CI_TP_CAT2(a, b)

extern "C" const CiKernelInst* CI_TP_CAT(ci_seasonal_tp_inst_nq, CI_TP_NQ)(void) {
  static const CiKernelInst inst = {(void*)&ci::gibbs_seasonal_tp_kernel<CI_TP_NQ>};
  return &inst;
}
