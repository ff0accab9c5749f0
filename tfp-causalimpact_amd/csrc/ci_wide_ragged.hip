// ci_wide_ragged.hip -- the RAGGED build of the time-parallel trend + seasonal Gibbs kernel
// (per-series lengths, ci_session_create_ragged_seasonal), one (TR, NS) instantiation per object
// file like ci_wide.hip.  Compile with -DCI_TR=<1|2> -DCI_NS=<seasons>.  Kept apart from
// ci_wide.hip: the stock instantiations are not compiled next to it and stay the code objects
// they were.
#include <hip/hip_runtime.h>

#define CI_SEASONAL_DECL_ONLY
#include "ci_wide.h"
#include "ci_inst.h"

#define CI_CAT_(a, b, c, d) a##b##c##d
#define CI_CAT(a, b, c, d) CI_CAT_(a, b, c, d)

// The device-function handle of gibbs_wide_kernel<CI_TR, CI_NS, false, true> (<= 52 design columns).
extern "C" const CiKernelInst* CI_CAT(ci_wide_ragged_inst_tr, CI_TR, _ns, CI_NS)(void) {
  static const CiKernelInst inst = {(void*)(&ci::gibbs_wide_kernel<CI_TR, CI_NS, false, true>)};
  return &inst;
}
