// ci_ragged.hip -- the RAGGED build of the four-wavefront Gibbs kernel (per-series lengths,
// ci_session_create_ragged), one (D, L) instantiation per object file like ci_inst.hip.  Compile
// with -DCI_D=<1|2> -DCI_L=<1|2|4|8|16>.  Kept apart from ci_inst.hip: the stock instantiations
// are not recompiled next to it and stay the code objects they were.
#include <hip/hip_runtime.h>

#include "ci_kernels.h"
#include "ci_inst.h"

#ifndef CI_D
#error "define CI_D"
#endif
#ifndef CI_L
#error "define CI_L"
#endif

#define CI_CAT_(a, b, c, d) a##b##c##d
#define CI_CAT(a, b, c, d) CI_CAT_(a, b, c, d)

namespace {

// The device-function handle of gibbs_kernel<CI_D, CI_L, pm, false, true> (pm as in ci_inst.hip;
// there is no instrumented ragged build).
void* gibbs_fn(int pm) {
  if (pm == 0) return (void*)(&ci::gibbs_kernel<CI_D, CI_L, 0, false, true>);
  if (pm == 1) return (void*)(&ci::gibbs_kernel<CI_D, CI_L, 1, false, true>);
  if (pm == 2) return (void*)(&ci::gibbs_kernel<CI_D, CI_L, 2, false, true>);
#if CI_L >= 8
  if (pm == 3) return (void*)(&ci::gibbs_kernel<CI_D, CI_L, 3, false, true>);
#endif
  return nullptr;
}

}  // namespace

extern "C" const CiRaggedInst* CI_CAT(ci_ragged_inst_d, CI_D, _l, CI_L)(void) {
  static const CiRaggedInst inst = {gibbs_fn};
  return &inst;
}
