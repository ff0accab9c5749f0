// ci_seasonal_mw.hip -- object file holding the multi-wavefront builds of the sequential seasonal
// Gibbs kernel (ci_seasonal_mw.h): states of 65-256 components, MW_NWV wavefronts per chain.  Bit 0
// of the selector: arrays over time in the HBM workspace; bit 1: P > MAXP (regression block there too).
#include <hip/hip_runtime.h>

#include "ci_seasonal.h"
#include "ci_inst.h"

extern "C" void* ci_gibbs_seasonal_mw_fn(int which) {
  switch (which) {
    case 0: return (void*)(&ci::gibbs_seasonal_kernel<false, false, ci::MW_NWV>);
    case 1: return (void*)(&ci::gibbs_seasonal_kernel<true, false, ci::MW_NWV>);
    case 2: return (void*)(&ci::gibbs_seasonal_kernel<false, true, ci::MW_NWV>);
    default: return (void*)(&ci::gibbs_seasonal_kernel<true, true, ci::MW_NWV>);
  }
}
