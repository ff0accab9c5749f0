// Instantiation unit of the block-model prediction-error filter (ci_predict_blocks.h) and its launch;
// ci_session_summarize_predictions_blocks (ci_forecast.hip) calls it.  With -DCI_FILTER_F64: the
// float64-input build and predict_blocks_launch_f64.
#include "ci_predict_blocks.h"

namespace ci {

using PredictBlocksFn = void (*)(PredBlocksArgs);

template <int G> static PredictBlocksFn predict_blocks_fn(int out) {
  if (out == PRED_FORECAST) return predict_blocks_kernel<G, PRED_FORECAST, CI_FILTER_F>;
  if (out == PRED_VARIANCE) return predict_blocks_kernel<G, PRED_VARIANCE, CI_FILTER_F>;
  return predict_blocks_kernel<G, PRED_PIT, CI_FILTER_F>;
}

// The lanes per filter of a state of d components: the smallest of 8, 16, 32, 64 that holds it.
#ifdef CI_FILTER_F64
int blocks_group_size(int d);
#else
int blocks_group_size(int d) { return d <= 8 ? 8 : d <= 16 ? 16 : d <= 32 ? 32 : 64; }
#endif

// One filter pass over B series: `out` one of PredOut, args.m.d <= 64.
hipError_t CI_FILTER_NAME(predict_blocks_launch)(hipStream_t stream, int B, int out, const PredBlocksArgs& args) {
  if (args.m.d < 1 || args.m.d > PB_MAX_STATE) return hipErrorInvalidValue;
  const int G = blocks_group_size(args.m.d);
  const PredictBlocksFn fn = G == 8 ? predict_blocks_fn<8>(out) : G == 16 ? predict_blocks_fn<16>(out)
                           : G == 32 ? predict_blocks_fn<32>(out) : predict_blocks_fn<64>(out);
  const int fpw = 64 / G;
  hipLaunchKernelGGL(fn, dim3((args.p.N + fpw - 1) / fpw, B), dim3(64), 0, stream, args);
  return hipGetLastError();
}

}  // namespace ci
