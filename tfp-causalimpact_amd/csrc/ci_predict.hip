// Instantiation unit of the prediction-error filter (ci_predict.h) and its launch;
// ci_session_summarize_predictions (ci_forecast.hip) calls it.  With -DCI_FILTER_F64: the float64-input
// build and predict_launch_f64.
#include "ci_predict.h"

namespace ci {

using PredictFn = void (*)(PredArgs);

template <int HAS_SLOPE, int NS> static PredictFn predict_fn(int out) {
  if (out == PRED_FORECAST) return predict_kernel<HAS_SLOPE, NS, PRED_FORECAST, CI_FILTER_F>;
  if (out == PRED_VARIANCE) return predict_kernel<HAS_SLOPE, NS, PRED_VARIANCE, CI_FILTER_F>;
  return predict_kernel<HAS_SLOPE, NS, PRED_PIT, CI_FILTER_F>;
}

template <int HAS_SLOPE> static PredictFn predict_fn(int ns, int out) {
  switch (ns) {
    case 0: return predict_fn<HAS_SLOPE, 0>(out);
    case 2: return predict_fn<HAS_SLOPE, 2>(out);
    case 3: return predict_fn<HAS_SLOPE, 3>(out);
    case 4: return predict_fn<HAS_SLOPE, 4>(out);
    case 5: return predict_fn<HAS_SLOPE, 5>(out);
    case 6: return predict_fn<HAS_SLOPE, 6>(out);
    case 7: return predict_fn<HAS_SLOPE, 7>(out);
    default: return nullptr;
  }
}

// One filter pass over B series: `out` one of PredOut, num_seasons 0 (no block) or 2..7.
hipError_t CI_FILTER_NAME(predict_launch)(hipStream_t stream, int B, int has_slope, int num_seasons, int out,
                          const PredArgs& args) {
  const PredictFn fn = has_slope ? predict_fn<1>(num_seasons, out) : predict_fn<0>(num_seasons, out);
  if (!fn) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fn, dim3((args.N + 63) / 64, B), dim3(64), 0, stream, args);
  return hipGetLastError();
}

}  // namespace ci
