// Instantiation unit of the component-summary kernels (ci_components.h) and their launches;
// ci_session_summarize_components (ci_summary.hip) calls these.
#include "ci_components.h"

namespace ci {

hipError_t comp_launch_gather(hipStream_t stream, int B, int N, int T, int K, int k, const float* in,
                              const double* scales, const double* shifts, double* out) {
  const dim3 grid((T + 63) / 64, (N + 63) / 64, B), block(64, 4);
  if (shifts)
    hipLaunchKernelGGL(comp_gather_kernel<true>, grid, block, 0, stream, N, T, K, k, in, scales, shifts, out);
  else
    hipLaunchKernelGGL(comp_gather_kernel<false>, grid, block, 0, stream, N, T, K, k, in, scales, shifts, out);
  return hipGetLastError();
}

hipError_t comp_launch_regression(hipStream_t stream, int B, int N, int T, int P, const float* Xt,
                                  const float* w, const int* series_T, const double* scales,
                                  double* out) {
  hipLaunchKernelGGL(comp_regression_kernel<float>, dim3((T + 63) / 64, (N + 63) / 64, B), dim3(64, 4), 0,
                     stream, N, T, P, Xt, w, series_T, scales, out);
  return hipGetLastError();
}

hipError_t comp_launch_regression_f64(hipStream_t stream, int B, int N, int T, int P, const double* Xt,
                                      const double* w, const int* series_T, const double* scales,
                                      double* out) {
  hipLaunchKernelGGL(comp_regression_kernel<double>, dim3((T + 63) / 64, (N + 63) / 64, B), dim3(64, 4), 0,
                     stream, N, T, P, Xt, w, series_T, scales, out);
  return hipGetLastError();
}

hipError_t comp_launch_row_stats(hipStream_t stream, size_t rows, int N, const double* M,
                                 double* mean, int* nonzero) {
  hipLaunchKernelGGL(comp_row_stats_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream,
                     rows, N, M, mean, nonzero);
  return hipGetLastError();
}

}  // namespace ci
