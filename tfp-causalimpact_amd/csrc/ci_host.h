// ci_host.h -- what every host unit of the C-ABI shares (ci_host.hip): the error string, HIP_TRY,
// the allocation pools and DevBuf, the device buffer that frees itself.  Internal: not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>

#include "../../include/causalimpact_amd.h"

namespace cih {

// The message ci_last_error returns: one thread-local object for the whole library.
extern thread_local std::string g_err;
int fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return cih::fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// Device allocations, streams and events are recycled through per-process pools (ci_host.hip).
// pool_free parks the buffer under the device it came from, whatever the current device is;
// pool_stream_put synchronises the stream before it parks it.
hipError_t pool_alloc(void** out, size_t bytes);
void pool_free(void* p, size_t bytes, int dev);
hipError_t pool_stream_get(hipStream_t* out);
void pool_stream_put(hipStream_t st, int dev);
hipError_t pool_event_get(hipEvent_t* out);
void pool_event_put(hipEvent_t ev, int dev);

// Compute units of `device` (256 if the query fails).
int device_cu_count(int device);

// A pooled device array that owns its memory: released when it goes out of scope, moved but never
// copied.  alloc() on a buffer that holds memory gives that back first.
template <class T> struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  int device = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept { swap(o); }
  DevBuf& operator=(DevBuf&& o) noexcept { swap(o); return *this; }   // (o frees what this held)
  void swap(DevBuf& o) { std::swap(p, o.p); std::swap(n, o.n); std::swap(device, o.device); }
  ~DevBuf() { release(); }
  hipError_t alloc(size_t count) {
    release();
    n = count;
    if (count == 0) return hipSuccess;
    (void)hipGetDevice(&device);
    return pool_alloc((void**)&p, count * sizeof(T));
  }
  void release() {
    if (p) pool_free((void*)p, n * sizeof(T), device);
    p = nullptr;
  }
};

// Copies a device array into the caller's buffer when the caller wants it (dst non-null) and the
// fit has it.
template <class T> hipError_t copy_out(T* dst, const DevBuf<T>& src) {
  if (!dst || src.n == 0) return hipSuccess;
  return hipMemcpy(dst, src.p, src.n * sizeof(T), hipMemcpyDeviceToHost);
}

// The result arrays of a fit, in the order of ci_outputs / ci_outputs_f64.
template <class T> struct OutBufs {
  const DevBuf<T> &obs, &lscale, &sscale, &w, &level, &slope, &pm, &traj, &drift, &seasonal;
  bool has_slope;
};
// Copies out every array the caller asked for; `slope` of a model without one reads 0.  (A streamed
// run delivers its results itself: ci_session_run_streamed.)
template <class O, class T> int copy_outputs(O* o, const OutBufs<T>& b) {
  HIP_TRY(copy_out(o->observation_noise_scale, b.obs));
  HIP_TRY(copy_out(o->level_scale, b.lscale));
  HIP_TRY(copy_out(o->slope_scale, b.sscale));
  HIP_TRY(copy_out(o->weights, b.w));
  HIP_TRY(copy_out(o->posterior_means, b.pm));
  HIP_TRY(copy_out(o->seasonal_drift_scales, b.drift));
  HIP_TRY(copy_out(o->level, b.level));
  HIP_TRY(copy_out(o->posterior_trajectories, b.traj));
  HIP_TRY(copy_out(o->seasonal_levels, b.seasonal));
  if (o->slope && b.has_slope) HIP_TRY(copy_out(o->slope, b.slope));
  if (o->slope && !b.has_slope) memset(o->slope, 0, b.level.n * sizeof(T));
  return 0;
}

}  // namespace cih
