// ci_host.hip -- the shared host layer of the C-ABI (ci_host.h): the error string, the pools of
// device buffers, streams, events and pinned host buffers, and the ci_device_* / ci_host_* /
// ci_pool_trim entry points.
#include "ci_host.h"

#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <vector>

namespace cih {

thread_local std::string g_err;

int fail(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return 1;
}

namespace {
// Device allocations are recycled through a small per-process pool (exact-size match per
// device, at most POOL_CAP bytes parked; ci_pool_trim returns them): a fit allocates ~10 buffers, 100+ MB of them outputs, and
// hipMalloc / hipFree of those cost several milliseconds per fit_causalimpact() call -- comparable
// to the 12 ms the sampler itself takes.  The pool holds no caller data and no pointers escape.
struct PoolEntry { void* p; size_t bytes; int device; };
std::mutex g_pool_mu;
std::vector<PoolEntry> g_pool;
size_t g_pool_bytes = 0;
// 32 GiB of 288: a 512-series batch parks 6 GB (1 GB each of level / trajectories, 2 GB each of the
// float64 summary matrices); with the 2 GiB cap of rounds 1-2 every batch call re-allocated them.
constexpr size_t POOL_CAP = (size_t)32 << 30;
constexpr size_t HOST_POOL_CAP = (size_t)2 << 30;   // pinned host memory is the scarcer resource
}  // namespace

hipError_t pool_alloc(void** out, size_t bytes) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = 0; i < g_pool.size(); ++i)
      if (g_pool[i].bytes == bytes && g_pool[i].device == dev) {
        *out = g_pool[i].p;
        g_pool_bytes -= bytes;
        g_pool[i] = g_pool.back();
        g_pool.pop_back();
        return hipSuccess;
      }
  }
  e = hipMalloc(out, bytes);
  if (e != hipSuccess) {
    // out of memory with buffers parked: give them back and retry once
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (auto& pe : g_pool) { (void)hipSetDevice(pe.device); (void)hipFree(pe.p); }
    g_pool.clear();
    g_pool_bytes = 0;
    (void)hipSetDevice(dev);
    e = hipMalloc(out, bytes);
  }
  return e;
}

void pool_free(void* p, size_t bytes, int dev) {
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (g_pool_bytes + bytes <= POOL_CAP && g_pool.size() < 256) {
      g_pool.push_back({p, bytes, dev});
      g_pool_bytes += bytes;
      return;
    }
  }
  (void)hipFree(p);
}

// Streams and events are recycled too: hipStreamCreate / hipStreamDestroy cost about a
// millisecond each on this runtime, four of them per fit.  A parked stream is idle (it is
// synchronised before it is parked) and carries no state of the session that used it.
namespace {
template <class H> struct Parked { H h; int device; };
std::vector<Parked<hipStream_t>> g_stream_pool;
std::vector<Parked<hipEvent_t>> g_event_pool;

// Takes a parked handle of the current device out of `pool`; false: none is parked.
template <class H> bool pool_take(std::vector<Parked<H>>& pool, H* out, hipError_t* err) {
  int dev = 0;
  *err = hipGetDevice(&dev);
  if (*err != hipSuccess) return true;
  std::lock_guard<std::mutex> lk(g_pool_mu);
  for (size_t i = 0; i < pool.size(); ++i)
    if (pool[i].device == dev) {
      *out = pool[i].h;
      pool[i] = pool.back();
      pool.pop_back();
      return true;
    }
  return false;
}
}  // namespace

hipError_t pool_stream_get(hipStream_t* out) {
  hipError_t e;
  return pool_take(g_stream_pool, out, &e) ? e : hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}

void pool_stream_put(hipStream_t st, int dev) {
  if (!st) return;
  if (hipStreamSynchronize(st) == hipSuccess) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (g_stream_pool.size() < 64) { g_stream_pool.push_back({st, dev}); return; }
  }
  (void)hipStreamDestroy(st);
}

hipError_t pool_event_get(hipEvent_t* out) {
  hipError_t e;
  return pool_take(g_event_pool, out, &e) ? e : hipEventCreate(out);
}

void pool_event_put(hipEvent_t ev, int dev) {
  if (!ev) return;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (g_event_pool.size() < 128) { g_event_pool.push_back({ev, dev}); return; }
  }
  (void)hipEventDestroy(ev);
}

int device_cu_count(int device) {
  int num_cus = 256;
  (void)hipDeviceGetAttribute(&num_cus, hipDeviceAttributeMultiprocessorCount, device);
  return num_cus;
}

namespace {
// Pinned host buffers (ci_host_alloc) are recycled the same way: pinning 100 MB costs tens of
// milliseconds, several fits' worth.
struct HostEntry { void* p; size_t bytes; };
std::mutex g_host_mu;
std::vector<HostEntry> g_host_pool;       // parked (free) buffers
std::vector<HostEntry> g_host_live;       // handed out
size_t g_host_pool_bytes = 0;
}  // namespace

}  // namespace cih

using namespace cih;

extern "C" {

const char* ci_last_error(void) { return g_err.c_str(); }

int ci_device_count(int* count) {
  if (!count) return fail("count is NULL");
  HIP_TRY(hipGetDeviceCount(count));
  return 0;
}

int ci_device_synchronize(int device) {
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}

int ci_host_alloc(void** ptr, size_t bytes) {
  if (!ptr || bytes == 0) return fail("ci_host_alloc: NULL pointer or zero size");
  {
    std::lock_guard<std::mutex> lk(g_host_mu);
    for (size_t i = 0; i < g_host_pool.size(); ++i)
      if (g_host_pool[i].bytes == bytes) {
        *ptr = g_host_pool[i].p;
        g_host_live.push_back(g_host_pool[i]);
        g_host_pool_bytes -= bytes;
        g_host_pool[i] = g_host_pool.back();
        g_host_pool.pop_back();
        return 0;
      }
  }
  void* p = nullptr;
  HIP_TRY(hipHostMalloc(&p, bytes, hipHostMallocDefault));
  std::lock_guard<std::mutex> lk(g_host_mu);
  g_host_live.push_back({p, bytes});
  *ptr = p;
  return 0;
}

int ci_host_free(void* ptr) {
  if (!ptr) return 0;
  HostEntry e{nullptr, 0};
  {
    std::lock_guard<std::mutex> lk(g_host_mu);
    for (size_t i = 0; i < g_host_live.size(); ++i)
      if (g_host_live[i].p == ptr) {
        e = g_host_live[i];
        g_host_live[i] = g_host_live.back();
        g_host_live.pop_back();
        break;
      }
    if (!e.p) return fail("ci_host_free: pointer was not allocated by ci_host_alloc");
    if (g_host_pool_bytes + e.bytes <= HOST_POOL_CAP && g_host_pool.size() < 64) {
      g_host_pool.push_back(e);
      g_host_pool_bytes += e.bytes;
      return 0;
    }
  }
  HIP_TRY(hipHostFree(e.p));
  return 0;
}

int ci_pool_trim(void) {
  {
    std::lock_guard<std::mutex> lk(g_host_mu);
    for (auto& he : g_host_pool) (void)hipHostFree(he.p);
    g_host_pool.clear();
    g_host_pool_bytes = 0;
  }
  std::lock_guard<std::mutex> lk(g_pool_mu);
  int dev = 0;
  (void)hipGetDevice(&dev);
  for (auto& pe : g_pool) { (void)hipSetDevice(pe.device); (void)hipFree(pe.p); }
  g_pool.clear();
  g_pool_bytes = 0;
  for (auto& se : g_stream_pool) { (void)hipSetDevice(se.device); (void)hipStreamDestroy(se.h); }
  g_stream_pool.clear();
  for (auto& ee : g_event_pool) { (void)hipSetDevice(ee.device); (void)hipEventDestroy(ee.h); }
  g_event_pool.clear();
  (void)hipSetDevice(dev);
  return 0;
}

}  // extern "C"
