// dev_buffers.h -- the plumbing of the synchronous host entry points (host pointers in, device buffers for the
// length of one call, host pointers out): the device check, the holder of the call's device allocations, the sizing of
// a slice of signals, and the timing events of the device entry points.
#pragma once
#include <vector>

#include "ssq_common.h"

namespace ssq {

inline int require_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) SSQ_FAIL("no HIP device visible (there is no CPU fallback)");
  return 0;
}

// Device buffers with one owner -- a synchronous host call, or a plan (its tables): hipMalloc per buffer, all freed
// when the holder is destroyed, so an entry point or a plan's creation may return through SSQ_HIP at any point and
// nobody lists the buffers a second time to free them.  A request of 0 bytes still allocates (16 bytes): a kernel
// never receives nullptr for a buffer that was asked for, only for an optional one the caller left out.
struct DeviceBufs {
  std::vector<void*> ptrs;
  DeviceBufs() = default;
  DeviceBufs(const DeviceBufs&) = delete;
  DeviceBufs& operator=(const DeviceBufs&) = delete;
  ~DeviceBufs() {
    for (void* p : ptrs) (void)hipFree(p);
  }
  hipError_t alloc(void** out, size_t bytes) {
    *out = nullptr;
    const hipError_t e = hipMalloc(out, bytes ? bytes : 16);
    if (e == hipSuccess) ptrs.push_back(*out);
    return e;
  }
  // alloc + copy of `bytes` from the host; only a request of 0 bytes copies nothing (src is then not read), so a
  // NULL src with bytes > 0 is a HIP error, not a silent allocation
  hipError_t upload(void** out, const void* src, size_t bytes) {
    hipError_t e = alloc(out, bytes);
    if (e == hipSuccess && bytes) e = hipMemcpy(*out, src, bytes, hipMemcpyHostToDevice);
    return e;
  }
  // upload of a host vector into a pointer of any element type
  template <typename P, typename V>
  hipError_t upload(P** out, const std::vector<V>& h) {
    return upload((void**)out, h.data(), sizeof(V) * h.size());
  }
};

// signals of `per_signal` device bytes each that fit beside `fixed` bytes: most of the free memory, at most `cap`
// (a signal's result does not depend on the slice it is in)
inline long long slice_signals(long long batch, double per_signal, double fixed, long long cap) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)1 << 30;
  double room = 0.8 * (double)free_b - fixed;
  long long s = room > per_signal ? (long long)(room / per_signal) : 1;      // one signal is always tried: hipMalloc reports the rest
  if (s > cap) s = cap;
  if (s > batch) s = batch;
  return s < 1 ? 1 : s;
}

// the timing events of one call, released on every path
struct TimingEvents {
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  TimingEvents() = default;
  TimingEvents(const TimingEvents&) = delete;
  TimingEvents& operator=(const TimingEvents&) = delete;
  ~TimingEvents() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  // creates the first `n` events and records ev[0] on `st`
  hipError_t start(int n, hipStream_t st) {
    for (int i = 0; i < n; ++i)
      if (hipError_t e = hipEventCreate(&ev[i]); e != hipSuccess) return e;
    return hipEventRecord(ev[0], st);
  }
};

// The launches of a device entry point on the null stream, synchronous.  `run(mid)` issues them and returns the entry
// point's status (0, or non-zero with the error set); kernel_ms (may be nullptr) receives their time: one float, or with `split` two, the launches before and
// after the point where `run` records the event `mid` it is handed (nullptr when no time is asked for).
template <typename Run>
int run_timed(float* kernel_ms, bool split, Run&& run) {
  if (!kernel_ms) {
    if (int rc = run((hipEvent_t) nullptr)) return rc;
    SSQ_HIP(hipDeviceSynchronize());
    return 0;
  }
  TimingEvents t;
  SSQ_HIP(t.start(3, nullptr));
  if (int rc = run(split ? t.ev[1] : (hipEvent_t) nullptr)) return rc;
  SSQ_HIP(hipEventRecord(t.ev[2], nullptr));
  SSQ_HIP(hipEventSynchronize(t.ev[2]));
  if (split) {
    SSQ_HIP(hipEventElapsedTime(&kernel_ms[0], t.ev[0], t.ev[1]));
    SSQ_HIP(hipEventElapsedTime(&kernel_ms[1], t.ev[1], t.ev[2]));
  } else {
    SSQ_HIP(hipEventElapsedTime(kernel_ms, t.ev[0], t.ev[2]));
  }
  return 0;
}

}  // namespace ssq
