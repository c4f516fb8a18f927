// dev_buffers.h -- the plumbing of the synchronous host entry points (host pointers in, device buffers for the
// length of one call, host pointers out): the device check and the holder of the call's device allocations.
#pragma once
#include <vector>

#include "ssq_common.h"

namespace ssq {

inline int require_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) SSQ_FAIL("no HIP device visible (there is no CPU fallback)");
  return 0;
}

// Device buffers of one synchronous host call: hipMalloc per buffer, all freed when the holder goes out of scope, so
// an entry point may return through SSQ_HIP at any point.  A request of 0 bytes still allocates (16 bytes): a kernel
// never receives nullptr for a buffer that was asked for, only for an optional one the caller left out.
struct HostCallBufs {
  std::vector<void*> ptrs;
  HostCallBufs() = default;
  HostCallBufs(const HostCallBufs&) = delete;
  HostCallBufs& operator=(const HostCallBufs&) = delete;
  ~HostCallBufs() {
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
};

}  // namespace ssq
