// dev_buffers.h -- the plumbing of the synchronous host entry points (host pointers in, device buffers for the
// length of one call, host pointers out): the device check, the holder of the call's device allocations, the sizing of
// a slice of signals (and the cap on it that lets a test reach the slices after the first), the sliced host call itself
// (host_slice sizes it, host_sliced runs it: H2D, run, D2H per slice), the timing events of the device entry points
// (run_timed: up to four parts, on the null stream or a caller's), and the two doors of a pipeline that is written once
// for both (pipe_host, pipe_exec).  The fp64 STFT pipelines (stft_frames64.h), the fp64 CWT map pipelines
// (cwt_maps64.h) and the two ConceFT transforms (stft_conceft.hip, cwt_conceft.hip) go through the same doors.  A host
// door sizes its slices with host_slice (a workspace linear in the signals), builds its own HostSlice from slice_signals
// (ConceFT: a workspace fixed by the call, beside which the signals are sliced), or takes the batch whole (cwt_pipe_host).
#pragma once
#include <atomic>
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

// the process-wide cap on a slice of the host entry points (ssq_host_slice_cap; 0: none)
inline std::atomic<long long>& host_slice_cap() {
  static std::atomic<long long> cap{0};
  return cap;
}

// signals of `per_signal` device bytes each that fit beside `fixed` bytes: most of the free memory, at most `cap` and
// at most host_slice_cap() (a signal's result does not depend on the slice it is in)
inline long long slice_signals(long long batch, double per_signal, double fixed, long long cap) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)1 << 30;
  double room = 0.8 * (double)free_b - fixed;
  long long s = room > per_signal ? (long long)(room / per_signal) : 1;      // one signal is always tried: hipMalloc reports the rest
  if (s > cap) s = cap;
  if (const long long hc = host_slice_cap().load(); hc > 0 && s > hc) s = hc;
  if (s > batch) s = batch;
  return s < 1 ? 1 : s;
}

// an output of a sliced host call: `bytes` per signal; host == nullptr: not asked for (no device buffer, nullptr to bind)
struct HostOut {
  void* host;
  size_t bytes;
};

// how a host call cuts its batch: signals per slice, and the workspace bytes of one slice
struct HostSlice {
  int64_t signals;
  size_t work_bytes;
};

// what a signal of a host call holds on the device outside its workspace: x and the outputs that were asked for
template <size_t N>
double host_signal_bytes(size_t x_bytes, const HostOut (&outs)[N]) {
  double per = (double)x_bytes;
  for (const HostOut& o : outs)
    if (o.host) per += (double)o.bytes;
  return per;
}

// the slice of a workspace that is linear in the signals (`work_bytes` each): slice_signals' of everything a signal
// needs on the device, host_signal_bytes and its workspace
template <size_t N>
HostSlice host_slice(int64_t batch, size_t x_bytes, const HostOut (&outs)[N], size_t work_bytes) {
  const int64_t slice = slice_signals(batch, host_signal_bytes(x_bytes, outs) + (double)work_bytes, 0.0, batch);
  return {slice, work_bytes * (size_t)slice};
}

// A synchronous host entry over a batch: x ([batch] x `x_bytes`) in, the outputs that were asked for out, in slices of
// sl.signals on a workspace of sl.work_bytes (host_slice's, or the caller's own: a workspace that is not linear in the
// signals takes the batch whole).  The buffers are allocated once.  bind(cap, d_outs, d_work) is called once with the
// slice's capacity in signals (where the pipeline carves its workspace and fixes its device pointers), then per slice:
// H2D of x, run(nb, d_x), D2H of each output.  bind and run return the entry point's status (0, or non-zero with the
// error set).
template <size_t N, typename Bind, typename Run>
int host_sliced(int64_t batch, HostSlice sl, const void* x, size_t x_bytes, const HostOut (&outs)[N], Bind&& bind, Run&& run) {
  const int64_t slice = sl.signals;
  DeviceBufs d;
  void *d_x, *d_work, *d_outs[N] = {};
  SSQ_HIP(d.alloc(&d_x, x_bytes * (size_t)slice));
  SSQ_HIP(d.alloc(&d_work, sl.work_bytes));
  for (size_t i = 0; i < N; ++i)
    if (outs[i].host) SSQ_HIP(d.alloc(&d_outs[i], outs[i].bytes * (size_t)slice));
  if (int rc = bind(slice, d_outs, d_work)) return rc;
  for (int64_t b0 = 0; b0 < batch; b0 += slice) {
    const int64_t nb = batch - b0 < slice ? batch - b0 : slice;
    SSQ_HIP(hipMemcpy(d_x, (const char*)x + x_bytes * (size_t)b0, x_bytes * (size_t)nb, hipMemcpyHostToDevice));
    if (int rc = run(nb, (const void*)d_x)) return rc;
    for (size_t i = 0; i < N; ++i)
      if (outs[i].host)
        SSQ_HIP(hipMemcpy((char*)outs[i].host + outs[i].bytes * (size_t)b0, d_outs[i], outs[i].bytes * (size_t)nb,
                          hipMemcpyDeviceToHost));
  }
  return 0;
}

// the timing events of one call, released on every path
struct TimingEvents {
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
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

// The launches of a device entry point, synchronous.  stream == nullptr: they are on the null stream and the call
// returns after hipDeviceSynchronize (the STFT entry points); else they are on *stream, the null stream included, and
// the call is synchronous on that stream (the CWT entry points).  `run(mid)` issues them and returns the entry point's
// status (0, or non-zero with the error set).  kernel_ms (may be nullptr) receives their time in n_mid + 1 consecutive
// parts (n_mid: 0 .. 3): `run` records the event mid[i], i < n_mid, on its stream where part i ends.  Without kernel_ms
// every mid[i] is nullptr and `run` records nothing.  An entry point that documents the time of several parts together
// reports their sum, which differs from one elapsed-time query across them by float rounding alone.
template <typename Run>
int run_timed(float* kernel_ms, int n_mid, const hipStream_t* stream, Run&& run) {
  TimingEvents t;
  const hipStream_t st = stream ? *stream : nullptr;
  if (!kernel_ms) {
    if (int rc = run((const hipEvent_t*)t.ev)) return rc;
    SSQ_HIP(stream ? hipStreamSynchronize(st) : hipDeviceSynchronize());
    return 0;
  }
  SSQ_HIP(t.start(n_mid + 2, st));
  if (int rc = run((const hipEvent_t*)t.ev + 1)) return rc;
  SSQ_HIP(hipEventRecord(t.ev[n_mid + 1], st));
  SSQ_HIP(hipEventSynchronize(t.ev[n_mid + 1]));
  for (int i = 0; i <= n_mid; ++i) SSQ_HIP(hipEventElapsedTime(&kernel_ms[i], t.ev[i], t.ev[i + 1]));
  return 0;
}

// The two doors of a pipeline on device buffers.  Pipe{c, s} holds the call and its shape by reference and has
//   tables()                  the call's tables on the device, once per call
//   bind(cap, outs, work)     outs: the device outputs in the entry point's order (nullptr: not asked for); work: the
//                             pipeline's workspace of `cap` signals, carved here by its one layout function
//   run(nb, d_x, mid)         the launches of nb <= cap signals; mid: run_timed's events (Pipe::kMid of them)
// each returning the entry point's status.  The mid events mark one boundary per call: a pipe whose timed stages
// alternate per inner slice (ConceFT) has kMid = 0, is handed a null kernel_ms and sums its own event pairs into a
// float* of its call struct, which the host door leaves null.  pipe_host: host pointers, in slices (sized from
// `work_bytes` a signal, or as the caller's HostSlice says); pipe_exec: the caller's device buffers and workspace at
// cap = batch, timed, `stream` as run_timed has it (the pipe itself knows where its launches go).
template <typename Pipe, typename Call, typename Shape, size_t N>
int pipe_host(const Call& c, const Shape& s, const void* x, size_t x_bytes, const HostOut (&outs)[N], HostSlice sl) {
  Pipe pl{c, s};
  if (int rc = pl.tables()) return rc;
  const hipEvent_t none[3] = {nullptr, nullptr, nullptr};
  return host_sliced(
      c.batch, sl, x, x_bytes, outs, [&](int64_t cap, void* const* o, void* work) { return pl.bind(cap, o, work); },
      [&](int64_t nb, const void* d_x) { return pl.run(nb, d_x, none); });
}

template <typename Pipe, typename Call, typename Shape, size_t N>
int pipe_host(const Call& c, const Shape& s, const void* x, size_t x_bytes, const HostOut (&outs)[N], size_t work_bytes) {
  return pipe_host<Pipe>(c, s, x, x_bytes, outs, host_slice(c.batch, x_bytes, outs, work_bytes));
}

template <typename Pipe, typename Call, typename Shape>
int pipe_exec(const Call& c, const Shape& s, const void* d_x, void* const* d_outs, void* d_work, float* kernel_ms,
              const hipStream_t* stream = nullptr) {
  Pipe pl{c, s};
  if (int rc = pl.tables()) return rc;
  if (int rc = pl.bind(c.batch, d_outs, d_work)) return rc;
  return run_timed(kernel_ms, Pipe::kMid, stream, [&](const hipEvent_t* mid) { return pl.run(c.batch, d_x, mid); });
}

}  // namespace ssq
