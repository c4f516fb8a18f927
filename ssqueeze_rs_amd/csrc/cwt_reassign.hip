// cwt_reassign.hip -- the reassigned scalogram, `upstream.reassign_cwt` (Auger and Flandrin 1995, III).
// Upstream has no such transform: the definition is the project's own, restated in numpy by
// tests/helpers/reassign_cwt_ref.py.  Every coefficient's energy |Wx|^2 moves in BOTH directions at once, to its
// instantaneous frequency (ssq_cwt's first-order operator) and its group delay.  dt enters at the end.  With the maps
// W, W1, Wt of cwt_maps64.h on columns n1 .. n1 + N - 1:
//   w   = |Im(W1/W)| / (2 pi dt)            fp64, rounded once to the call's dtype; +inf where |W| < gamma
//   tau = clamp(Re(Wt/W), -N, N) dt         fp64, rounded once to the call's dtype; +inf where |W| < gamma
//   k'  = ssqueeze.hip's bin rule on the reported w, in its dtype (then flipped, as ssq_cwt2 flips)
//   m'  = clip(j + rint(tau / dt), 0, N - 1) in the call's dtype (cwt_maps64.h's time rule)
//   Rx[k', m'] += |Wx[i, j]|^2              of the REPORTED Wx, formed in fp64; no row weights
// The pipeline up to the operator is cwt_maps64.h's.  Then:
//   cwt_reassign_operator_kernel : one thread per (row, column), lanes along time: the three values, 1 / P, 1 / |W|^2
//                              once; Wx, optionally w and tau, and the two int32 targets (k', m'; -1 where the bin is
//                              not kept), formed from the values AS ROUNDED to the call's dtype.  It also reduces
//                              max |Wx|^2 per signal (cwt_flush_max): a wave reduction, a four-value step through LDS,
//                              then ONE 64-bit integer atomic max per workgroup on the bit pattern of the double.
//   cwt_reassign_scatter_kernel : after all chunks (the scale is per signal).  One thread per source bin, lanes along
//                              time; a kept bin loads Wx, forms |Wx|^2 in fp64, converts it to fixed point (quantum
//                              q = Pmax 2^-S, S = min(38, 62 - ceil(log2(na N))), Pmax the smallest power of two >= the
//                              signal's max |Wx|^2) and issues one device-scope 64-bit integer atomic add into the
//                              zeroed accumulator [batch][na][N] in device memory.  No LDS tile: a coefficient's time
//                              reach is the wavelet's support at its scale, the whole signal for the top octaves.
//                              Integer adds commute: a cell's bits depend on the set of its contributions alone.  A
//                              contribution is at most 2^S quanta and a cell takes at most na N <= 2^(62 - S) of them.
//   cwt_reassign_readout_kernel : converts every cell once to fp64, scales it by q, rounds to the call's dtype and writes
//                              every cell of Rx exactly once.
// The head of the workspace (cwt_maps64.h's cwt_head): the signals' maxima [batch], the accumulators [batch][na][N] and
// the two int32 target maps [batch][na][N], kk then mm.  CwtRPipe runs the launches behind both doors.
#include <cmath>

#include "bin_rule.h"
#include "cwt_maps64.h"

namespace ssq {

constexpr unsigned kCwtRMapSet = kMapW | kMapW1 | kMapWt;
constexpr int kCwtRMaps = cwt_map_count(kCwtRMapSet);
constexpr int kCwtRQuantumBitsMax = 38;                       // upstream.REASSIGN_CWT_QUANTUM_LOG2_MAX

template <typename O>
struct CwtROpDev {
  const cpx<double>* maps;   // [rows][3][P]: the unnormalised inverse transforms
  cpx<O>* Wx;                // [batch * na][N], these five at the chunk's first row
  O* w;                      // or nullptr
  O* tau;                    // or nullptr
  int* kk;
  int* mm;
  unsigned long long* emax;  // [batch]: bit pattern of max |Wx|^2, zeroed before the first chunk
  long long P, N, n1, r0, rows;
  int na;
  double inv_P, gamma, inv_two_pi_dt, dt;
  O dt_o;                    // dt in the call's dtype: the time rule runs on the tau the call reports
  BinRule<O> rule;           // the bin rule (bin_rule.h) runs on the w the call reports
};

// grid (ceil(N / 256), min(rows, 65535)): thread = column j of row rl.  No thread leaves early (cwt_flush_max).
template <typename O>
__global__ __launch_bounds__(kCwtThreads) void cwt_reassign_operator_kernel(const CwtROpDev<O> p) {
  using T = double;
  __shared__ T red[kCwtThreads / 64];
  const long long j = (long long)blockIdx.x * kCwtThreads + threadIdx.x;
  const bool live = j < p.N;
  T mx = (T)0;
  long long b_cur = -1;
  for (long long rl = blockIdx.y; rl < p.rows; rl += gridDim.y) {
    const long long b = (p.r0 + rl) / p.na;
    if (b != b_cur) {
      if (b_cur >= 0) cwt_flush_max(mx, red, p.emax + b_cur);
      mx = (T)0;
      b_cur = b;
    }
    if (!live) continue;
    const cpx<T>* __restrict__ in = p.maps + rl * kCwtRMaps * p.P + p.n1 + j;
    const cpx<T> W = cscale(in[0], p.inv_P), W1 = cscale(in[p.P], p.inv_P), Wt = cscale(in[2 * p.P], p.inv_P);
    const T den = W.x * W.x + W.y * W.y;
    const T inv_den = (T)1 / den;
    const T im1 = (W1.y * W.x - W1.x * W.y) * inv_den;                      // Im(W1 / W)
    const T re_t = (Wt.x * W.x + Wt.y * W.y) * inv_den;                     // Re(Wt / W)
    const bool keep = !(hypot(W.x, W.y) < p.gamma);
    const cpx<O> Wo = {(O)W.x, (O)W.y};
    O w = (O)INFINITY, tau = (O)INFINITY;
    int kk = -1, mm = -1;
    if (keep) {
      w = (O)(fabs(im1) * p.inv_two_pi_dt);
      tau = (O)(clamp_keep_nan(re_t, (T)p.N) * p.dt);
      kk = isinf(w) ? -1 : bin_of(p.rule, w);
      cwt_time_target(tau, p.dt_o, j, p.N, mm);
      if (kk < 0) mm = -1;                                                   // (an infinite quotient: not a target)
    }
    const long long o = rl * p.N + j;
    p.Wx[o] = Wo;
    if (p.w) p.w[o] = kk < 0 ? (O)INFINITY : w;
    if (p.tau) p.tau[o] = kk < 0 ? (O)INFINITY : tau;
    p.kk[o] = kk;
    p.mm[o] = mm;
    mx = fmax(mx, energy_f64<O>(Wo));                                // (a NaN is not a maximum)
  }
  if (b_cur >= 0) cwt_flush_max(mx, red, p.emax + b_cur);
}

// the signal's scale: Pmax = the smallest power of two >= max |Wx|^2, quantum q = Pmax 2^-qbits (exponent clamped so
// that both q and 1 / q are normal numbers; a signal of zeros, or one whose energy is not finite, gets q = 0)
__device__ __forceinline__ void cwt_reassign_quantum(unsigned long long bits, int qbits, double* q, double* inv_q) {
  *q = 0.0;
  *inv_q = 0.0;
  int lp;
  if (cwt_pow2_above(bits, &lp)) {
    lp = lp < -960 ? -960 : (lp > 960 ? 960 : lp);
    *q = ldexp(1.0, lp - qbits);
    *inv_q = ldexp(1.0, qbits - lp);
  }
}

template <typename O>
struct CwtRScatDev {
  const cpx<O>* Wx;                  // [batch][na][N]
  const int* kk;                     // [batch][na][N]: target row, -1 where the bin is not kept
  const int* mm;                     // [batch][na][N]: target column
  const unsigned long long* emax;    // [batch]
  unsigned long long* acc;           // [batch][na][N]: the fixed-point cells, zeroed before the scatter
  O* Rx;                             // [batch][na][N]
  long long batch, plane, N;         // plane = na N <= 2^40
  int na, qbits;
};

// grid (min(ceil(plane / 256), 2^31 - 1), min(batch, 65535)): 64-bit flat index i over a signal's na x N bins, lanes
// along time, the x blocks stride over the plane and the y blocks over the signals
template <typename O>
__global__ __launch_bounds__(kCwtThreads) void cwt_reassign_scatter_kernel(const CwtRScatDev<O> p) {
  const long long stride = (long long)gridDim.x * kCwtThreads;
  const double cap = ldexp(1.0, p.qbits);
  for (long long b = blockIdx.y; b < p.batch; b += gridDim.y) {
    double q, inv_q;
    cwt_reassign_quantum(p.emax[b], p.qbits, &q, &inv_q);
    if (q == 0.0) continue;
    const long long base = b * p.plane;
    for (long long i = (long long)blockIdx.x * kCwtThreads + threadIdx.x; i < p.plane; i += stride) {
      const int kk = p.kk[base + i];
      if (kk < 0) continue;
      const int mm = p.mm[base + i];
      if (kk >= p.na || mm < 0 || mm >= p.N) continue;                    // (never: the operator kernel clips both)
      const double e = energy_f64<O>(p.Wx[base + i]);
      if (!(e == e)) continue;                                            // a NaN coefficient carries no energy
      const long long f = to_fixed_f64(fmin(e * inv_q, cap));    // <= 2^qbits quanta
      atomicAdd(p.acc + base + (long long)kk * p.N + mm, (unsigned long long)f);
    }
  }
}

template <typename O>
__global__ __launch_bounds__(kCwtThreads) void cwt_reassign_readout_kernel(const CwtRScatDev<O> p) {
  const long long stride = (long long)gridDim.x * kCwtThreads;
  for (long long b = blockIdx.y; b < p.batch; b += gridDim.y) {
    double q, inv_q;
    cwt_reassign_quantum(p.emax[b], p.qbits, &q, &inv_q);
    const long long base = b * p.plane;
    for (long long i = (long long)blockIdx.x * kCwtThreads + threadIdx.x; i < p.plane; i += stride)
      p.Rx[base + i] = (O)((double)(long long)p.acc[base + i] * q);
  }
}

}  // namespace ssq

using namespace ssq;

namespace {

// the head: 8 bytes of accumulator and two int32 targets per cell
constexpr CwtMapsKind kCwtRKind = {"reassign_cwt", "ssq_reassign_cwt_workspace_bytes", 16.0, 4.0e18, 0, 8, 2};

struct CwtRCall : CwtMapsCall {
  int freq_kind, variant;
  int64_t freq_transition;
  const double* f_asc;
};

int cwtr_check(const CwtRCall& c, CwtMapsShape* s) {
  const auto rows = [&]() -> int {
    if (!c.scales || !c.f_asc) SSQ_FAIL("NULL argument");
    for (int64_t i = 0; i < c.na; ++i) {
      if (!(c.scales[i] > 0) || !std::isfinite(c.scales[i])) SSQ_FAIL("reassign_cwt: scales must be positive and finite");
      if (!std::isfinite(c.f_asc[i])) SSQ_FAIL("reassign_cwt: ssq_freqs_asc must be finite");
    }
    return 0;
  };
  return cwt_maps_check(kCwtRKind, kCwtRMaps, nullptr, c, rows, &c.freq_kind, c.freq_transition, nullptr, s);
}

// reassign_cwt on device buffers (cwt_pipe_host, pipe_exec): the chunks with the operator, the scatter, the read-out.
// The targets go to the caller's planes where given, else to the head's.  kernel_ms: three parts, the events before and
// after the scatter kernel.
template <typename T>
struct CwtRPipe {
  static constexpr int kMid = 2;
  const CwtRCall& c;
  const CwtMapsShape& s;
  DeviceBufs d;
  void *scales, *work, *Wx, *w, *tau;
  int *kk, *mm;
  CwtROpDev<T> op;
  CwtRScatDev<T> sc;
  int tables() {
    SSQ_HIP(d.upload(&scales, c.scales, sizeof(double) * (size_t)c.na));
    // (cwtr_check has made each of the rule's checks already)
    return bin_rule<T>(c.f_asc, c.na, c.freq_kind, c.freq_transition, (c.variant & SSQ_VARIANT_FLIPUD) ? 1 : 0, op.rule);
  }
  int bind(int64_t, void* const* outs /* Rx, Wx, w, tau, kk, mm */, void* wk) {
    work = wk;
    Wx = outs[1];
    w = outs[2];
    tau = outs[3];
    kk = outs[4] ? static_cast<int*>(outs[4]) : cwt_head_at<int>(work, s.head.planes);
    mm = outs[5] ? static_cast<int*>(outs[5]) : cwt_head_at<int>(work, s.head.planes) + s.cells;
    op.emax = cwt_head_at<unsigned long long>(work, s.head.emax);
    op.P = s.P;
    op.N = c.N;
    op.n1 = s.n1;
    op.na = (int)c.na;
    op.inv_P = 1.0 / (double)s.P;
    op.gamma = s.gamma;
    op.inv_two_pi_dt = 1.0 / (6.283185307179586 * c.dt);
    op.dt = c.dt;
    op.dt_o = (T)c.dt;
    int L = 0;
    while (((int64_t)1 << L) < s.plane) ++L;                    // ceil(log2(na N)) <= 40
    sc.Wx = static_cast<const cpx<T>*>(Wx);
    sc.kk = kk;
    sc.mm = mm;
    sc.emax = op.emax;
    sc.acc = cwt_head_at<unsigned long long>(work, s.head.acc);
    sc.Rx = static_cast<T*>(outs[0]);
    sc.batch = c.batch;
    sc.plane = s.plane;
    sc.N = c.N;
    sc.na = (int)c.na;
    sc.qbits = std::min(kCwtRQuantumBitsMax, 62 - L);
    return 0;
  }
  int run(int64_t, const void* d_x, const hipEvent_t* mid) {
    const int64_t N = c.N;
    const hipStream_t st = c.st;
    SSQ_HIP(hipMemsetAsync(op.emax, 0, (size_t)(s.head.planes - s.head.emax), st));   // the maxima and the accumulators
    const auto launch_op = [&](const cpx<double>* maps, int64_t r0, int64_t nr) -> int {
      op.maps = maps;
      op.Wx = static_cast<cpx<T>*>(Wx) + r0 * N;
      op.w = w ? static_cast<T*>(w) + r0 * N : nullptr;
      op.tau = tau ? static_cast<T*>(tau) + r0 * N : nullptr;
      op.kk = kk + r0 * N;
      op.mm = mm + r0 * N;
      op.r0 = r0;
      op.rows = nr;
      hipLaunchKernelGGL((cwt_reassign_operator_kernel<T>), cwt_rows_grid(N, nr), dim3(kCwtThreads), 0, st, op);
      SSQ_HIP(hipGetLastError());
      return 0;
    };
    if (int rc = cwt_maps_chunks<T, kCwtRMapSet>(c, s, d_x, scales, work, launch_op)) return rc;
    const dim3 grid((unsigned)std::min<int64_t>((s.plane + kCwtThreads - 1) / kCwtThreads, 0x7fffffffLL),
                    (unsigned)std::min<int64_t>(c.batch, 65535));
    if (mid[0]) SSQ_HIP(hipEventRecord(mid[0], st));
    hipLaunchKernelGGL((cwt_reassign_scatter_kernel<T>), grid, dim3(kCwtThreads), 0, st, sc);
    SSQ_HIP(hipGetLastError());
    if (mid[1]) SSQ_HIP(hipEventRecord(mid[1], st));
    hipLaunchKernelGGL((cwt_reassign_readout_kernel<T>), grid, dim3(kCwtThreads), 0, st, sc);
    SSQ_HIP(hipGetLastError());
    return 0;
  }
};

}  // namespace

extern "C" {

int64_t ssq_reassign_cwt_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int64_t* min_bytes) {
  CwtMapsShape s;
  if (cwt_maps_shape(kCwtRKind, kCwtRMaps, nullptr, dtype, batch, n_signal, na, &s)) return -1;
  if (min_bytes) *min_bytes = s.min_bytes;
  return s.pref_bytes;
}

int ssq_reassign_cwt_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                          const double* scales, int64_t na, double dt, const double* ssq_freqs_asc, int freq_kind,
                          int64_t freq_transition, int padtype, double gamma, int variant, void* d_Rx, void* d_Wx,
                          void* d_w, void* d_tau, void* d_kk, void* d_mm, void* d_workspace, int64_t workspace_bytes,
                          void* stream, float* kernel_ms) {
  if (!d_x || !d_Rx || !d_Wx || !d_workspace) SSQ_FAIL("NULL argument");
  const CwtRCall c{{dtype, wavelet, padtype, batch, n_signal, na, p0, p1, dt, gamma, scales, (hipStream_t)stream},
                   freq_kind, variant, freq_transition, ssq_freqs_asc};
  CwtMapsShape s;
  if (int rc = cwtr_check(c, &s)) return rc;
  if (int rc = cwt_exec_bytes(kCwtRKind, &s, workspace_bytes)) return rc;
  if (int rc = require_device()) return rc;
  void* const outs[] = {d_Rx, d_Wx, d_w, d_tau, d_kk, d_mm};
  float part[3], *ms = kernel_ms ? part : nullptr;
  const int rc = dtype == SSQ_F32 ? pipe_exec<CwtRPipe<float>>(c, s, d_x, outs, d_workspace, ms, &c.st)
                                  : pipe_exec<CwtRPipe<double>>(c, s, d_x, outs, d_workspace, ms, &c.st);
  if (rc == 0 && kernel_ms) {
    kernel_ms[0] = part[0] + part[1] + part[2];                // all the kernels
    kernel_ms[1] = part[1];                                    // the scatter kernel alone
  }
  return rc;
}

int ssq_reassign_cwt_host(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                          const double* scales, int64_t na, double dt, const double* ssq_freqs_asc, int freq_kind,
                          int64_t freq_transition, int padtype, double gamma, int variant, int64_t work_limit_bytes,
                          void* Rx, void* Wx, void* w, void* tau, void* kk, void* mm) {
  if (!x || !Rx || !Wx) SSQ_FAIL("NULL argument");
  const CwtRCall c{{dtype, wavelet, padtype, batch, n_signal, na, p0, p1, dt, gamma, scales, nullptr},
                   freq_kind, variant, freq_transition, ssq_freqs_asc};
  CwtMapsShape s;
  if (int rc = cwtr_check(c, &s)) return rc;
  if (int rc = cwt_host_bytes(kCwtRKind, &s, batch, work_limit_bytes)) return rc;
  if (int rc = require_device()) return rc;
  const size_t el = (dtype == SSQ_F32 ? 4 : 8) * (size_t)s.plane, i32 = sizeof(int32_t) * (size_t)s.plane;
  const HostOut outs[] = {{Rx, el}, {Wx, 2 * el}, {w, el}, {tau, el}, {kk, i32}, {mm, i32}};
  return dtype == SSQ_F32 ? cwt_pipe_host<CwtRPipe<float>>(c, s, x, outs) : cwt_pipe_host<CwtRPipe<double>>(c, s, x, outs);
}

}  // extern "C"
