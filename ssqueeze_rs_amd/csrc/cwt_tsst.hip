// cwt_tsst.hip -- the time-reassigned synchrosqueezed CWT, `upstream.tssq_cwt`.  Upstream has no such
// transform: the definition is the project's own, restated in numpy by tests/helpers/tssq_cwt_ref.py.  Every complex
// coefficient moves along TIME inside its own row, to its group delay, and is rotated to keep its phase reference; rows do
// not mix.  dt enters at the end.  With the maps of cwt_maps64.h (order 1: W and Wt; order 2: all five) on columns
// n1 .. n1 + N - 1:
//   nu_i = wc / (2 pi a_i) cycles/sample: the row's frequency, an argument [na] (the library never derives it)
//   d1  = Re(Wt / W)
//   D   = W^2 + Wt1 W - Wt W1      num = W2 W - W1^2
//   d2  = d1 - Im((D / num) (2 pi nu_i + i W1 / W))        the group delay of the locally fitted log-quadratic spectrum
//   off = d2 where order = 2, |num| > gamma^2, d2 is finite and |d2| <= N, else d1; clamped to [-N, N] (a NaN stays)
//   tau = off dt, fp64 rounded once to the call's dtype; +inf where |W| < gamma
//   m'  = clip(j + rint(tau / dt), 0, N - 1) in the call's dtype, on the REPORTED tau (cwt_maps64.h's time rule)
//   Tx[i, m'] += Wx[i, j] exp(-2 pi i frac(nu_i (j - m')))  of the REPORTED Wx, the product in fp64
// The pipeline up to the operator is cwt_maps64.h's.  Then:
//   cwt_tsst_operator_kernel<O, ORDER> : one thread per (row, column), lanes along time: the values, 1 / P, 1 / |W|^2 and
//                              1 / |num|^2 once; Wx, optionally tau, and the int32 target m' (-1 where the bin is not
//                              kept), formed from the values AS ROUNDED to the call's dtype.  It also reduces max |Wx|^2
//                              per signal (cwt_flush_max).
//   cwt_tsst_scatter_kernel<O> : after all chunks (the scale is per signal).  One thread per source bin, 64-bit flat index,
//                              lanes along time; a kept bin loads Wx, rotates it in fp64, converts both parts to fixed
//                              point (quantum q = A 2^-S, S = min(38, 61 - ceil(log2 N)), A the smallest power of two >=
//                              sqrt(Pmax), Pmax the smallest power of two >= the signal's max |Wx|^2); adjacent lanes of a
//                              wave that name one cell (an impulse: all 64) are merged by an exact integer segmented sum
//                              over cross-lane shuffles, and the last lane of every run issues two device-scope 64-bit
//                              integer atomic adds into the zeroed accumulator [batch][na][N][2].  Signed sums are two's
//                              complement in the unsigned add.  Integer adds commute and associate: a cell's bits depend
//                              on the set of its contributions alone, merged or not.  A part is at most 2^S quanta and a
//                              cell takes at most N of them (one row), so |cell| < 2^61.
//   cwt_tsst_readout_kernel<O> : converts every cell once to fp64, scales it by q, rounds to the call's dtype and writes
//                              every cell of Tx exactly once.
// The rotation's angle is formed in turns: one fma of the exact product nu r against rint(nu r), rounded once, then sinpi
// / cospi: its error does not grow with |r| <= N.
// The head of the workspace (cwt_maps64.h's cwt_head): the signals' maxima [batch], the accumulators [batch][na][N][2]
// and the int32 target map [batch][na][N].  CwtTPipe runs the two halves behind both doors.
#include <cmath>

#include "cwt_tsst.h"

namespace ssq {

// grid (ceil(N / 256), min(rows, 65535)): thread = column j of row rl.  No thread leaves early (cwt_flush_max).
template <typename O, int ORDER>
__global__ __launch_bounds__(kCwtThreads) void cwt_tsst_operator_kernel(const CwtTOpDev<O> p) {
  using T = double;
  constexpr int M = cwt_tsst_maps(ORDER);
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
    const cpx<T>* __restrict__ in = p.maps + rl * M * p.P + p.n1 + j;
    const cpx<T> W = cscale(in[0], p.inv_P), Wt = cscale(in[(ORDER == 2 ? 3 : 1) * p.P], p.inv_P);
    const T den = W.x * W.x + W.y * W.y;
    const T inv_den = (T)1 / den;
    T off = (Wt.x * W.x + Wt.y * W.y) * inv_den;                            // d1 = Re(Wt / W)
    if constexpr (ORDER == 2) {
      const cpx<T> W1 = cscale(in[p.P], p.inv_P), W2 = cscale(in[2 * p.P], p.inv_P), Wt1 = cscale(in[4 * p.P], p.inv_P);
      const cpx<T> D = cmul(W, W) + cmul(Wt1, W) - cmul(Wt, W1);
      const cpx<T> num = cmul(W2, W) - cmul(W1, W1);
      const cpx<T> o = {(W1.x * W.x + W1.y * W.y) * inv_den, (W1.y * W.x - W1.x * W.y) * inv_den};   // W1 / W
      const cpx<T> z = {(T)6.283185307179586 * p.nu[(p.r0 + rl) - b * p.na] - o.y, o.x};             // 2 pi nu + i W1 / W
      const T nn = num.x * num.x + num.y * num.y;
      const T inv_nn = (T)1 / nn;
      const cpx<T> g = {(D.x * num.x + D.y * num.y) * inv_nn, (D.y * num.x - D.x * num.y) * inv_nn};   // D / num
      const T d2 = off - (g.x * z.y + g.y * z.x);
      if (hypot(num.x, num.y) > p.gamma_sq && isfinite(d2) && fabs(d2) <= (T)p.N) off = d2;
    }
    const bool keep = !(hypot(W.x, W.y) < p.gamma);
    const cpx<O> Wo = {(O)W.x, (O)W.y};
    O tau = (O)INFINITY;
    int mm = -1;
    if (keep) {
      tau = (O)(clamp_keep_nan(off, (T)p.N) * p.dt);
      if (!isinf(tau)) {                                                      // (an offset that overflows: not a target)
        cwt_time_target(tau, p.dt_o, j, p.N, mm);
      } else {
        tau = (O)INFINITY;
      }
    }
    const long long o = rl * p.N + j;
    p.Wx[o] = Wo;
    if (p.tau) p.tau[o] = tau;
    p.mm[o] = mm;
    mx = fmax(mx, energy_f64<O>(Wo));                                // (a NaN is not a maximum)
  }
  if (b_cur >= 0) cwt_flush_max(mx, red, p.emax + b_cur);
}

// the signal's scale: Pmax = the smallest power of two >= max |Wx|^2, A = the smallest power of two >= sqrt(Pmax), quantum
// q = A 2^-qbits (both q and 1 / q normal numbers; a signal of zeros, or one whose energy is not finite, gets q = 0)
__device__ __forceinline__ void cwt_tsst_quantum(unsigned long long bits, int qbits, double* q, double* inv_q) {
  *q = 0.0;
  *inv_q = 0.0;
  int lp;
  if (cwt_pow2_above(bits, &lp)) {
    const int la = (lp + 1) >> 1;                                        // ceil(lp / 2): A = 2^la
    *q = ldexp(1.0, la - qbits);
    *inv_q = ldexp(1.0, qbits - la);
  }
}

// grid (min(ceil(plane / 256), 2^31 - 1), min(batch, 65535)): 64-bit flat index i over a signal's na x N bins, lanes
// along time, the x blocks stride over the plane and the y blocks over the signals
template <typename O>
__global__ __launch_bounds__(kCwtThreads) void cwt_tsst_scatter_kernel(const CwtTScatDev<O> p) {
  const long long stride = (long long)gridDim.x * kCwtThreads;
  const double cap = ldexp(1.0, p.qbits);
  for (long long b = blockIdx.y; b < p.batch; b += gridDim.y) {
    double q, inv_q;
    cwt_tsst_quantum(p.emax[b], p.qbits, &q, &inv_q);
    if (q == 0.0) continue;
    const long long base = b * p.plane;
    const int lane = threadIdx.x & 63;
    // the loop is uniform over the wave (start and stride are multiples of 64): every lane takes part in the shuffles
    for (long long i = (long long)blockIdx.x * kCwtThreads + threadIdx.x; i - lane < p.plane; i += stride) {
      long long cellno = -1, fr = 0, fi = 0;                               // cellno -1: nothing to add
      if (i < p.plane) {
        const int mm = p.mm[base + i];
        const cpx<O> S = p.Wx[base + i];
        const double a = (double)S.x, c = (double)S.y;
        // (mm is never above N - 1: the operator kernel clips); a NaN coefficient adds nothing
        if (mm >= 0 && mm < p.N && a == a && c == c) {
          const long long row = i / p.N;
          const double nu = p.nu[row];
          const double r = (double)((i - row * p.N) - (long long)mm);     // j - m', |r| < N <= 2^26: exact
          // frac(nu r) in turns, |f| <= 1/2 (+ 1 ulp): ONE fma on the exact product.  (Written as (t - rint(t)) +
          // fma(nu, r, -t) the compiler contracts the first term to this very fma and the remainder is counted twice:
          // an angle error of up to half an ulp of nu r turns, which grows with |r|.  DESIGN 4.22.)
          const double f = fma(nu, r, -rint(nu * r));
          const double sn = sinpi(-2.0 * f), cs = cospi(-2.0 * f);
          const double re = a * cs - c * sn, im = a * sn + c * cs;
          fr = to_fixed_f64(fmax(fmin(re * inv_q, cap), -cap));           // |.| <= 2^qbits quanta
          fi = to_fixed_f64(fmax(fmin(im * inv_q, cap), -cap));
          cellno = base + row * p.N + mm;
        }
      }
      // runs of adjacent lanes that name one cell: an exact integer segmented sum, then one pair of adds per run by the
      // run's last lane.  A run's head is a lane whose left neighbour names another cell (a lane with nothing to add is a
      // run of its own); a lane's run starts at the highest head at or below it.  At most 64 parts of <= 2^qbits quanta.
      const long long left = __shfl_up(cellno, 1, 64);
      const bool head = lane == 0 || left != cellno || cellno < 0;
      const unsigned long long heads = __ballot(head);
      if (~heads != 0ull) {                                               // some run is longer than one lane
        const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const long long ur = __shfl_up(fr, d, 64), ui = __shfl_up(fi, d, 64);
          if (lane - d >= start) {
            fr += ur;
            fi += ui;
          }
        }
      }
      const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
      if (last && cellno >= 0) {
        unsigned long long* cell = p.acc + 2 * cellno;
        atomicAdd(cell, (unsigned long long)fr);
        atomicAdd(cell + 1, (unsigned long long)fi);
      }
    }
  }
}

template <typename O>
__global__ __launch_bounds__(kCwtThreads) void cwt_tsst_readout_kernel(const CwtTScatDev<O> p) {
  const long long stride = (long long)gridDim.x * kCwtThreads;
  for (long long b = blockIdx.y; b < p.batch; b += gridDim.y) {
    double q, inv_q;
    cwt_tsst_quantum(p.emax[b], p.qbits, &q, &inv_q);
    const long long base = b * p.plane;
    for (long long i = (long long)blockIdx.x * kCwtThreads + threadIdx.x; i < p.plane; i += stride) {
      const unsigned long long* cell = p.acc + 2 * (base + i);
      p.Tx[base + i] = {(O)((double)(long long)cell[0] * q), (O)((double)(long long)cell[1] * q)};
    }
  }
}

// ---------------------------------------------------------------- host side ----
// the two halves of the pipeline (cwt_tsst.h), which cwt_tmsst.hip runs with its walk between them

int cwtt_check(const CwtMapsKind& k, const char* own_fail, const CwtTCall& c, CwtMapsShape* s) {
  const std::string pre = std::string(k.name) + ": ";
  const auto rows = [&]() -> int {
    if (!c.scales || !c.nu) SSQ_FAIL("NULL argument");
    for (int64_t i = 0; i < c.na; ++i) {
      if (!(c.scales[i] > 0) || !std::isfinite(c.scales[i])) SSQ_FAIL(pre + "scales must be positive and finite");
      if (!(c.nu[i] > 0) || !std::isfinite(c.nu[i])) SSQ_FAIL(pre + "row_freqs must be positive and finite");
    }
    return 0;
  };
  return cwt_maps_check(k, cwt_tsst_maps(c.order), own_fail, c, rows, nullptr, 0, nullptr, s);
}

int cwtt_tables(DeviceBufs& d, const CwtTCall& c, void** d_scales, void** d_nu) {
  SSQ_HIP(d.upload(d_scales, c.scales, sizeof(double) * (size_t)c.na));
  SSQ_HIP(d.upload(d_nu, c.nu, sizeof(double) * (size_t)c.na));
  return 0;
}

namespace {

template <typename T, int ORDER>
int cwtt_operator_order(const CwtTCall& c, const CwtMapsShape& s, const void* d_x, const void* d_scales, const void* d_nu,
                        void* d_Wx, void* d_tau, int* mm, void* d_work) {
  const int64_t N = c.N, na = c.na;
  const hipStream_t st = c.st;
  CwtTOpDev<T> op{};
  op.nu = static_cast<const double*>(d_nu);
  op.emax = cwt_head_at<unsigned long long>(d_work, s.head.emax);                                        // [batch]
  SSQ_HIP(hipMemsetAsync(op.emax, 0, (size_t)(s.head.planes - s.head.emax), st));   // the maxima and the accumulators
  op.P = s.P;
  op.N = N;
  op.n1 = s.n1;
  op.na = (int)na;
  op.inv_P = 1.0 / (double)s.P;
  op.gamma = s.gamma;
  op.gamma_sq = s.gamma * s.gamma;
  op.dt = c.dt;
  op.dt_o = (T)c.dt;
  const auto launch_op = [&](const cpx<double>* maps, int64_t r0, int64_t nr) -> int {
    op.maps = maps;
    op.Wx = static_cast<cpx<T>*>(d_Wx) + r0 * N;
    op.tau = d_tau ? static_cast<T*>(d_tau) + r0 * N : nullptr;
    op.mm = mm + r0 * N;
    op.r0 = r0;
    op.rows = nr;
    hipLaunchKernelGGL((cwt_tsst_operator_kernel<T, ORDER>), cwt_rows_grid(N, nr), dim3(kCwtThreads), 0, st, op);
    SSQ_HIP(hipGetLastError());
    return 0;
  };
  return cwt_maps_chunks<T, cwt_tsst_map_set(ORDER)>(c, s, d_x, d_scales, d_work, launch_op);
}

}  // namespace

template <typename T>
int cwtt_operator_run(const CwtTCall& c, const CwtMapsShape& s, const void* d_x, const void* d_scales, const void* d_nu,
                      void* d_Wx, void* d_tau, int* mm, void* d_work) {
  return c.order == 2 ? cwtt_operator_order<T, 2>(c, s, d_x, d_scales, d_nu, d_Wx, d_tau, mm, d_work)
                      : cwtt_operator_order<T, 1>(c, s, d_x, d_scales, d_nu, d_Wx, d_tau, mm, d_work);
}

template <typename T>
int cwtt_scatter_run(const CwtTCall& c, const CwtMapsShape& s, const void* d_nu, const void* d_Wx, const int* mm,
                     void* d_work, void* d_Tx, hipEvent_t mid) {
  const int64_t batch = c.batch, N = c.N;
  const hipStream_t st = c.st;
  int L = 0;
  while (((int64_t)1 << L) < N) ++L;                          // ceil(log2 N) <= 26
  CwtTScatDev<T> sc{};
  sc.Wx = static_cast<const cpx<T>*>(d_Wx);
  sc.mm = mm;
  sc.nu = static_cast<const double*>(d_nu);
  sc.emax = cwt_head_at<unsigned long long>(d_work, s.head.emax);
  sc.acc = cwt_head_at<unsigned long long>(d_work, s.head.acc);
  sc.Tx = static_cast<cpx<T>*>(d_Tx);
  sc.batch = batch;
  sc.plane = s.plane;
  sc.N = N;
  sc.qbits = std::min(kCwtTQuantumBitsMax, 61 - L);
  const dim3 grid((unsigned)std::min<int64_t>((s.plane + kCwtThreads - 1) / kCwtThreads, 0x7fffffffLL),
                  (unsigned)std::min<int64_t>(batch, 65535));
  hipLaunchKernelGGL((cwt_tsst_scatter_kernel<T>), grid, dim3(kCwtThreads), 0, st, sc);
  SSQ_HIP(hipGetLastError());
  if (mid) SSQ_HIP(hipEventRecord(mid, st));
  hipLaunchKernelGGL((cwt_tsst_readout_kernel<T>), grid, dim3(kCwtThreads), 0, st, sc);
  SSQ_HIP(hipGetLastError());
  return 0;
}

template int cwtt_operator_run<float>(const CwtTCall&, const CwtMapsShape&, const void*, const void*, const void*, void*,
                                      void*, int*, void*);
template int cwtt_operator_run<double>(const CwtTCall&, const CwtMapsShape&, const void*, const void*, const void*, void*,
                                       void*, int*, void*);
template int cwtt_scatter_run<float>(const CwtTCall&, const CwtMapsShape&, const void*, const void*, const int*, void*,
                                     void*, hipEvent_t);
template int cwtt_scatter_run<double>(const CwtTCall&, const CwtMapsShape&, const void*, const void*, const int*, void*,
                                      void*, hipEvent_t);

}  // namespace ssq

using namespace ssq;

namespace {

// the head: 16 bytes of accumulator and one int32 target per cell
constexpr CwtMapsKind kCwtTKind = {"tssq_cwt", "ssq_tssq_cwt_workspace_bytes", 20.0, 4.0e18, 0, 16, 1};

// tssq_cwt on device buffers (cwt_pipe_host, pipe_exec): the operator part, then the scatter with its read-out.  The
// targets go to the caller's plane if given, else to the head's.  kernel_ms: three parts, the events before and after
// the scatter kernel.
template <typename T>
struct CwtTPipe {
  static constexpr int kMid = 2;
  const CwtTCall& c;
  const CwtMapsShape& s;
  DeviceBufs d;
  void *scales, *nu, *work, *Tx, *Wx, *tau;
  int* mm;
  int tables() { return cwtt_tables(d, c, &scales, &nu); }
  int bind(int64_t, void* const* outs /* Tx, Wx, tau, mm */, void* wk) {
    work = wk;
    Tx = outs[0];
    Wx = outs[1];
    tau = outs[2];
    mm = outs[3] ? static_cast<int*>(outs[3]) : cwt_head_at<int>(work, s.head.planes);
    return 0;
  }
  int run(int64_t, const void* d_x, const hipEvent_t* mid) {
    if (int rc = cwtt_operator_run<T>(c, s, d_x, scales, nu, Wx, tau, mm, work)) return rc;
    if (mid[0]) SSQ_HIP(hipEventRecord(mid[0], c.st));
    return cwtt_scatter_run<T>(c, s, nu, Wx, mm, work, Tx, mid[1]);
  }
};

}  // namespace

extern "C" {

int64_t ssq_tssq_cwt_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int order, int64_t* min_bytes) {
  CwtMapsShape s;
  if (cwt_maps_shape(kCwtTKind, cwt_tsst_maps(order), cwtt_order_fail(order), dtype, batch, n_signal, na, &s)) return -1;
  if (min_bytes) *min_bytes = s.min_bytes;
  return s.pref_bytes;
}

int ssq_tssq_cwt_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                      const double* scales, const double* row_freqs, int64_t na, double dt, int padtype, int order,
                      double gamma, void* d_Tx, void* d_Wx, void* d_tau, void* d_mm, void* d_workspace,
                      int64_t workspace_bytes, void* stream, float* kernel_ms) {
  if (!d_x || !d_Tx || !d_Wx || !d_workspace) SSQ_FAIL("NULL argument");
  const CwtTCall c{{dtype, wavelet, padtype, batch, n_signal, na, p0, p1, dt, gamma, scales, (hipStream_t)stream},
                   order, row_freqs};
  CwtMapsShape s;
  if (int rc = cwtt_check(kCwtTKind, cwtt_order_fail(order), c, &s)) return rc;
  if (int rc = cwt_exec_bytes(kCwtTKind, &s, workspace_bytes)) return rc;
  if (int rc = require_device()) return rc;
  void* const outs[] = {d_Tx, d_Wx, d_tau, d_mm};
  float part[3], *ms = kernel_ms ? part : nullptr;
  const int rc = dtype == SSQ_F32 ? pipe_exec<CwtTPipe<float>>(c, s, d_x, outs, d_workspace, ms, &c.st)
                                  : pipe_exec<CwtTPipe<double>>(c, s, d_x, outs, d_workspace, ms, &c.st);
  if (rc == 0 && kernel_ms) {
    kernel_ms[0] = part[0] + part[1] + part[2];                // all the kernels
    kernel_ms[1] = part[1];                                    // the scatter kernel alone
    kernel_ms[2] = part[0];                                    // everything before the scatter
  }
  return rc;
}

int ssq_tssq_cwt_host(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                      const double* scales, const double* row_freqs, int64_t na, double dt, int padtype, int order,
                      double gamma, int64_t work_limit_bytes, void* Tx, void* Wx, void* tau, void* mm) {
  if (!x || !Tx || !Wx) SSQ_FAIL("NULL argument");
  const CwtTCall c{{dtype, wavelet, padtype, batch, n_signal, na, p0, p1, dt, gamma, scales, nullptr}, order, row_freqs};
  CwtMapsShape s;
  if (int rc = cwtt_check(kCwtTKind, cwtt_order_fail(order), c, &s)) return rc;
  if (int rc = cwt_host_bytes(kCwtTKind, &s, batch, work_limit_bytes)) return rc;
  if (int rc = require_device()) return rc;
  const size_t el = (dtype == SSQ_F32 ? 4 : 8) * (size_t)s.plane;
  const HostOut outs[] = {{Tx, 2 * el}, {Wx, 2 * el}, {tau, el}, {mm, sizeof(int32_t) * (size_t)s.plane}};
  return dtype == SSQ_F32 ? cwt_pipe_host<CwtTPipe<float>>(c, s, x, outs) : cwt_pipe_host<CwtTPipe<double>>(c, s, x, outs);
}

}  // extern "C"
