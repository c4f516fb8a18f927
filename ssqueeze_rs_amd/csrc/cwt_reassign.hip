// cwt_reassign.hip -- the reassigned scalogram, `upstream.reassign_cwt` (Auger and Flandrin 1995, III).
// Upstream has no such transform: the definition is the project's own, restated in numpy by
// tests/helpers/reassign_cwt_ref.py.  Every coefficient's energy |Wx|^2 moves in BOTH directions at once, to its
// instantaneous frequency (ssq_cwt's first-order operator) and its group delay.  Per-sample units, dt enters at the end.
// With P, n1, n2 = p2up(N), xh, xi_k, T0 and T1 exactly those of cwt_sst2.hip:
//   W = F^-1[xh T0]     W1 = F^-1[xh i xi T0]     Wt = F^-1[xh (-i) T1]           columns n1 .. n1 + N - 1
//   w   = |Im(W1/W)| / (2 pi dt)            fp64, rounded once to the call's dtype; +inf where |W| < gamma
//   tau = clamp(Re(Wt/W), -N, N) dt         fp64, rounded once to the call's dtype; +inf where |W| < gamma
//   k'  = ssqueeze.hip's bin rule on the reported w, in its dtype (then flipped, as ssq_cwt2 flips)
//   m'  = clip(j + rint(tau / dt), 0, N - 1) in the call's dtype
//   Rx[k', m'] += |Wx[i, j]|^2              of the REPORTED Wx, formed in fp64; no row weights
//
//   cwt_pad_kernel (cwt_pad.h), cwt_reassign_spectra_kernel : cwt_sst2.hip's first two steps, the second with three
//                              product spectra a row instead of five; the transforms between them are
//                              fft_any_batched's.
//   cwt_reassign_operator_kernel : one thread per (row, column), lanes along time: the three values, 1 / P, 1 / |W|^2
//                              once; Wx, optionally w and tau, and the two int32 targets (k', m'; -1 where the bin is
//                              not kept), formed from the values AS ROUNDED to the call's dtype.  It also reduces
//                              max |Wx|^2 per signal: a wave reduction, a four-value step through LDS, then ONE 64-bit
//                              integer atomic max per workgroup on the bit pattern of the non-negative double.
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
// Transforms and operator run in fp64 for float32 calls too (the decision of DESIGN 4.11 and 4.12, taken over).  A row is
// transformed on its own by every kernel, so its result depends neither on the chunk it is in nor on the batch.
#include <cmath>
#include <vector>

#include "../../include/ssq_hip.h"
#include "bin_rule.h"
#include "cwt_pad.h"
#include "cwt_sst2_wavelets.h"
#include "dev_buffers.h"
#include "fft_generic.h"
#include "host_math.h"

namespace ssq {

constexpr int kCwtRThreads = 256;
constexpr int kCwtRMaps = 3;                                  // W, W1, Wt
constexpr int kCwtRQuantumBitsMax = 38;                       // upstream.REASSIGN_CWT_QUANTUM_LOG2_MAX

struct CwtRSpecDev {
  const cpx<double>* xh;     // [batch][P]: the forward DFTs
  const double* scales;      // [na]
  cpx<double>* spec;         // [rows][3][P]: the chunk's product spectra (then, in place, their inverse transforms)
  long long P, r0, rows;     // the chunk: rows r0 .. r0 + rows - 1 of the batch x na
  int na;
  Cwt2Wavelet wv;
};

// grid (ceil(P / 256), min(rows, 65535)): thread k of row r0 + rl
__global__ __launch_bounds__(kCwtRThreads) void cwt_reassign_spectra_kernel(const CwtRSpecDev p) {
  const long long k = (long long)blockIdx.x * kCwtRThreads + threadIdx.x;
  if (k >= p.P) return;
  const bool live = 2 * k <= p.P;
  for (long long rl = blockIdx.y; rl < p.rows; rl += gridDim.y) {
    const long long r = p.r0 + rl;
    const long long b = r / p.na;
    const double a = p.scales[r - b * p.na];
    cpx<double>* __restrict__ out = p.spec + rl * kCwtRMaps * p.P + k;
    cpx<double> s0 = {0.0, 0.0}, s1 = s0, s3 = s0;
    if (live) {
      double xi, T0, T1;
      cwt2_tables_at(p.wv, a, k, p.P, &xi, &T0, &T1);
      const cpx<double> X = p.xh[b * p.P + k];
      const double xT0 = xi * T0;
      s0 = {X.x * T0, X.y * T0};
      s1 = {-X.y * xT0, X.x * xT0};                           // X i xi T0
      s3 = {X.y * T1, -X.x * T1};                             // X (-i) T1
    }
    out[0] = s0;
    out[p.P] = s1;
    out[2 * p.P] = s3;
  }
}

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

// max over the workgroup of a non-negative value, then one integer atomic max on its bit pattern (non-negative doubles
// order as their bit patterns do; max is order-independent).  Called by every thread of the workgroup.
__device__ __forceinline__ void cwt_reassign_flush_max(double mx, double* red, unsigned long long* dst) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) mx = fmax(mx, __shfl_xor(mx, s, 64));
  __syncthreads();                                           // (the previous flush's reads of `red` are over)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = red[0];
#pragma unroll
    for (int i = 1; i < kCwtRThreads / 64; ++i) v = fmax(v, red[i]);
    if (v > 0.0) atomicMax(dst, (unsigned long long)__double_as_longlong(v));
  }
}

// grid (ceil(N / 256), min(rows, 65535)): thread = column j of row rl.  No thread leaves early: the maximum's reduction
// has workgroup barriers, and the signal a row belongs to is the same for the whole workgroup.
template <typename O>
__global__ __launch_bounds__(kCwtRThreads) void cwt_reassign_operator_kernel(const CwtROpDev<O> p) {
  using T = double;
  __shared__ T red[kCwtRThreads / 64];
  const long long j = (long long)blockIdx.x * kCwtRThreads + threadIdx.x;
  const bool live = j < p.N;
  T mx = (T)0;
  long long b_cur = -1;
  for (long long rl = blockIdx.y; rl < p.rows; rl += gridDim.y) {
    const long long b = (p.r0 + rl) / p.na;
    if (b != b_cur) {
      if (b_cur >= 0) cwt_reassign_flush_max(mx, red, p.emax + b_cur);
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
      // the time rule on the reported tau.  |tau / dt| <= N (1 + eps), the offset being clamped; the bound below only
      // keeps the quotient of an extreme dt inside the integer
      const O vt = tau / p.dt_o;
      const O rv = isfinite(vt) ? rint(vt) : (O)0;
      const long long r = (long long)(rv < (O)-134217728 ? (O)-134217728 : (rv > (O)134217728 ? (O)134217728 : rv));
      long long mt = j + r;
      mt = mt < 0 ? 0 : (mt > p.N - 1 ? p.N - 1 : mt);
      mm = (int)mt;
      if (kk < 0) mm = -1;                                                    // (an infinite quotient: not a target)
    }
    const long long o = rl * p.N + j;
    p.Wx[o] = Wo;
    if (p.w) p.w[o] = kk < 0 ? (O)INFINITY : w;
    if (p.tau) p.tau[o] = kk < 0 ? (O)INFINITY : tau;
    p.kk[o] = kk;
    p.mm[o] = mm;
    mx = fmax(mx, energy_f64<O>(Wo));                                // (a NaN is not a maximum)
  }
  if (b_cur >= 0) cwt_reassign_flush_max(mx, red, p.emax + b_cur);
}

// the signal's scale: Pmax = the smallest power of two >= max |Wx|^2, quantum q = Pmax 2^-qbits (exponent clamped so
// that both q and 1 / q are normal numbers; a signal of zeros, or one whose energy is not finite, gets q = 0)
__device__ __forceinline__ void cwt_reassign_quantum(unsigned long long bits, int qbits, double* q, double* inv_q) {
  const double mx = __longlong_as_double((long long)bits);
  *q = 0.0;
  *inv_q = 0.0;
  if (mx > 0.0 && mx <= 1.7976931348623157e308) {
    int ex;
    const double fr = frexp(mx, &ex);                                    // mx = fr 2^ex, fr in [0.5, 1)
    int lp = fr == 0.5 ? ex - 1 : ex;
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
__global__ __launch_bounds__(kCwtRThreads) void cwt_reassign_scatter_kernel(const CwtRScatDev<O> p) {
  const long long stride = (long long)gridDim.x * kCwtRThreads;
  const double cap = ldexp(1.0, p.qbits);
  for (long long b = blockIdx.y; b < p.batch; b += gridDim.y) {
    double q, inv_q;
    cwt_reassign_quantum(p.emax[b], p.qbits, &q, &inv_q);
    if (q == 0.0) continue;
    const long long base = b * p.plane;
    for (long long i = (long long)blockIdx.x * kCwtRThreads + threadIdx.x; i < p.plane; i += stride) {
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
__global__ __launch_bounds__(kCwtRThreads) void cwt_reassign_readout_kernel(const CwtRScatDev<O> p) {
  const long long stride = (long long)gridDim.x * kCwtRThreads;
  for (long long b = blockIdx.y; b < p.batch; b += gridDim.y) {
    double q, inv_q;
    cwt_reassign_quantum(p.emax[b], p.qbits, &q, &inv_q);
    const long long base = b * p.plane;
    for (long long i = (long long)blockIdx.x * kCwtRThreads + threadIdx.x; i < p.plane; i += stride)
      p.Rx[base + i] = (O)((double)(long long)p.acc[base + i] * q);
  }
}

}  // namespace ssq

using namespace ssq;

namespace {

constexpr int64_t kCwtRDefaultWorkBytes = (int64_t)2 << 30;   // the chunk area of the preferred workspace is capped here

struct CwtRShape {
  int64_t P = 0, n1 = 0, n2 = 0, rows = 0, plane = 0;
  int qbits = 0;
  double gamma = 0.0;
  int64_t fixed_bytes = 0, min_bytes = 0, pref_bytes = 0;
};

// workspace: first what does not depend on R -- the signals' maxima [batch] (to a multiple of 16 bytes), the accumulators
// [batch][na][N] and the two int32 target maps [batch][na][N] -- then xh [batch][P] and a chunk area of R rows ([R][3][P]
// spectra and as much again for the transforms' ping-pong)
int64_t cwtr_chunk_bytes(int64_t batch, int64_t P, int64_t R) { return 16 * P * (batch + 2 * kCwtRMaps * R); }
int64_t cwtr_emax_bytes(int64_t batch) { return (8 * batch + 15) / 16 * 16; }
int64_t cwtr_fixed_bytes(int64_t batch, int64_t plane) { return cwtr_emax_bytes(batch) + 16 * batch * plane; }

int cwtr_shape_only(int dtype, int64_t batch, int64_t N, int64_t na, CwtRShape* s) {
  if (dtype != SSQ_F32 && dtype != SSQ_F64) SSQ_FAIL("dtype must be SSQ_F32 or SSQ_F64");
  if (batch < 1) SSQ_FAIL("batch must be >= 1");
  if (N < 2 || N > ((int64_t)1 << 26)) SSQ_FAIL("reassign_cwt: n_signal must be in [2, 2^26]");
  if (na < 2 || na > 32767) SSQ_FAIL("reassign_cwt: na must be in [2, 32767]");
  if (na * N > ((int64_t)1 << 40)) SSQ_FAIL("reassign_cwt: na * n_signal must be <= 2^40");
  host::p2up(N, &s->P, &s->n1, &s->n2);
  if (s->P < N || (s->P & (s->P - 1)) != 0) SSQ_FAIL("reassign_cwt: bad padded length");
  if ((double)batch * (double)na * (double)N * 16.0 > 4.0e18 || (double)batch * (double)s->P * 16.0 > 4.0e18)
    SSQ_FAIL("reassign_cwt: transform too large");
  s->rows = batch * na;
  s->plane = na * N;
  int L = 0;
  while (((int64_t)1 << L) < s->plane) ++L;                   // ceil(log2(na N)) <= 40
  s->qbits = std::min(kCwtRQuantumBitsMax, 62 - L);
  s->fixed_bytes = cwtr_fixed_bytes(batch, s->plane);
  s->min_bytes = cwtr_chunk_bytes(batch, s->P, 1) + s->fixed_bytes;
  int64_t R = (kCwtRDefaultWorkBytes - 16 * s->P * batch) / (16 * s->P * 2 * kCwtRMaps);
  if (R > s->rows) R = s->rows;
  if (R < 1) R = 1;
  s->pref_bytes = cwtr_chunk_bytes(batch, s->P, R) + s->fixed_bytes;
  return 0;
}

// every argument check of the entry points (sets the error and returns non-zero): nothing here touches the GPU
int cwtr_check(int dtype, int64_t batch, int64_t N, int wavelet, double p0, double p1, const double* scales, int64_t na,
               double dt, const double* f_asc, int freq_kind, int64_t freq_transition, int padtype, double gamma,
               CwtRShape* s) {
  if (int rc = cwtr_shape_only(dtype, batch, N, na, s)) return rc;
  if (wavelet != SSQ_WAVELET_GMW && wavelet != SSQ_WAVELET_MORLET) SSQ_FAIL("reassign_cwt: unknown wavelet");
  if (!(p0 > 0) || !std::isfinite(p0)) SSQ_FAIL("reassign_cwt: wavelet parameter p0 must be positive");
  if (wavelet == SSQ_WAVELET_GMW && (!(p1 > 0) || !std::isfinite(p1)))
    SSQ_FAIL("reassign_cwt: wavelet parameter p1 must be positive");
  if (!scales || !f_asc) SSQ_FAIL("NULL argument");
  for (int64_t i = 0; i < na; ++i) {
    if (!(scales[i] > 0) || !std::isfinite(scales[i])) SSQ_FAIL("reassign_cwt: scales must be positive and finite");
    if (!std::isfinite(f_asc[i])) SSQ_FAIL("reassign_cwt: ssq_freqs_asc must be finite");
  }
  if (!(dt > 0) || !std::isfinite(dt)) SSQ_FAIL("reassign_cwt: dt must be positive");
  if (freq_kind != SSQ_FREQS_LOG && freq_kind != SSQ_FREQS_LINEAR && freq_kind != SSQ_FREQS_LOG_PIECEWISE)
    SSQ_FAIL("reassign_cwt: freq_kind must be SSQ_FREQS_LOG, _LINEAR or _LOG_PIECEWISE");
  if (freq_kind == SSQ_FREQS_LOG_PIECEWISE && (freq_transition < 2 || freq_transition > na - 1))
    SSQ_FAIL("reassign_cwt: freq_transition must be 2 .. na-1 for SSQ_FREQS_LOG_PIECEWISE");
  if (padtype < SSQ_PAD_REFLECT || padtype > SSQ_PAD_WRAP) SSQ_FAIL("reassign_cwt: unknown padtype");
  if (std::isnan(gamma)) SSQ_FAIL("reassign_cwt: gamma is NaN");
  s->gamma = gamma < 0 ? 10.0 * (dtype == SSQ_F64 ? 2.2204460492503131e-16 : 1.1920928955078125e-07) : gamma;
  return 0;
}

struct CwtRCall {
  int dtype, wavelet, freq_kind, padtype, variant;
  int64_t batch, N, na, freq_transition;
  double p0, p1, dt;
  const double *scales, *f_asc;
};

// The whole transform on device buffers; `work_bytes` >= s.min_bytes sets the rows per chunk.  d_w, d_tau, d_kk, d_mm may
// be nullptr (the targets then live in the workspace alone).  Synchronous.  kernel_ms: two floats, all kernels and the
// scatter kernel alone.
template <typename T>
int cwtr_run(const CwtRCall& c, const CwtRShape& s, const void* d_x, void* d_Rx, void* d_Wx, void* d_w, void* d_tau,
             void* d_kk, void* d_mm, void* d_work, int64_t work_bytes, hipStream_t st, float* kernel_ms) {
  HostCallBufs d;
  TimingEvents t;
  void* d_scales = nullptr;
  SSQ_HIP(d.upload(&d_scales, c.scales, sizeof(double) * (size_t)c.na));
  if (kernel_ms) SSQ_HIP(t.start(4, st));
  const int64_t P = s.P;
  int64_t R = (work_bytes - s.fixed_bytes - 16 * P * c.batch) / (16 * P * 2 * kCwtRMaps);
  if (R > s.rows) R = s.rows;
  char* head = static_cast<char*>(d_work);
  unsigned long long* emax = reinterpret_cast<unsigned long long*>(head);                                  // [batch]
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(head + cwtr_emax_bytes(c.batch));       // [batch][na][N]
  int* kk = d_kk ? static_cast<int*>(d_kk) : reinterpret_cast<int*>(acc + c.batch * s.plane);
  int* mm = d_mm ? static_cast<int*>(d_mm) : reinterpret_cast<int*>(acc + c.batch * s.plane) + c.batch * s.plane;
  cpx<double>* xh = reinterpret_cast<cpx<double>*>(head + s.fixed_bytes);
  cpx<double>* spec = xh + c.batch * P;                        // [R][3][P]
  cpx<double>* pong = spec + R * kCwtRMaps * P;                // [R][3][P]
  SSQ_HIP(hipMemsetAsync(head, 0, (size_t)(cwtr_emax_bytes(c.batch) + 8 * c.batch * s.plane), st));
  SSQ_HIP(cwt_pad<T>(static_cast<const T*>(d_x), xh, c.batch, c.N, P, s.n1, c.padtype, st));
  const int64_t fb = 2 * kCwtRMaps * R;                        // signals per forward call: the chunk area is its ping-pong
  for (int64_t b0 = 0; b0 < c.batch; b0 += fb)
    SSQ_HIP(fft_any_batched<double>(xh + b0 * P, spec, P, std::min<int64_t>(fb, c.batch - b0), -1, st));
  CwtRSpecDev sp{};
  sp.xh = xh;
  sp.scales = static_cast<const double*>(d_scales);
  sp.spec = spec;
  sp.P = P;
  sp.na = (int)c.na;
  sp.wv = cwt2_wavelet(c.wavelet, c.p0, c.p1);
  CwtROpDev<T> op{};
  op.maps = spec;
  op.emax = emax;
  op.P = P;
  op.N = c.N;
  op.n1 = s.n1;
  op.na = (int)c.na;
  op.inv_P = 1.0 / (double)P;
  op.gamma = s.gamma;
  op.inv_two_pi_dt = 1.0 / (6.283185307179586 * c.dt);
  op.dt = c.dt;
  op.dt_o = (T)c.dt;
  if (int rc = bin_rule<T>(c.f_asc, c.na, c.freq_kind, c.freq_transition, (c.variant & SSQ_VARIANT_FLIPUD) ? 1 : 0, op.rule))
    return rc;                                                 // (cwtr_check has made each of its checks already)
  for (int64_t r0 = 0; r0 < s.rows; r0 += R) {
    const int64_t nr = std::min<int64_t>(R, s.rows - r0);
    sp.r0 = r0;
    sp.rows = nr;
    hipLaunchKernelGGL(cwt_reassign_spectra_kernel, cwt_rows_grid(P, nr), dim3(kCwtRThreads), 0, st, sp);
    SSQ_HIP(hipGetLastError());
    SSQ_HIP(fft_any_batched<double>(spec, pong, P, kCwtRMaps * nr, +1, st));
    op.Wx = static_cast<cpx<T>*>(d_Wx) + r0 * c.N;
    op.w = d_w ? static_cast<T*>(d_w) + r0 * c.N : nullptr;
    op.tau = d_tau ? static_cast<T*>(d_tau) + r0 * c.N : nullptr;
    op.kk = kk + r0 * c.N;
    op.mm = mm + r0 * c.N;
    op.r0 = r0;
    op.rows = nr;
    hipLaunchKernelGGL((cwt_reassign_operator_kernel<T>), cwt_rows_grid(c.N, nr), dim3(kCwtRThreads), 0, st, op);
    SSQ_HIP(hipGetLastError());
  }
  CwtRScatDev<T> sc{};
  sc.Wx = static_cast<const cpx<T>*>(d_Wx);
  sc.kk = kk;
  sc.mm = mm;
  sc.emax = emax;
  sc.acc = acc;
  sc.Rx = static_cast<T*>(d_Rx);
  sc.batch = c.batch;
  sc.plane = s.plane;
  sc.N = c.N;
  sc.na = (int)c.na;
  sc.qbits = s.qbits;
  const dim3 grid((unsigned)std::min<int64_t>((s.plane + kCwtRThreads - 1) / kCwtRThreads, 0x7fffffffLL),
                  (unsigned)std::min<int64_t>(c.batch, 65535));
  if (kernel_ms) SSQ_HIP(hipEventRecord(t.ev[1], st));
  hipLaunchKernelGGL((cwt_reassign_scatter_kernel<T>), grid, dim3(kCwtRThreads), 0, st, sc);
  SSQ_HIP(hipGetLastError());
  if (kernel_ms) SSQ_HIP(hipEventRecord(t.ev[2], st));
  hipLaunchKernelGGL((cwt_reassign_readout_kernel<T>), grid, dim3(kCwtRThreads), 0, st, sc);
  SSQ_HIP(hipGetLastError());
  if (kernel_ms) {
    SSQ_HIP(hipEventRecord(t.ev[3], st));
    SSQ_HIP(hipEventSynchronize(t.ev[3]));
    SSQ_HIP(hipEventElapsedTime(&kernel_ms[0], t.ev[0], t.ev[3]));
    SSQ_HIP(hipEventElapsedTime(&kernel_ms[1], t.ev[1], t.ev[2]));
  }
  SSQ_HIP(hipStreamSynchronize(st));                           // (the scales above are freed on return)
  return 0;
}

template <typename T>
int cwtr_host_typed(const CwtRCall& c, const CwtRShape& s, const void* x, int64_t work_bytes, void* Rx, void* Wx, void* w,
                    void* tau, void* kk, void* mm) {
  HostCallBufs d;
  const size_t n = (size_t)s.rows * (size_t)c.N;
  void *d_x, *d_Rx, *d_Wx, *d_work, *d_w = nullptr, *d_tau = nullptr;
  SSQ_HIP(d.upload(&d_x, x, sizeof(T) * (size_t)c.batch * (size_t)c.N));
  SSQ_HIP(d.alloc(&d_Rx, sizeof(T) * n));
  SSQ_HIP(d.alloc(&d_Wx, sizeof(cpx<T>) * n));
  if (w) SSQ_HIP(d.alloc(&d_w, sizeof(T) * n));
  if (tau) SSQ_HIP(d.alloc(&d_tau, sizeof(T) * n));
  SSQ_HIP(d.alloc(&d_work, (size_t)work_bytes));
  if (int rc = cwtr_run<T>(c, s, d_x, d_Rx, d_Wx, d_w, d_tau, nullptr, nullptr, d_work, work_bytes, nullptr, nullptr))
    return rc;
  SSQ_HIP(hipMemcpy(Rx, d_Rx, sizeof(T) * n, hipMemcpyDeviceToHost));
  SSQ_HIP(hipMemcpy(Wx, d_Wx, sizeof(cpx<T>) * n, hipMemcpyDeviceToHost));
  if (w) SSQ_HIP(hipMemcpy(w, d_w, sizeof(T) * n, hipMemcpyDeviceToHost));
  if (tau) SSQ_HIP(hipMemcpy(tau, d_tau, sizeof(T) * n, hipMemcpyDeviceToHost));
  // the targets of the workspace: behind the maxima and the accumulators at its head
  const char* tgt = static_cast<const char*>(d_work) + cwtr_emax_bytes(c.batch) + 8 * n;
  if (kk) SSQ_HIP(hipMemcpy(kk, tgt, sizeof(int) * n, hipMemcpyDeviceToHost));
  if (mm) SSQ_HIP(hipMemcpy(mm, tgt + sizeof(int) * n, sizeof(int) * n, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

extern "C" {

int64_t ssq_reassign_cwt_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int64_t* min_bytes) {
  CwtRShape s;
  if (cwtr_shape_only(dtype, batch, n_signal, na, &s)) return -1;
  if (min_bytes) *min_bytes = s.min_bytes;
  return s.pref_bytes;
}

int ssq_reassign_cwt_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                          const double* scales, int64_t na, double dt, const double* ssq_freqs_asc, int freq_kind,
                          int64_t freq_transition, int padtype, double gamma, int variant, void* d_Rx, void* d_Wx,
                          void* d_w, void* d_tau, void* d_kk, void* d_mm, void* d_workspace, int64_t workspace_bytes,
                          void* stream, float* kernel_ms) {
  if (!d_x || !d_Rx || !d_Wx || !d_workspace) SSQ_FAIL("NULL argument");
  CwtRShape s;
  if (int rc = cwtr_check(dtype, batch, n_signal, wavelet, p0, p1, scales, na, dt, ssq_freqs_asc, freq_kind, freq_transition,
                          padtype, gamma, &s))
    return rc;
  if (workspace_bytes < s.min_bytes)
    SSQ_FAIL("reassign_cwt: workspace smaller than the min_bytes of ssq_reassign_cwt_workspace_bytes");
  if (int rc = require_device()) return rc;
  const CwtRCall c{dtype, wavelet, freq_kind, padtype, variant, batch, n_signal, na, freq_transition,
                   p0,    p1,      dt,        scales,  ssq_freqs_asc};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dtype == SSQ_F32 ? cwtr_run<float>(c, s, d_x, d_Rx, d_Wx, d_w, d_tau, d_kk, d_mm, d_workspace, workspace_bytes, st,
                                            kernel_ms)
                          : cwtr_run<double>(c, s, d_x, d_Rx, d_Wx, d_w, d_tau, d_kk, d_mm, d_workspace, workspace_bytes, st,
                                             kernel_ms);
}

int ssq_reassign_cwt_host(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                          const double* scales, int64_t na, double dt, const double* ssq_freqs_asc, int freq_kind,
                          int64_t freq_transition, int padtype, double gamma, int variant, int64_t work_limit_bytes,
                          void* Rx, void* Wx, void* w, void* tau, void* kk, void* mm) {
  if (!x || !Rx || !Wx) SSQ_FAIL("NULL argument");
  CwtRShape s;
  if (int rc = cwtr_check(dtype, batch, n_signal, wavelet, p0, p1, scales, na, dt, ssq_freqs_asc, freq_kind, freq_transition,
                          padtype, gamma, &s))
    return rc;
  if (work_limit_bytes < 0 || (work_limit_bytes > 0 && work_limit_bytes < s.min_bytes))
    SSQ_FAIL("reassign_cwt: work_limit_bytes below the min_bytes of ssq_reassign_cwt_workspace_bytes");
  if (int rc = require_device()) return rc;
  const int64_t work = work_limit_bytes > 0
                           ? std::min(work_limit_bytes, cwtr_chunk_bytes(batch, s.P, s.rows) + s.fixed_bytes)
                           : s.pref_bytes;
  const CwtRCall c{dtype, wavelet, freq_kind, padtype, variant, batch, n_signal, na, freq_transition,
                   p0,    p1,      dt,        scales,  ssq_freqs_asc};
  return dtype == SSQ_F32 ? cwtr_host_typed<float>(c, s, x, work, Rx, Wx, w, tau, kk, mm)
                          : cwtr_host_typed<double>(c, s, x, work, Rx, Wx, w, tau, kk, mm);
}

}  // extern "C"
