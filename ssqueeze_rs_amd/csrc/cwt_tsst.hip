// cwt_tsst.hip -- the time-reassigned synchrosqueezed CWT, `upstream.tssq_cwt`.  Upstream has no such
// transform: the definition is the project's own, restated in numpy by tests/helpers/tssq_cwt_ref.py.  Every complex
// coefficient moves along TIME inside its own row, to its group delay, and is rotated to keep its phase reference; rows do
// not mix.  Per-sample units, dt enters at the end.  With P, n1, n2 = p2up(N), xh, xi_k, T0 and T1 exactly those of
// cwt_sst2.hip, on columns n1 .. n1 + N - 1:
//   W = F^-1[xh T0]   W1 = F^-1[xh i xi T0]   W2 = F^-1[xh (-xi^2) T0]   Wt = F^-1[xh (-i) T1]   Wt1 = F^-1[xh xi T1]
//   nu_i = wc / (2 pi a_i) cycles/sample: the row's frequency, an argument [na] (the library never derives it)
//   d1  = Re(Wt / W)
//   D   = W^2 + Wt1 W - Wt W1      num = W2 W - W1^2
//   d2  = d1 - Im((D / num) (2 pi nu_i + i W1 / W))        the group delay of the locally fitted log-quadratic spectrum
//   off = d2 where order = 2, |num| > gamma^2, d2 is finite and |d2| <= N, else d1; clamped to [-N, N] (a NaN stays)
//   tau = off dt, fp64 rounded once to the call's dtype; +inf where |W| < gamma
//   m'  = clip(j + rint(tau / dt), 0, N - 1) in the call's dtype, on the REPORTED tau (cwt_reassign.hip's time rule)
//   Tx[i, m'] += Wx[i, j] exp(-2 pi i frac(nu_i (j - m')))  of the REPORTED Wx, the product in fp64
//
//   cwt_pad_kernel (cwt_pad.h), cwt_tsst_spectra_kernel<ORDER> : cwt_sst2.hip's first two steps; order 1 forms two product
//                              spectra a row (W, Wt), order 2 the five.  The transforms between them are fft_any_batched's.
//   cwt_tsst_operator_kernel<O, ORDER> : one thread per (row, column), lanes along time: the values, 1 / P, 1 / |W|^2 and
//                              1 / |num|^2 once; Wx, optionally tau, and the int32 target m' (-1 where the bin is not
//                              kept), formed from the values AS ROUNDED to the call's dtype.  It also reduces max |Wx|^2
//                              per signal as cwt_reassign.hip does: a wave reduction, a four-value step through LDS, then
//                              ONE 64-bit integer atomic max per workgroup on the bit pattern of the non-negative double.
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
// The rotation's angle is formed in turns: t = nu r with the product's rounding error recovered by an fma, then
// t - rint(t) (exact) plus that remainder, and sinpi / cospi: its error does not grow with |r| <= N.
// Transforms and operator run in fp64 for float32 calls too (the decision of DESIGN 4.11 and 4.12, taken over).  A row is
// transformed on its own by every kernel, so its result depends neither on the chunk it is in nor on the batch.
#include <cmath>
#include <vector>

#include "../../include/ssq_hip.h"
#include "cwt_pad.h"
#include "cwt_sst2_wavelets.h"
#include "dev_buffers.h"
#include "fft_generic.h"
#include "host_math.h"

namespace ssq {

constexpr int kCwtTThreads = 256;
constexpr int kCwtTQuantumBitsMax = 38;                       // upstream.TSSQ_CWT_QUANTUM_LOG2_MAX

constexpr int cwt_tsst_maps(int order) { return order == 2 ? 5 : 2; }   // W, Wt | W, W1, W2, Wt, Wt1

struct CwtTSpecDev {
  const cpx<double>* xh;     // [batch][P]: the forward DFTs
  const double* scales;      // [na]
  cpx<double>* spec;         // [rows][maps][P]: the chunk's product spectra (then, in place, their inverse transforms)
  long long P, r0, rows;     // the chunk: rows r0 .. r0 + rows - 1 of the batch x na
  int na;
  Cwt2Wavelet wv;
};

// grid (ceil(P / 256), min(rows, 65535)): thread k of row r0 + rl
template <int ORDER>
__global__ __launch_bounds__(kCwtTThreads) void cwt_tsst_spectra_kernel(const CwtTSpecDev p) {
  constexpr int M = cwt_tsst_maps(ORDER);
  const long long k = (long long)blockIdx.x * kCwtTThreads + threadIdx.x;
  if (k >= p.P) return;
  const bool live = 2 * k <= p.P;
  for (long long rl = blockIdx.y; rl < p.rows; rl += gridDim.y) {
    const long long r = p.r0 + rl;
    const long long b = r / p.na;
    const double a = p.scales[r - b * p.na];
    cpx<double>* __restrict__ out = p.spec + rl * M * p.P + k;
    cpx<double> s0 = {0.0, 0.0}, s1 = s0, s2 = s0, s3 = s0, s4 = s0;
    if (live) {
      double xi, T0, T1;
      cwt2_tables_at(p.wv, a, k, p.P, &xi, &T0, &T1);
      const cpx<double> X = p.xh[b * p.P + k];
      s0 = {X.x * T0, X.y * T0};
      s3 = {X.y * T1, -X.x * T1};                             // X (-i) T1
      if constexpr (ORDER == 2) {
        const double xT0 = xi * T0;
        s1 = {-X.y * xT0, X.x * xT0};                         // X i xi T0
        s2 = {-X.x * (xi * xT0), -X.y * (xi * xT0)};          // X (-xi^2) T0
        s4 = {X.x * (xi * T1), X.y * (xi * T1)};              // X xi T1
      }
    }
    if constexpr (ORDER == 2) {
      out[0] = s0;
      out[p.P] = s1;
      out[2 * p.P] = s2;
      out[3 * p.P] = s3;
      out[4 * p.P] = s4;
    } else {
      out[0] = s0;
      out[p.P] = s3;
    }
  }
}

template <typename O>
struct CwtTOpDev {
  const cpx<double>* maps;   // [rows][maps][P]: the unnormalised inverse transforms
  const double* nu;          // [na]: the rows' frequencies, cycles/sample
  cpx<O>* Wx;                // [batch * na][N], these three at the chunk's first row
  O* tau;                    // or nullptr
  int* mm;
  unsigned long long* emax;  // [batch]: bit pattern of max |Wx|^2, zeroed before the first chunk
  long long P, N, n1, r0, rows;
  int na;
  double inv_P, gamma, gamma_sq, dt;
  O dt_o;                    // dt in the call's dtype: the time rule runs on the tau the call reports
};

// max over the workgroup of a non-negative value, then one integer atomic max on its bit pattern (non-negative doubles
// order as their bit patterns do; max is order-independent).  Called by every thread of the workgroup.
__device__ __forceinline__ void cwt_tsst_flush_max(double mx, double* red, unsigned long long* dst) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) mx = fmax(mx, __shfl_xor(mx, s, 64));
  __syncthreads();                                           // (the previous flush's reads of `red` are over)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = red[0];
#pragma unroll
    for (int i = 1; i < kCwtTThreads / 64; ++i) v = fmax(v, red[i]);
    if (v > 0.0) atomicMax(dst, (unsigned long long)__double_as_longlong(v));
  }
}

// grid (ceil(N / 256), min(rows, 65535)): thread = column j of row rl.  No thread leaves early: the maximum's reduction
// has workgroup barriers, and the signal a row belongs to is the same for the whole workgroup.
template <typename O, int ORDER>
__global__ __launch_bounds__(kCwtTThreads) void cwt_tsst_operator_kernel(const CwtTOpDev<O> p) {
  using T = double;
  constexpr int M = cwt_tsst_maps(ORDER);
  __shared__ T red[kCwtTThreads / 64];
  const long long j = (long long)blockIdx.x * kCwtTThreads + threadIdx.x;
  const bool live = j < p.N;
  T mx = (T)0;
  long long b_cur = -1;
  for (long long rl = blockIdx.y; rl < p.rows; rl += gridDim.y) {
    const long long b = (p.r0 + rl) / p.na;
    if (b != b_cur) {
      if (b_cur >= 0) cwt_tsst_flush_max(mx, red, p.emax + b_cur);
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
        // the time rule on the reported tau.  |tau / dt| <= N (1 + eps), the offset being clamped; the bound below only
        // keeps the quotient of an extreme dt inside the integer
        const O vt = tau / p.dt_o;
        const O rv = isfinite(vt) ? rint(vt) : (O)0;
        const long long r = (long long)(rv < (O)-134217728 ? (O)-134217728 : (rv > (O)134217728 ? (O)134217728 : rv));
        long long mt = j + r;
        mt = mt < 0 ? 0 : (mt > p.N - 1 ? p.N - 1 : mt);
        mm = (int)mt;
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
  if (b_cur >= 0) cwt_tsst_flush_max(mx, red, p.emax + b_cur);
}

// the signal's scale: Pmax = the smallest power of two >= max |Wx|^2, A = the smallest power of two >= sqrt(Pmax), quantum
// q = A 2^-qbits (both q and 1 / q normal numbers; a signal of zeros, or one whose energy is not finite, gets q = 0)
__device__ __forceinline__ void cwt_tsst_quantum(unsigned long long bits, int qbits, double* q, double* inv_q) {
  const double mx = __longlong_as_double((long long)bits);
  *q = 0.0;
  *inv_q = 0.0;
  if (mx > 0.0 && mx <= 1.7976931348623157e308) {
    int ex;
    const double fr = frexp(mx, &ex);                                    // mx = fr 2^ex, fr in [0.5, 1)
    const int lp = fr == 0.5 ? ex - 1 : ex;                              // Pmax = 2^lp, |lp| <= 1075
    const int la = (lp + 1) >> 1;                                        // ceil(lp / 2): A = 2^la
    *q = ldexp(1.0, la - qbits);
    *inv_q = ldexp(1.0, qbits - la);
  }
}

template <typename O>
struct CwtTScatDev {
  const cpx<O>* Wx;                  // [batch][na][N]
  const int* mm;                     // [batch][na][N]: target column, -1 where the bin is not kept
  const double* nu;                  // [na]
  const unsigned long long* emax;    // [batch]
  unsigned long long* acc;           // [batch][na][N][2]: the fixed-point cells, zeroed before the scatter
  cpx<O>* Tx;                        // [batch][na][N]
  long long batch, plane, N;         // plane = na N <= 2^40
  int qbits;
};

// grid (min(ceil(plane / 256), 2^31 - 1), min(batch, 65535)): 64-bit flat index i over a signal's na x N bins, lanes
// along time, the x blocks stride over the plane and the y blocks over the signals
template <typename O>
__global__ __launch_bounds__(kCwtTThreads) void cwt_tsst_scatter_kernel(const CwtTScatDev<O> p) {
  const long long stride = (long long)gridDim.x * kCwtTThreads;
  const double cap = ldexp(1.0, p.qbits);
  for (long long b = blockIdx.y; b < p.batch; b += gridDim.y) {
    double q, inv_q;
    cwt_tsst_quantum(p.emax[b], p.qbits, &q, &inv_q);
    if (q == 0.0) continue;
    const long long base = b * p.plane;
    const int lane = threadIdx.x & 63;
    // the loop is uniform over the wave (start and stride are multiples of 64): every lane takes part in the shuffles
    for (long long i = (long long)blockIdx.x * kCwtTThreads + threadIdx.x; i - lane < p.plane; i += stride) {
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
          const double t = nu * r;
          const double f = (t - rint(t)) + fma(nu, r, -t);                // frac(nu r) in turns, |f| <= 1/2 (+ 1 ulp)
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
__global__ __launch_bounds__(kCwtTThreads) void cwt_tsst_readout_kernel(const CwtTScatDev<O> p) {
  const long long stride = (long long)gridDim.x * kCwtTThreads;
  for (long long b = blockIdx.y; b < p.batch; b += gridDim.y) {
    double q, inv_q;
    cwt_tsst_quantum(p.emax[b], p.qbits, &q, &inv_q);
    const long long base = b * p.plane;
    for (long long i = (long long)blockIdx.x * kCwtTThreads + threadIdx.x; i < p.plane; i += stride) {
      const unsigned long long* cell = p.acc + 2 * (base + i);
      p.Tx[base + i] = {(O)((double)(long long)cell[0] * q), (O)((double)(long long)cell[1] * q)};
    }
  }
}

}  // namespace ssq

using namespace ssq;

namespace {

constexpr int64_t kCwtTDefaultWorkBytes = (int64_t)2 << 30;   // the chunk area of the preferred workspace is capped here

struct CwtTShape {
  int64_t P = 0, n1 = 0, n2 = 0, rows = 0, plane = 0;
  int qbits = 0, maps = 0;
  double gamma = 0.0;
  int64_t fixed_bytes = 0, min_bytes = 0, pref_bytes = 0;
};

// workspace: first what does not depend on R -- the signals' maxima [batch] (to a multiple of 16 bytes), the accumulators
// [batch][na][N][2] and the int32 target map [batch][na][N] (to a multiple of 16 bytes) -- then xh [batch][P] and a chunk
// area of R rows ([R][maps][P] spectra and as much again for the transforms' ping-pong)
int64_t cwtt_chunk_bytes(int64_t batch, int64_t P, int64_t R, int maps) { return 16 * P * (batch + 2 * maps * R); }
int64_t cwtt_emax_bytes(int64_t batch) { return (8 * batch + 15) / 16 * 16; }
int64_t cwtt_fixed_bytes(int64_t batch, int64_t plane) {
  return cwtt_emax_bytes(batch) + 16 * batch * plane + (4 * batch * plane + 15) / 16 * 16;
}

int cwtt_shape_only(int dtype, int64_t batch, int64_t N, int64_t na, int order, CwtTShape* s) {
  if (dtype != SSQ_F32 && dtype != SSQ_F64) SSQ_FAIL("dtype must be SSQ_F32 or SSQ_F64");
  if (batch < 1) SSQ_FAIL("batch must be >= 1");
  if (order != 1 && order != 2) SSQ_FAIL("tssq_cwt: order must be 1 or 2");
  if (N < 2 || N > ((int64_t)1 << 26)) SSQ_FAIL("tssq_cwt: n_signal must be in [2, 2^26]");
  if (na < 2 || na > 32767) SSQ_FAIL("tssq_cwt: na must be in [2, 32767]");
  if (na * N > ((int64_t)1 << 40)) SSQ_FAIL("tssq_cwt: na * n_signal must be <= 2^40");
  host::p2up(N, &s->P, &s->n1, &s->n2);
  if (s->P < N || (s->P & (s->P - 1)) != 0) SSQ_FAIL("tssq_cwt: bad padded length");
  if ((double)batch * (double)na * (double)N * 20.0 > 4.0e18 || (double)batch * (double)s->P * 16.0 > 4.0e18)
    SSQ_FAIL("tssq_cwt: transform too large");
  s->rows = batch * na;
  s->plane = na * N;
  s->maps = cwt_tsst_maps(order);
  int L = 0;
  while (((int64_t)1 << L) < N) ++L;                          // ceil(log2 N) <= 26
  s->qbits = std::min(kCwtTQuantumBitsMax, 61 - L);
  s->fixed_bytes = cwtt_fixed_bytes(batch, s->plane);
  s->min_bytes = cwtt_chunk_bytes(batch, s->P, 1, s->maps) + s->fixed_bytes;
  int64_t R = (kCwtTDefaultWorkBytes - 16 * s->P * batch) / (16 * s->P * 2 * s->maps);
  if (R > s->rows) R = s->rows;
  if (R < 1) R = 1;
  s->pref_bytes = cwtt_chunk_bytes(batch, s->P, R, s->maps) + s->fixed_bytes;
  return 0;
}

// every argument check of the entry points (sets the error and returns non-zero): nothing here touches the GPU
int cwtt_check(int dtype, int64_t batch, int64_t N, int wavelet, double p0, double p1, const double* scales,
               const double* nu, int64_t na, double dt, int padtype, int order, double gamma, CwtTShape* s) {
  if (int rc = cwtt_shape_only(dtype, batch, N, na, order, s)) return rc;
  if (wavelet != SSQ_WAVELET_GMW && wavelet != SSQ_WAVELET_MORLET) SSQ_FAIL("tssq_cwt: unknown wavelet");
  if (!(p0 > 0) || !std::isfinite(p0)) SSQ_FAIL("tssq_cwt: wavelet parameter p0 must be positive");
  if (wavelet == SSQ_WAVELET_GMW && (!(p1 > 0) || !std::isfinite(p1)))
    SSQ_FAIL("tssq_cwt: wavelet parameter p1 must be positive");
  if (!scales || !nu) SSQ_FAIL("NULL argument");
  for (int64_t i = 0; i < na; ++i) {
    if (!(scales[i] > 0) || !std::isfinite(scales[i])) SSQ_FAIL("tssq_cwt: scales must be positive and finite");
    if (!(nu[i] > 0) || !std::isfinite(nu[i])) SSQ_FAIL("tssq_cwt: row_freqs must be positive and finite");
  }
  if (!(dt > 0) || !std::isfinite(dt)) SSQ_FAIL("tssq_cwt: dt must be positive");
  if (padtype < SSQ_PAD_REFLECT || padtype > SSQ_PAD_WRAP) SSQ_FAIL("tssq_cwt: unknown padtype");
  if (std::isnan(gamma)) SSQ_FAIL("tssq_cwt: gamma is NaN");
  s->gamma = gamma < 0 ? 10.0 * (dtype == SSQ_F64 ? 2.2204460492503131e-16 : 1.1920928955078125e-07) : gamma;
  return 0;
}

struct CwtTCall {
  int dtype, wavelet, padtype, order;
  int64_t batch, N, na;
  double p0, p1, dt;
  const double *scales, *nu;
};

// The whole transform on device buffers; `work_bytes` >= s.min_bytes sets the rows per chunk.  d_tau, d_mm may be nullptr
// (the targets then live in the workspace alone).  Synchronous.  kernel_ms: three floats, all kernels, the scatter kernel
// alone, and everything before the scatter.
template <typename T, int ORDER>
int cwtt_run(const CwtTCall& c, const CwtTShape& s, const void* d_x, void* d_Tx, void* d_Wx, void* d_tau, void* d_mm,
             void* d_work, int64_t work_bytes, hipStream_t st, float* kernel_ms) {
  constexpr int M = cwt_tsst_maps(ORDER);
  HostCallBufs d;
  TimingEvents t;
  void *d_scales = nullptr, *d_nu = nullptr;
  SSQ_HIP(d.upload(&d_scales, c.scales, sizeof(double) * (size_t)c.na));
  SSQ_HIP(d.upload(&d_nu, c.nu, sizeof(double) * (size_t)c.na));
  if (kernel_ms) SSQ_HIP(t.start(4, st));
  const int64_t P = s.P;
  int64_t R = (work_bytes - s.fixed_bytes - 16 * P * c.batch) / (16 * P * 2 * M);
  if (R > s.rows) R = s.rows;
  const int64_t cells = c.batch * s.plane;
  char* head = static_cast<char*>(d_work);
  unsigned long long* emax = reinterpret_cast<unsigned long long*>(head);                                  // [batch]
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(head + cwtt_emax_bytes(c.batch));       // [cells][2]
  int* mm = d_mm ? static_cast<int*>(d_mm) : reinterpret_cast<int*>(acc + 2 * cells);
  cpx<double>* xh = reinterpret_cast<cpx<double>*>(head + s.fixed_bytes);
  cpx<double>* spec = xh + c.batch * P;                        // [R][M][P]
  cpx<double>* pong = spec + R * M * P;                        // [R][M][P]
  SSQ_HIP(hipMemsetAsync(head, 0, (size_t)(cwtt_emax_bytes(c.batch) + 16 * cells), st));
  SSQ_HIP(cwt_pad<T>(static_cast<const T*>(d_x), xh, c.batch, c.N, P, s.n1, c.padtype, st));
  const int64_t fb = 2 * M * R;                                // signals per forward call: the chunk area is its ping-pong
  for (int64_t b0 = 0; b0 < c.batch; b0 += fb)
    SSQ_HIP(fft_any_batched<double>(xh + b0 * P, spec, P, std::min<int64_t>(fb, c.batch - b0), -1, st));
  CwtTSpecDev sp{};
  sp.xh = xh;
  sp.scales = static_cast<const double*>(d_scales);
  sp.spec = spec;
  sp.P = P;
  sp.na = (int)c.na;
  sp.wv = cwt2_wavelet(c.wavelet, c.p0, c.p1);
  CwtTOpDev<T> op{};
  op.maps = spec;
  op.nu = static_cast<const double*>(d_nu);
  op.emax = emax;
  op.P = P;
  op.N = c.N;
  op.n1 = s.n1;
  op.na = (int)c.na;
  op.inv_P = 1.0 / (double)P;
  op.gamma = s.gamma;
  op.gamma_sq = s.gamma * s.gamma;
  op.dt = c.dt;
  op.dt_o = (T)c.dt;
  for (int64_t r0 = 0; r0 < s.rows; r0 += R) {
    const int64_t nr = std::min<int64_t>(R, s.rows - r0);
    sp.r0 = r0;
    sp.rows = nr;
    hipLaunchKernelGGL((cwt_tsst_spectra_kernel<ORDER>), cwt_rows_grid(P, nr), dim3(kCwtTThreads), 0, st, sp);
    SSQ_HIP(hipGetLastError());
    SSQ_HIP(fft_any_batched<double>(spec, pong, P, M * nr, +1, st));
    op.Wx = static_cast<cpx<T>*>(d_Wx) + r0 * c.N;
    op.tau = d_tau ? static_cast<T*>(d_tau) + r0 * c.N : nullptr;
    op.mm = mm + r0 * c.N;
    op.r0 = r0;
    op.rows = nr;
    hipLaunchKernelGGL((cwt_tsst_operator_kernel<T, ORDER>), cwt_rows_grid(c.N, nr), dim3(kCwtTThreads), 0, st, op);
    SSQ_HIP(hipGetLastError());
  }
  CwtTScatDev<T> sc{};
  sc.Wx = static_cast<const cpx<T>*>(d_Wx);
  sc.mm = mm;
  sc.nu = static_cast<const double*>(d_nu);
  sc.emax = emax;
  sc.acc = acc;
  sc.Tx = static_cast<cpx<T>*>(d_Tx);
  sc.batch = c.batch;
  sc.plane = s.plane;
  sc.N = c.N;
  sc.qbits = s.qbits;
  const dim3 grid((unsigned)std::min<int64_t>((s.plane + kCwtTThreads - 1) / kCwtTThreads, 0x7fffffffLL),
                  (unsigned)std::min<int64_t>(c.batch, 65535));
  if (kernel_ms) SSQ_HIP(hipEventRecord(t.ev[1], st));
  hipLaunchKernelGGL((cwt_tsst_scatter_kernel<T>), grid, dim3(kCwtTThreads), 0, st, sc);
  SSQ_HIP(hipGetLastError());
  if (kernel_ms) SSQ_HIP(hipEventRecord(t.ev[2], st));
  hipLaunchKernelGGL((cwt_tsst_readout_kernel<T>), grid, dim3(kCwtTThreads), 0, st, sc);
  SSQ_HIP(hipGetLastError());
  if (kernel_ms) {
    SSQ_HIP(hipEventRecord(t.ev[3], st));
    SSQ_HIP(hipEventSynchronize(t.ev[3]));
    SSQ_HIP(hipEventElapsedTime(&kernel_ms[0], t.ev[0], t.ev[3]));
    SSQ_HIP(hipEventElapsedTime(&kernel_ms[1], t.ev[1], t.ev[2]));
    SSQ_HIP(hipEventElapsedTime(&kernel_ms[2], t.ev[0], t.ev[1]));
  }
  SSQ_HIP(hipStreamSynchronize(st));                           // (the tables above are freed on return)
  return 0;
}

template <typename T>
int cwtt_run_order(const CwtTCall& c, const CwtTShape& s, const void* d_x, void* d_Tx, void* d_Wx, void* d_tau, void* d_mm,
                   void* d_work, int64_t work_bytes, hipStream_t st, float* kernel_ms) {
  return c.order == 2 ? cwtt_run<T, 2>(c, s, d_x, d_Tx, d_Wx, d_tau, d_mm, d_work, work_bytes, st, kernel_ms)
                      : cwtt_run<T, 1>(c, s, d_x, d_Tx, d_Wx, d_tau, d_mm, d_work, work_bytes, st, kernel_ms);
}

template <typename T>
int cwtt_host_typed(const CwtTCall& c, const CwtTShape& s, const void* x, int64_t work_bytes, void* Tx, void* Wx, void* tau,
                    void* mm) {
  HostCallBufs d;
  const size_t n = (size_t)s.rows * (size_t)c.N;
  void *d_x, *d_Tx, *d_Wx, *d_work, *d_tau = nullptr;
  SSQ_HIP(d.upload(&d_x, x, sizeof(T) * (size_t)c.batch * (size_t)c.N));
  SSQ_HIP(d.alloc(&d_Tx, sizeof(cpx<T>) * n));
  SSQ_HIP(d.alloc(&d_Wx, sizeof(cpx<T>) * n));
  if (tau) SSQ_HIP(d.alloc(&d_tau, sizeof(T) * n));
  SSQ_HIP(d.alloc(&d_work, (size_t)work_bytes));
  if (int rc = cwtt_run_order<T>(c, s, d_x, d_Tx, d_Wx, d_tau, nullptr, d_work, work_bytes, nullptr, nullptr)) return rc;
  SSQ_HIP(hipMemcpy(Tx, d_Tx, sizeof(cpx<T>) * n, hipMemcpyDeviceToHost));
  SSQ_HIP(hipMemcpy(Wx, d_Wx, sizeof(cpx<T>) * n, hipMemcpyDeviceToHost));
  if (tau) SSQ_HIP(hipMemcpy(tau, d_tau, sizeof(T) * n, hipMemcpyDeviceToHost));
  // the targets of the workspace: behind the maxima and the accumulators at its head
  if (mm)
    SSQ_HIP(hipMemcpy(mm, static_cast<const char*>(d_work) + cwtt_emax_bytes(c.batch) + 16 * n, sizeof(int) * n,
                      hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

extern "C" {

int64_t ssq_tssq_cwt_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int order, int64_t* min_bytes) {
  CwtTShape s;
  if (cwtt_shape_only(dtype, batch, n_signal, na, order, &s)) return -1;
  if (min_bytes) *min_bytes = s.min_bytes;
  return s.pref_bytes;
}

int ssq_tssq_cwt_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                      const double* scales, const double* row_freqs, int64_t na, double dt, int padtype, int order,
                      double gamma, void* d_Tx, void* d_Wx, void* d_tau, void* d_mm, void* d_workspace,
                      int64_t workspace_bytes, void* stream, float* kernel_ms) {
  if (!d_x || !d_Tx || !d_Wx || !d_workspace) SSQ_FAIL("NULL argument");
  CwtTShape s;
  if (int rc = cwtt_check(dtype, batch, n_signal, wavelet, p0, p1, scales, row_freqs, na, dt, padtype, order, gamma, &s))
    return rc;
  if (workspace_bytes < s.min_bytes) SSQ_FAIL("tssq_cwt: workspace smaller than the min_bytes of ssq_tssq_cwt_workspace_bytes");
  if (int rc = require_device()) return rc;
  const CwtTCall c{dtype, wavelet, padtype, order, batch, n_signal, na, p0, p1, dt, scales, row_freqs};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dtype == SSQ_F32
             ? cwtt_run_order<float>(c, s, d_x, d_Tx, d_Wx, d_tau, d_mm, d_workspace, workspace_bytes, st, kernel_ms)
             : cwtt_run_order<double>(c, s, d_x, d_Tx, d_Wx, d_tau, d_mm, d_workspace, workspace_bytes, st, kernel_ms);
}

int ssq_tssq_cwt_host(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                      const double* scales, const double* row_freqs, int64_t na, double dt, int padtype, int order,
                      double gamma, int64_t work_limit_bytes, void* Tx, void* Wx, void* tau, void* mm) {
  if (!x || !Tx || !Wx) SSQ_FAIL("NULL argument");
  CwtTShape s;
  if (int rc = cwtt_check(dtype, batch, n_signal, wavelet, p0, p1, scales, row_freqs, na, dt, padtype, order, gamma, &s))
    return rc;
  if (work_limit_bytes < 0 || (work_limit_bytes > 0 && work_limit_bytes < s.min_bytes))
    SSQ_FAIL("tssq_cwt: work_limit_bytes below the min_bytes of ssq_tssq_cwt_workspace_bytes");
  if (int rc = require_device()) return rc;
  const int64_t work = work_limit_bytes > 0
                           ? std::min(work_limit_bytes, cwtt_chunk_bytes(batch, s.P, s.rows, s.maps) + s.fixed_bytes)
                           : s.pref_bytes;
  const CwtTCall c{dtype, wavelet, padtype, order, batch, n_signal, na, p0, p1, dt, scales, row_freqs};
  return dtype == SSQ_F32 ? cwtt_host_typed<float>(c, s, x, work, Tx, Wx, tau, mm)
                          : cwtt_host_typed<double>(c, s, x, work, Tx, Wx, tau, mm);
}

}  // extern "C"
