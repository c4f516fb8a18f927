// cwt_sst2.hip -- second-order ("vertical") synchrosqueezed CWT, `upstream.ssq_cwt2` (Oberlin and Meignen
// 2017, restated for frequency-domain tables).  Upstream has no such transform: the definition is the project's own,
// restated in numpy by tests/helpers/cwt_sst2_ref.py.  Per-sample units, dt enters at the end.  With P, n1, n2 =
// p2up(N), xh the forward DFT of the padded signal, xi_k = 2 pi k / P (k <= P/2, analytic tables: zero above) and, for
// scale a, T0(k) = psih(a xi_k), T1(k) = a psih'(a xi_k) (cwt_sst2_wavelets.h; both halved at 2k == P):
//   W = F^-1[xh T0]   W1 = F^-1[xh i xi T0]   W2 = F^-1[xh (-xi^2) T0]   Wt = F^-1[xh (-i) T1]   Wt1 = F^-1[xh xi T1]
//   D = W^2 + Wt1 W - Wt W1      c = (W2 W - W1^2) / D      om1 = W1 / W      om2 = om1 - c Wt / W
//   w2 = |Im om2| / (2 pi dt) where |D| > gamma^2 and Im om2 is finite, else |Im om1| / (2 pi dt) (ssq_cwt's w);
//   +inf where |W| < gamma (phase_one's rule, ssqueeze.hip).
// A self-contained pipeline beside the tuned CWT plan (api_cwt.hip and its kernels are not involved):
//   cwt_pad_kernel        (cwt_pad.h) pads and widens the signals to complex fp64; the forward DFT is
//                         fft_any_batched's.
//   cwt2_spectra_kernel   for a chunk of (signal, scale) rows: T0, T1 in fp64 in the kernel and the five product spectra
//                         into the workspace, one thread per bin k, coalesced along k, zeros above P/2.
//   (fft_any_batched)     the 5 x rows inverse transforms of the chunk: the generic streaming passes, not the tile FFTs
//                         of cwt_kernels.h -- a first version with no time target (DESIGN 4.12 has the cost).
//   cwt2_operator_kernel  one thread per (row, column), lanes along time: the five values, 1 / P, the operator with
//                         1 / |W|^2 and 1 / |D|^2 formed once, Wx and w2 out in the call's dtype.
//   ssq_ssqueeze_w_exec   the deterministic scatter of Wx under w2 (rows ascending, no atomics) into Tx.
// Transforms and operator run in fp64 for float32 calls too: the operator is a quotient of two differences of products
// (the decision of DESIGN 4.11, taken over).  Wx and w2 are rounded once on store, the scatter runs in the call's dtype
// on the rounded values, so Tx is the scatter of what the call reports.  A row is transformed on its own by every
// kernel, so its result depends neither on the chunk it is in nor on the batch.
#include <cmath>
#include <vector>

#include "../../include/ssq_hip.h"
#include "cwt_pad.h"
#include "cwt_sst2_wavelets.h"
#include "dev_buffers.h"
#include "fft_generic.h"
#include "host_math.h"

namespace ssq {

constexpr int kCwt2Threads = 256;
constexpr int kCwt2Maps = 5;                                  // W, W1, W2, Wt, Wt1

struct Cwt2SpecDev {
  const cpx<double>* xh;     // [batch][P]: the forward DFTs
  const double* scales;      // [na]
  cpx<double>* spec;         // [rows][5][P]: the chunk's product spectra (then, in place, their inverse transforms)
  long long P, r0, rows;     // the chunk: rows r0 .. r0 + rows - 1 of the batch x na
  int na;
  Cwt2Wavelet wv;
};

// grid (ceil(P / 256), min(rows, 65535)): thread k of row r0 + rl
__global__ __launch_bounds__(kCwt2Threads) void cwt2_spectra_kernel(const Cwt2SpecDev p) {
  const long long k = (long long)blockIdx.x * kCwt2Threads + threadIdx.x;
  if (k >= p.P) return;
  const bool live = 2 * k <= p.P;
  for (long long rl = blockIdx.y; rl < p.rows; rl += gridDim.y) {
    const long long r = p.r0 + rl;
    const long long b = r / p.na;
    const double a = p.scales[r - b * p.na];
    cpx<double>* __restrict__ out = p.spec + rl * kCwt2Maps * p.P + k;
    cpx<double> s0 = {0.0, 0.0}, s1 = s0, s2 = s0, s3 = s0, s4 = s0;
    if (live) {
      double xi, T0, T1;
      cwt2_tables_at(p.wv, a, k, p.P, &xi, &T0, &T1);
      const cpx<double> X = p.xh[b * p.P + k];
      const double xT0 = xi * T0;
      s0 = {X.x * T0, X.y * T0};
      s1 = {-X.y * xT0, X.x * xT0};                           // X i xi T0
      s2 = {-X.x * (xi * xT0), -X.y * (xi * xT0)};            // X (-xi^2) T0
      s3 = {X.y * T1, -X.x * T1};                             // X (-i) T1
      s4 = {X.x * (xi * T1), X.y * (xi * T1)};                // X xi T1
    }
    out[0] = s0;
    out[p.P] = s1;
    out[2 * p.P] = s2;
    out[3 * p.P] = s3;
    out[4 * p.P] = s4;
  }
}

template <typename O>
struct Cwt2OpDev {
  const cpx<double>* maps;   // [rows][5][P]: the unnormalised inverse transforms
  cpx<O>* Wx;                // [batch * na][N], at the chunk's first row
  O* w2;
  long long P, N, n1, rows;
  double inv_P, gamma, gamma_sq, inv_two_pi_dt;
};

// grid (ceil(N / 256), min(rows, 65535)): thread = column j of row rl
template <typename O>
__global__ __launch_bounds__(kCwt2Threads) void cwt2_operator_kernel(const Cwt2OpDev<O> p) {
  using T = double;
  const long long j = (long long)blockIdx.x * kCwt2Threads + threadIdx.x;
  if (j >= p.N) return;
  for (long long rl = blockIdx.y; rl < p.rows; rl += gridDim.y) {
    const cpx<T>* __restrict__ in = p.maps + rl * kCwt2Maps * p.P + p.n1 + j;
    const cpx<T> W = cscale(in[0], p.inv_P), W1 = cscale(in[p.P], p.inv_P), W2 = cscale(in[2 * p.P], p.inv_P),
                 Wt = cscale(in[3 * p.P], p.inv_P), Wt1 = cscale(in[4 * p.P], p.inv_P);
    const T den = W.x * W.x + W.y * W.y;
    const T inv_den = (T)1 / den;
    const T im1 = (W1.y * W.x - W1.x * W.y) * inv_den;                      // Im(W1 / W)
    const cpx<T> D = cmul(W, W) + cmul(Wt1, W) - cmul(Wt, W1);
    const cpx<T> num = cmul(W2, W) - cmul(W1, W1);
    const cpx<T> r = {(Wt.x * W.x + Wt.y * W.y) * inv_den, (Wt.y * W.x - Wt.x * W.y) * inv_den};    // Wt / W
    const cpx<T> nr = cmul(num, r);
    const T dd = D.x * D.x + D.y * D.y;
    const T inv_dd = (T)1 / dd;
    const T im2 = im1 - (nr.y * D.x - nr.x * D.y) * inv_dd;                 // Im(om1 - c Wt / W)
    const bool second = hypot(D.x, D.y) > p.gamma_sq && isfinite(im2);
    T w = fabs(second ? im2 : im1) * p.inv_two_pi_dt;
    if (hypot(W.x, W.y) < p.gamma) w = (T)INFINITY;
    const long long o = rl * p.N + j;
    p.Wx[o] = {(O)W.x, (O)W.y};
    p.w2[o] = (O)w;
  }
}

}  // namespace ssq

using namespace ssq;

namespace {

constexpr int64_t kCwt2DefaultWorkBytes = (int64_t)2 << 30;   // the preferred workspace is capped here

struct Cwt2Shape {
  int64_t P = 0, n1 = 0, n2 = 0, rows = 0;
  double gamma = 0.0;
  int64_t min_bytes = 0, pref_bytes = 0;
};

// workspace: xh [batch][P], then a chunk area of R rows: [R][5][P] spectra and as much again for the transforms' ping-pong
int64_t cwt2_work_bytes(int64_t batch, int64_t P, int64_t R) { return 16 * P * (batch + 2 * kCwt2Maps * R); }

int cwt2_shape_only(int dtype, int64_t batch, int64_t N, int64_t na, Cwt2Shape* s) {
  if (dtype != SSQ_F32 && dtype != SSQ_F64) SSQ_FAIL("dtype must be SSQ_F32 or SSQ_F64");
  if (batch < 1) SSQ_FAIL("batch must be >= 1");
  if (N < 2 || N > ((int64_t)1 << 26)) SSQ_FAIL("ssq_cwt2: n_signal must be in [2, 2^26]");
  if (na < 2 || na > 32767) SSQ_FAIL("ssq_cwt2: na must be in [2, 32767]");
  host::p2up(N, &s->P, &s->n1, &s->n2);
  if (s->P < N || (s->P & (s->P - 1)) != 0) SSQ_FAIL("ssq_cwt2: bad padded length");
  if ((double)batch * (double)na * (double)N * 16.0 > 9.0e18 || (double)batch * (double)s->P * 16.0 > 4.0e18)
    SSQ_FAIL("ssq_cwt2: transform too large");
  s->rows = batch * na;
  s->min_bytes = cwt2_work_bytes(batch, s->P, 1);
  int64_t R = (kCwt2DefaultWorkBytes - 16 * s->P * batch) / (16 * s->P * 2 * kCwt2Maps);
  if (R > s->rows) R = s->rows;
  if (R < 1) R = 1;
  s->pref_bytes = cwt2_work_bytes(batch, s->P, R);
  return 0;
}

// every argument check of the entry points (sets the error and returns non-zero): nothing here touches the GPU
int cwt2_check(int dtype, int64_t batch, int64_t N, int wavelet, double p0, double p1, const double* scales, int64_t na,
               double dt, const double* row_const, const double* f_asc, int freq_kind, int64_t freq_transition, int padtype,
               int squeezing, double gamma, Cwt2Shape* s) {
  if (int rc = cwt2_shape_only(dtype, batch, N, na, s)) return rc;
  if (wavelet != SSQ_WAVELET_GMW && wavelet != SSQ_WAVELET_MORLET) SSQ_FAIL("ssq_cwt2: unknown wavelet");
  if (!(p0 > 0) || !std::isfinite(p0)) SSQ_FAIL("ssq_cwt2: wavelet parameter p0 must be positive");
  if (wavelet == SSQ_WAVELET_GMW && (!(p1 > 0) || !std::isfinite(p1))) SSQ_FAIL("ssq_cwt2: wavelet parameter p1 must be positive");
  if (!scales || !row_const || !f_asc) SSQ_FAIL("NULL argument");
  for (int64_t i = 0; i < na; ++i) {
    if (!(scales[i] > 0) || !std::isfinite(scales[i])) SSQ_FAIL("ssq_cwt2: scales must be positive and finite");
    if (!std::isfinite(row_const[i])) SSQ_FAIL("ssq_cwt2: row_const must be finite");
    if (!std::isfinite(f_asc[i])) SSQ_FAIL("ssq_cwt2: ssq_freqs_asc must be finite");
  }
  if (!(dt > 0) || !std::isfinite(dt)) SSQ_FAIL("ssq_cwt2: dt must be positive");
  if (freq_kind != SSQ_FREQS_LOG && freq_kind != SSQ_FREQS_LINEAR && freq_kind != SSQ_FREQS_LOG_PIECEWISE)
    SSQ_FAIL("ssq_cwt2: freq_kind must be SSQ_FREQS_LOG, _LINEAR or _LOG_PIECEWISE");
  if (freq_kind == SSQ_FREQS_LOG_PIECEWISE && (freq_transition < 2 || freq_transition > na - 1))
    SSQ_FAIL("ssq_cwt2: freq_transition must be 2 .. na-1 for SSQ_FREQS_LOG_PIECEWISE");
  if (padtype < SSQ_PAD_REFLECT || padtype > SSQ_PAD_WRAP) SSQ_FAIL("ssq_cwt2: unknown padtype");
  if (squeezing != SSQ_SQUEEZE_SUM && squeezing != SSQ_SQUEEZE_LEBESGUE) SSQ_FAIL("ssq_cwt2: squeezing must be 'sum' or 'lebesgue'");
  if (std::isnan(gamma)) SSQ_FAIL("ssq_cwt2: gamma is NaN");
  s->gamma = gamma < 0 ? 10.0 * (dtype == SSQ_F64 ? 2.2204460492503131e-16 : 1.1920928955078125e-07) : gamma;
  return 0;
}

struct Cwt2Call {
  int dtype, wavelet, freq_kind, padtype, squeezing, variant;
  int64_t batch, N, na, freq_transition;
  double p0, p1, dt;
  const double *scales, *row_const, *f_asc;
};

// The whole transform on device buffers; `work_bytes` >= s.min_bytes sets the rows per chunk.  Synchronous.
template <typename T>
int cwt2_run(const Cwt2Call& c, const Cwt2Shape& s, const void* d_x, void* d_Tx, void* d_Wx, void* d_w2, void* d_work,
             int64_t work_bytes, hipStream_t st, float* kernel_ms) {
  HostCallBufs d;
  TimingEvents t;
  void *d_scales = nullptr, *d_rc = nullptr;
  SSQ_HIP(d.upload(&d_scales, c.scales, sizeof(double) * (size_t)c.na));
  {
    const std::vector<T> rc(c.row_const, c.row_const + c.na);
    SSQ_HIP(d.upload(&d_rc, rc.data(), sizeof(T) * (size_t)c.na));
  }
  if (kernel_ms) SSQ_HIP(t.start(2, st));
  const int64_t P = s.P;
  int64_t R = (work_bytes - 16 * P * c.batch) / (16 * P * 2 * kCwt2Maps);
  if (R > s.rows) R = s.rows;
  cpx<double>* xh = static_cast<cpx<double>*>(d_work);
  cpx<double>* spec = xh + c.batch * P;                        // [R][5][P]
  cpx<double>* pong = spec + R * kCwt2Maps * P;                // [R][5][P]
  SSQ_HIP(cwt_pad<T>(static_cast<const T*>(d_x), xh, c.batch, c.N, P, s.n1, c.padtype, st));
  const int64_t fb = 2 * kCwt2Maps * R;                        // signals per forward call: the chunk area is its ping-pong
  for (int64_t b0 = 0; b0 < c.batch; b0 += fb)
    SSQ_HIP(fft_any_batched<double>(xh + b0 * P, spec, P, std::min<int64_t>(fb, c.batch - b0), -1, st));
  Cwt2SpecDev sp{};
  sp.xh = xh;
  sp.scales = static_cast<const double*>(d_scales);
  sp.spec = spec;
  sp.P = P;
  sp.na = (int)c.na;
  sp.wv = cwt2_wavelet(c.wavelet, c.p0, c.p1);
  Cwt2OpDev<T> op{};
  op.maps = spec;
  op.P = P;
  op.N = c.N;
  op.n1 = s.n1;
  op.inv_P = 1.0 / (double)P;
  op.gamma = s.gamma;
  op.gamma_sq = s.gamma * s.gamma;
  op.inv_two_pi_dt = 1.0 / (6.283185307179586 * c.dt);
  for (int64_t r0 = 0; r0 < s.rows; r0 += R) {
    const int64_t nr = std::min<int64_t>(R, s.rows - r0);
    sp.r0 = r0;
    sp.rows = nr;
    hipLaunchKernelGGL(cwt2_spectra_kernel, cwt_rows_grid(P, nr), dim3(kCwt2Threads), 0, st, sp);
    SSQ_HIP(hipGetLastError());
    SSQ_HIP(fft_any_batched<double>(spec, pong, P, kCwt2Maps * nr, +1, st));
    op.Wx = static_cast<cpx<T>*>(d_Wx) + r0 * c.N;
    op.w2 = static_cast<T*>(d_w2) + r0 * c.N;
    op.rows = nr;
    hipLaunchKernelGGL((cwt2_operator_kernel<T>), cwt_rows_grid(c.N, nr), dim3(kCwt2Threads), 0, st, op);
    SSQ_HIP(hipGetLastError());
  }
  if (int rc = ssq_ssqueeze_w_exec(c.dtype, d_Wx, d_w2, c.batch, c.na, c.N, d_rc, c.f_asc, c.freq_kind, c.freq_transition,
                                   c.squeezing, (c.variant & SSQ_VARIANT_FLIPUD) ? 1 : 0, d_Tx, st))
    return rc;
  if (kernel_ms) {
    SSQ_HIP(hipEventRecord(t.ev[1], st));
    SSQ_HIP(hipEventSynchronize(t.ev[1]));
    SSQ_HIP(hipEventElapsedTime(kernel_ms, t.ev[0], t.ev[1]));
  }
  SSQ_HIP(hipStreamSynchronize(st));                           // (the tables above are freed on return)
  return 0;
}

template <typename T>
int cwt2_host_typed(const Cwt2Call& c, const Cwt2Shape& s, const void* x, int64_t work_bytes, void* Tx, void* Wx, void* w2) {
  HostCallBufs d;
  const size_t n = (size_t)s.rows * (size_t)c.N;
  void *d_x, *d_Tx, *d_Wx, *d_w2, *d_work;
  SSQ_HIP(d.upload(&d_x, x, sizeof(T) * (size_t)c.batch * (size_t)c.N));
  SSQ_HIP(d.alloc(&d_Tx, sizeof(cpx<T>) * n));
  SSQ_HIP(d.alloc(&d_Wx, sizeof(cpx<T>) * n));
  SSQ_HIP(d.alloc(&d_w2, sizeof(T) * n));
  SSQ_HIP(d.alloc(&d_work, (size_t)work_bytes));
  if (int rc = cwt2_run<T>(c, s, d_x, d_Tx, d_Wx, d_w2, d_work, work_bytes, nullptr, nullptr)) return rc;
  SSQ_HIP(hipMemcpy(Tx, d_Tx, sizeof(cpx<T>) * n, hipMemcpyDeviceToHost));
  SSQ_HIP(hipMemcpy(Wx, d_Wx, sizeof(cpx<T>) * n, hipMemcpyDeviceToHost));
  if (w2) SSQ_HIP(hipMemcpy(w2, d_w2, sizeof(T) * n, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

extern "C" {

int64_t ssq_ssq_cwt2_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int64_t* min_bytes) {
  Cwt2Shape s;
  if (cwt2_shape_only(dtype, batch, n_signal, na, &s)) return -1;
  if (min_bytes) *min_bytes = s.min_bytes;
  return s.pref_bytes;
}

int ssq_ssq_cwt2_tables(int wavelet, double p0, double p1, double scale, int64_t P, double* T0, double* T1) {
  if (!T0 || !T1) SSQ_FAIL("NULL argument");
  if (wavelet != SSQ_WAVELET_GMW && wavelet != SSQ_WAVELET_MORLET) SSQ_FAIL("ssq_cwt2: unknown wavelet");
  if (!(p0 > 0) || !std::isfinite(p0)) SSQ_FAIL("ssq_cwt2: wavelet parameter p0 must be positive");
  if (wavelet == SSQ_WAVELET_GMW && (!(p1 > 0) || !std::isfinite(p1))) SSQ_FAIL("ssq_cwt2: wavelet parameter p1 must be positive");
  if (!(scale > 0) || !std::isfinite(scale)) SSQ_FAIL("ssq_cwt2: scale must be positive and finite");
  if (P < 2 || (P & (P - 1)) != 0) SSQ_FAIL("ssq_cwt2: P must be a power of two >= 2");
  const Cwt2Wavelet wv = cwt2_wavelet(wavelet, p0, p1);
  for (int64_t k = 0; k < P; ++k) {
    double xi;
    T0[k] = 0.0;
    T1[k] = 0.0;
    if (2 * k <= P) cwt2_tables_at(wv, scale, k, P, &xi, &T0[k], &T1[k]);
  }
  return 0;
}

int ssq_ssq_cwt2_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                      const double* scales, int64_t na, double dt, const double* row_const, const double* ssq_freqs_asc,
                      int freq_kind, int64_t freq_transition, int padtype, int squeezing, double gamma, int variant,
                      void* d_Tx, void* d_Wx, void* d_w2, void* d_workspace, int64_t workspace_bytes, void* stream,
                      float* kernel_ms) {
  if (!d_x || !d_Tx || !d_Wx || !d_w2 || !d_workspace) SSQ_FAIL("NULL argument");
  Cwt2Shape s;
  if (int rc = cwt2_check(dtype, batch, n_signal, wavelet, p0, p1, scales, na, dt, row_const, ssq_freqs_asc, freq_kind,
                          freq_transition, padtype, squeezing, gamma, &s))
    return rc;
  if (workspace_bytes < s.min_bytes) SSQ_FAIL("ssq_cwt2: workspace smaller than the min_bytes of ssq_ssq_cwt2_workspace_bytes");
  if (int rc = require_device()) return rc;
  const Cwt2Call c{dtype, wavelet, freq_kind, padtype, squeezing, variant, batch, n_signal, na, freq_transition,
                   p0,    p1,      dt,        scales,  row_const, ssq_freqs_asc};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dtype == SSQ_F32 ? cwt2_run<float>(c, s, d_x, d_Tx, d_Wx, d_w2, d_workspace, workspace_bytes, st, kernel_ms)
                          : cwt2_run<double>(c, s, d_x, d_Tx, d_Wx, d_w2, d_workspace, workspace_bytes, st, kernel_ms);
}

int ssq_ssq_cwt2_host(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                      const double* scales, int64_t na, double dt, const double* row_const, const double* ssq_freqs_asc,
                      int freq_kind, int64_t freq_transition, int padtype, int squeezing, double gamma, int variant,
                      int64_t work_limit_bytes, void* Tx, void* Wx, void* w2) {
  if (!x || !Tx || !Wx) SSQ_FAIL("NULL argument");
  Cwt2Shape s;
  if (int rc = cwt2_check(dtype, batch, n_signal, wavelet, p0, p1, scales, na, dt, row_const, ssq_freqs_asc, freq_kind,
                          freq_transition, padtype, squeezing, gamma, &s))
    return rc;
  if (work_limit_bytes < 0 || (work_limit_bytes > 0 && work_limit_bytes < s.min_bytes))
    SSQ_FAIL("ssq_cwt2: work_limit_bytes below the min_bytes of ssq_ssq_cwt2_workspace_bytes");
  if (int rc = require_device()) return rc;
  int64_t work = work_limit_bytes > 0 ? std::min(work_limit_bytes, cwt2_work_bytes(batch, s.P, s.rows)) : s.pref_bytes;
  const Cwt2Call c{dtype, wavelet, freq_kind, padtype, squeezing, variant, batch, n_signal, na, freq_transition,
                   p0,    p1,      dt,        scales,  row_const, ssq_freqs_asc};
  return dtype == SSQ_F32 ? cwt2_host_typed<float>(c, s, x, work, Tx, Wx, w2) : cwt2_host_typed<double>(c, s, x, work, Tx, Wx, w2);
}

}  // extern "C"
