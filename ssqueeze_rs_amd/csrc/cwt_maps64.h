// cwt_maps64.h -- the fp64 map pipeline that cwt_sst2.hip (ssq_cwt2), cwt_reassign.hip (reassign_cwt) and cwt_tsst.hip
// (tssq_cwt) share, and through the halves those lend, cwt_msst.hip (mssq_cwt) and cwt_tmsst.hip
// (tmssq_cwt).  A self-contained pipeline beside the tuned CWT plan (api_cwt.hip and its kernels are not involved).
// Per-sample units.  With P, n1, n2 = p2up(N), xh the forward DFT of the padded signal, xi_k = 2 pi k / P
// (k <= P/2, analytic tables: zero above) and, for scale a, T0(k) = psih(a xi_k), T1(k) = a psih'(a xi_k)
// (cwt_sst2_wavelets.h; both halved at 2k == P), a row (signal, scale) has up to five maps:
//   W = F^-1[xh T0]   W1 = F^-1[xh i xi T0]   W2 = F^-1[xh (-xi^2) T0]   Wt = F^-1[xh (-i) T1]   Wt1 = F^-1[xh xi T1]
//   cwt_pad_kernel            pads (pad_index.h, no padded real copy) and widens the signals to complex fp64; the
//                             forward DFT is fft_any_batched's.
//   cwt_spectra_kernel<MAPS>  for a chunk of rows: T0, T1 in fp64 in the kernel and the product spectra of the set MAPS
//                             into the workspace, [rows][M][P] in the order above, one thread per bin k, coalesced
//                             along k, zeros above P/2.
//   (fft_any_batched)         the M x rows inverse transforms of the chunk: the generic streaming passes, not the tile
//                             FFTs of cwt_kernels.h.
//   the transform's operator  called back per chunk: one thread per (row, column) reads [rows][M][P] at n1 + j.
// Transforms and operators run in fp64 for float32 calls too: the operators are quotients of differences of products
// (the decision of DESIGN 4.11, taken over).  A row is transformed on its own by every kernel, so its result depends
// neither on the chunk it is in nor on the batch.  Here too: what the operator, scatter and read-out kernels of the two
// scatter transforms share (the maximum's reduction, the time rule, the power of two of a quantum), and the shape,
// workspace layout and argument checks of the entry points.  The workspace is a fixed head of the transform's own
// (cwt_head: mssq_cwt's w_n plane, or the signals' maxima, the accumulators and the int32 target planes; none for
// ssq_cwt2), then xh [batch][P] and a chunk area of R rows: [R][M][P] spectra and as much again for the transforms'
// ping-pong.  Each transform is one pipe struct (tables, bind, run) behind the two doors of dev_buffers.h; the doors
// take the batch whole (cwt_pipe_host), because the workspace is not linear in the signals.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/ssq_hip.h"
#include "cwt_sst2_wavelets.h"
#include "dev_buffers.h"
#include "fft_generic.h"
#include "host_math.h"
#include "pad_index.h"

namespace ssq {

constexpr int kCwtThreads = 256;

// a grid of 256-lane workgroups along `cols`, its y blocks striding over `rows`
inline dim3 cwt_rows_grid(int64_t cols, int64_t rows) {
  return dim3((unsigned)((cols + kCwtThreads - 1) / kCwtThreads), (unsigned)std::min<int64_t>(rows, 65535));
}

// xh[b][m] = (x[b][pad_index(m - n1)], 0) in fp64, m < P.  grid (ceil(P / 256), min(batch, 65535))
template <typename O>
__global__ __launch_bounds__(kCwtThreads) void cwt_pad_kernel(const O* __restrict__ x, cpx<double>* __restrict__ xh,
                                                              long long batch, long long N, long long P, long long n1,
                                                              int padtype) {
  const long long m = (long long)blockIdx.x * kCwtThreads + threadIdx.x;
  if (m >= P) return;
  const long long src = pad_index(padtype, m - n1, N);
  for (long long b = blockIdx.y; b < batch; b += gridDim.y)
    xh[b * P + m] = {src >= 0 ? (double)x[b * N + src] : 0.0, 0.0};
}

// a set of maps, and a map's slot in a row of the set: the order W, W1, W2, Wt, Wt1 restricted to it
enum : unsigned { kMapW = 1, kMapW1 = 2, kMapW2 = 4, kMapWt = 8, kMapWt1 = 16, kMapsAll = 31 };
constexpr int cwt_map_count(unsigned maps) { return maps ? (int)(maps & 1) + cwt_map_count(maps >> 1) : 0; }
constexpr int cwt_map_slot(unsigned maps, unsigned map) { return cwt_map_count(maps & (map - 1)); }

struct CwtSpecDev {
  const cpx<double>* xh;     // [batch][P]: the forward DFTs
  const double* scales;      // [na]
  cpx<double>* spec;         // [rows][M][P]: the chunk's product spectra (then, in place, their inverse transforms)
  long long P, r0, rows;     // the chunk: rows r0 .. r0 + rows - 1 of the batch x na
  int na;
  Cwt2Wavelet wv;
};

// grid (ceil(P / 256), min(rows, 65535)): thread k of row r0 + rl
template <unsigned MAPS>
__global__ __launch_bounds__(kCwtThreads) void cwt_spectra_kernel(const CwtSpecDev p) {
  static_assert((MAPS & kMapW) && MAPS <= kMapsAll, "a set of the five maps with W in it");
  constexpr int M = cwt_map_count(MAPS);
  const long long k = (long long)blockIdx.x * kCwtThreads + threadIdx.x;
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
      const double xT0 = xi * T0;
      s0 = {X.x * T0, X.y * T0};
      if constexpr (MAPS & kMapW1) s1 = {-X.y * xT0, X.x * xT0};                    // X i xi T0
      if constexpr (MAPS & kMapW2) s2 = {-X.x * (xi * xT0), -X.y * (xi * xT0)};     // X (-xi^2) T0
      if constexpr (MAPS & kMapWt) s3 = {X.y * T1, -X.x * T1};                      // X (-i) T1
      if constexpr (MAPS & kMapWt1) s4 = {X.x * (xi * T1), X.y * (xi * T1)};        // X xi T1
    }
    out[0] = s0;
    if constexpr (MAPS & kMapW1) out[cwt_map_slot(MAPS, kMapW1) * p.P] = s1;
    if constexpr (MAPS & kMapW2) out[cwt_map_slot(MAPS, kMapW2) * p.P] = s2;
    if constexpr (MAPS & kMapWt) out[cwt_map_slot(MAPS, kMapWt) * p.P] = s3;
    if constexpr (MAPS & kMapWt1) out[cwt_map_slot(MAPS, kMapWt1) * p.P] = s4;
  }
}

// max over the workgroup of a non-negative value, then one integer atomic max on its bit pattern (non-negative doubles
// order as their bit patterns do; max is order-independent).  Called by every thread of the workgroup of kCwtThreads;
// red: kCwtThreads / 64 values of LDS.  An operator kernel that reduces max |Wx|^2 per signal lets no thread leave early
// (the barriers here) and flushes when its row loop passes to another signal: the signal a row belongs to is the same
// for the whole workgroup.
__device__ __forceinline__ void cwt_flush_max(double mx, double* red, unsigned long long* dst) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) mx = fmax(mx, __shfl_xor(mx, s, 64));
  __syncthreads();                                           // (the previous flush's reads of `red` are over)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = red[0];
#pragma unroll
    for (int i = 1; i < kCwtThreads / 64; ++i) v = fmax(v, red[i]);
    if (v > 0.0) atomicMax(dst, (unsigned long long)__double_as_longlong(v));
  }
}

// The time rule on the tau a call reports: mm = clip(j + rint(tau / dt), 0, N - 1) in the call's dtype.
// |tau / dt| <= N (1 + eps), the offset being clamped; the bound below only keeps the quotient of an extreme dt inside
// the integer.  (It assigns through a reference: DESIGN 4.12 has what a returned value did to the operator kernels.)
template <typename O>
__device__ __forceinline__ void cwt_time_target(O tau, O dt_o, long long j, long long N, int& mm) {
  const O vt = tau / dt_o;
  const O rv = isfinite(vt) ? rint(vt) : (O)0;
  const long long r = (long long)(rv < (O)-134217728 ? (O)-134217728 : (rv > (O)134217728 ? (O)134217728 : rv));
  long long mt = j + r;
  mt = mt < 0 ? 0 : (mt > N - 1 ? N - 1 : mt);
  mm = (int)mt;
}

// lp with 2^lp the smallest power of two >= a signal's max |Wx|^2 (`bits`: what cwt_flush_max left), |lp| <= 1075;
// false for a signal of zeros or one whose energy is not finite.  The quantum rules of the scatters build on it.
__device__ __forceinline__ bool cwt_pow2_above(unsigned long long bits, int* lp) {
  const double mx = __longlong_as_double((long long)bits);
  if (!(mx > 0.0 && mx <= 1.7976931348623157e308)) return false;
  int ex;
  const double fr = frexp(mx, &ex);                                    // mx = fr 2^ex, fr in [0.5, 1)
  *lp = fr == 0.5 ? ex - 1 : ex;
  return true;
}

// ---------------------------------------------------------------- host side ----

constexpr int64_t kCwtDefaultWorkBytes = (int64_t)2 << 30;    // the chunk area of the preferred workspace is capped here

// what the messages and limits of a transform's entry points differ in
struct CwtMapsKind {
  const char* name;            // the prefix of its messages
  const char* bytes_fn;        // its *_workspace_bytes function, named by the workspace messages
  double big_bytes, big_limit; // batch na N big_bytes > big_limit: "transform too large"
  // its head, per (signal, row, column): planes of the call's real dtype in front (mssq_cwt's w_n), bytes of accumulator
  // (0: no maxima either, and no na N <= 2^40 limit: ssq_cwt2 and mssq_cwt scatter without accumulators), int32 planes
  int real_planes, acc_bytes, int_planes;
};

// what the entry points of the transforms take in common; st: the stream of a device entry point (the host doors run
// on the null stream).  A transform's own call struct derives from it.
struct CwtMapsCall {
  int dtype, wavelet, padtype;
  int64_t batch, N, na;
  double p0, p1, dt, gamma;
  const double* scales;
  hipStream_t st;
};

// The head of a workspace, the one layout of every kind (byte offsets): the real planes [cells] each, the signals'
// maxima [batch] (to a multiple of 16 bytes), the accumulators [cells] and the int32 planes [cells] each; `bytes` to a
// multiple of 16.  The maxima and the accumulators (emax .. planes) are what a call zeroes.
struct CwtHead {
  int64_t emax = 0, acc = 0, planes = 0, bytes = 0;
};

struct CwtMapsShape {
  int64_t P = 0, n1 = 0, n2 = 0, rows = 0, plane = 0, cells = 0;
  int maps = 0;
  double gamma = 0.0;
  CwtHead head;
  int64_t min_bytes = 0, pref_bytes = 0;
  int64_t work_bytes = 0;      // of the workspace the call runs in (cwt_exec_bytes, cwt_host_bytes): sets the rows per chunk
};

// xh and the chunk area of R rows; the signals' maxima [batch] to a multiple of 16 bytes; rows per chunk in `bytes`
inline int64_t cwt_chunk_bytes(int64_t batch, int64_t P, int64_t R, int maps) { return 16 * P * (batch + 2 * maps * R); }
inline int64_t cwt_emax_bytes(int64_t batch) { return (8 * batch + 15) / 16 * 16; }
inline int64_t cwt_chunk_rows(int64_t bytes, int64_t batch, int64_t P, int maps) {
  return (bytes - 16 * P * batch) / (16 * P * 2 * maps);
}
inline CwtHead cwt_head(const CwtMapsKind& k, int dtype, int64_t batch, int64_t cells) {
  CwtHead h;
  h.emax = (k.real_planes * (dtype == SSQ_F32 ? 4 : 8) * cells + 15) / 16 * 16;
  h.acc = h.emax + (k.acc_bytes ? cwt_emax_bytes(batch) : 0);
  h.planes = h.acc + k.acc_bytes * cells;
  h.bytes = (h.planes + 4 * k.int_planes * cells + 15) / 16 * 16;
  return h;
}
template <typename P>
P* cwt_head_at(void* d_work, int64_t offset) {
  return reinterpret_cast<P*>(static_cast<char*>(d_work) + offset);
}

// The limits of the three transforms and the shape they work on (sets the error and returns non-zero).  own_fail: the
// message of the entry point's own argument check (order), or nullptr where it passed; it is reported in its place.
inline int cwt_maps_shape(const CwtMapsKind& k, int maps, const char* own_fail, int dtype, int64_t batch, int64_t N,
                          int64_t na, CwtMapsShape* s) {
  const std::string pre = std::string(k.name) + ": ";
  if (dtype != SSQ_F32 && dtype != SSQ_F64) SSQ_FAIL("dtype must be SSQ_F32 or SSQ_F64");
  if (batch < 1) SSQ_FAIL("batch must be >= 1");
  if (own_fail) SSQ_FAIL(pre + own_fail);
  if (N < 2 || N > ((int64_t)1 << 26)) SSQ_FAIL(pre + "n_signal must be in [2, 2^26]");
  if (na < 2 || na > 32767) SSQ_FAIL(pre + "na must be in [2, 32767]");
  if (k.acc_bytes && na * N > ((int64_t)1 << 40)) SSQ_FAIL(pre + "na * n_signal must be <= 2^40");
  host::p2up(N, &s->P, &s->n1, &s->n2);
  if (s->P < N || (s->P & (s->P - 1)) != 0) SSQ_FAIL(pre + "bad padded length");
  if ((double)batch * (double)na * (double)N * k.big_bytes > k.big_limit || (double)batch * (double)s->P * 16.0 > 4.0e18)
    SSQ_FAIL(pre + "transform too large");
  s->rows = batch * na;
  s->plane = na * N;
  s->cells = batch * s->plane;
  s->maps = maps;
  s->head = cwt_head(k, dtype, batch, s->cells);
  s->min_bytes = cwt_chunk_bytes(batch, s->P, 1, maps) + s->head.bytes;
  const int64_t R = std::max<int64_t>(1, std::min(cwt_chunk_rows(kCwtDefaultWorkBytes, batch, s->P, maps), s->rows));
  s->pref_bytes = cwt_chunk_bytes(batch, s->P, R, maps) + s->head.bytes;
  return 0;
}

inline int cwt_wavelet_check(const std::string& pre, int wavelet, double p0, double p1) {
  if (wavelet != SSQ_WAVELET_GMW && wavelet != SSQ_WAVELET_MORLET) SSQ_FAIL(pre + "unknown wavelet");
  if (!(p0 > 0) || !std::isfinite(p0)) SSQ_FAIL(pre + "wavelet parameter p0 must be positive");
  if (wavelet == SSQ_WAVELET_GMW && (!(p1 > 0) || !std::isfinite(p1))) SSQ_FAIL(pre + "wavelet parameter p1 must be positive");
  return 0;
}

// Every argument check of the entry points, in their order (sets the error and returns non-zero): nothing here touches
// the GPU.  The transform's own checks are reported in their places: own_fail as in cwt_maps_shape; rows() checks its
// [na] arrays (NULL, then row by row with its checks interleaved) and returns non-zero with the error set;
// f_kind / f_transition: the bin grid of the transforms that have one (ssq_cwt2, reassign_cwt), else f_kind = nullptr;
// last_fail: the message of a check between padtype and gamma (squeezing), or nullptr.
template <typename Rows>
int cwt_maps_check(const CwtMapsKind& k, int maps, const char* own_fail, const CwtMapsCall& c, Rows&& rows,
                   const int* f_kind, int64_t f_transition, const char* last_fail, CwtMapsShape* s) {
  if (int rc = cwt_maps_shape(k, maps, own_fail, c.dtype, c.batch, c.N, c.na, s)) return rc;
  const std::string pre = std::string(k.name) + ": ";
  if (int rc = cwt_wavelet_check(pre, c.wavelet, c.p0, c.p1)) return rc;
  if (int rc = rows()) return rc;
  if (!(c.dt > 0) || !std::isfinite(c.dt)) SSQ_FAIL(pre + "dt must be positive");
  if (f_kind) {
    if (*f_kind != SSQ_FREQS_LOG && *f_kind != SSQ_FREQS_LINEAR && *f_kind != SSQ_FREQS_LOG_PIECEWISE)
      SSQ_FAIL(pre + "freq_kind must be SSQ_FREQS_LOG, _LINEAR or _LOG_PIECEWISE");
    if (*f_kind == SSQ_FREQS_LOG_PIECEWISE && (f_transition < 2 || f_transition > c.na - 1))
      SSQ_FAIL(pre + "freq_transition must be 2 .. na-1 for SSQ_FREQS_LOG_PIECEWISE");
  }
  if (c.padtype < SSQ_PAD_REFLECT || c.padtype > SSQ_PAD_WRAP) SSQ_FAIL(pre + "unknown padtype");
  if (last_fail) SSQ_FAIL(pre + last_fail);
  if (std::isnan(c.gamma)) SSQ_FAIL(pre + "gamma is NaN");
  s->gamma = c.gamma < 0 ? 10.0 * (c.dtype == SSQ_F64 ? 2.2204460492503131e-16 : 1.1920928955078125e-07) : c.gamma;
  return 0;
}

// the workspace of a device entry point: at least min_bytes
inline int cwt_exec_bytes(const CwtMapsKind& k, CwtMapsShape* s, int64_t workspace_bytes) {
  if (workspace_bytes < s->min_bytes)
    SSQ_FAIL(std::string(k.name) + ": workspace smaller than the min_bytes of " + k.bytes_fn);
  s->work_bytes = workspace_bytes;
  return 0;
}

// the workspace a host entry point allocates: pref_bytes, or with a limit what the limit allows, all rows in one chunk
// at the most.  The limit counts what lies behind the real planes in front (mssq_cwt: ssq_cwt2's workspace, as that
// entry point's limit does); they are added to it.
inline int cwt_host_bytes(const CwtMapsKind& k, CwtMapsShape* s, int64_t batch, int64_t work_limit_bytes) {
  const int64_t front = s->head.emax;
  if (work_limit_bytes < 0 || (work_limit_bytes > 0 && work_limit_bytes < s->min_bytes - front))
    SSQ_FAIL(std::string(k.name) + ": work_limit_bytes below the min_bytes of " + k.bytes_fn);
  s->work_bytes = work_limit_bytes > 0
                      ? front + std::min(work_limit_bytes, cwt_chunk_bytes(batch, s->P, s->rows, s->maps) + s->head.bytes - front)
                      : s->pref_bytes;
  return 0;
}

// the host door of a transform's pipe: the batch in one slice on the workspace cwt_host_bytes chose
template <typename Pipe, typename Call, size_t N>
int cwt_pipe_host(const Call& c, const CwtMapsShape& s, const void* x, const HostOut (&outs)[N]) {
  return pipe_host<Pipe>(c, s, x, (size_t)(c.dtype == SSQ_F32 ? 4 : 8) * (size_t)c.N, outs,
                         HostSlice{c.batch, (size_t)s.work_bytes});
}

// The pipeline up to the operator on device buffers, asynchronous on c.st: carves `d_work` (s.work_bytes >= s.min_bytes
// sets the rows per chunk) behind the head, pads, runs the forward transforms and walks the chunks; per chunk the
// spectra kernel, the inverse transforms, then op(maps, r0, nr) launches the transform's operator on rows r0 .. r0 + nr
// - 1, whose maps are [nr][M][P] at `maps` (non-zero with the error set ends the walk).  d_scales: c.scales on the device.
template <typename T, unsigned MAPS, typename Op>
int cwt_maps_chunks(const CwtMapsCall& c, const CwtMapsShape& s, const void* d_x, const void* d_scales, void* d_work,
                    Op&& op) {
  constexpr int M = cwt_map_count(MAPS);
  const int64_t P = s.P;
  const hipStream_t st = c.st;
  const int64_t R = std::min(cwt_chunk_rows(s.work_bytes - s.head.bytes, c.batch, P, M), s.rows);
  cpx<double>* xh = cwt_head_at<cpx<double>>(d_work, s.head.bytes);
  cpx<double>* spec = xh + c.batch * P;                        // [R][M][P]
  cpx<double>* pong = spec + R * M * P;                        // [R][M][P]
  hipLaunchKernelGGL((cwt_pad_kernel<T>), cwt_rows_grid(P, c.batch), dim3(kCwtThreads), 0, st, static_cast<const T*>(d_x), xh,
                     (long long)c.batch, (long long)c.N, (long long)P, (long long)s.n1, c.padtype);
  SSQ_HIP(hipGetLastError());
  const int64_t fb = 2 * M * R;                                // signals per forward call: the chunk area is its ping-pong
  for (int64_t b0 = 0; b0 < c.batch; b0 += fb)
    SSQ_HIP(fft_any_batched<double>(xh + b0 * P, spec, P, std::min<int64_t>(fb, c.batch - b0), -1, st));
  CwtSpecDev sp{};
  sp.xh = xh;
  sp.scales = static_cast<const double*>(d_scales);
  sp.spec = spec;
  sp.P = P;
  sp.na = (int)c.na;
  sp.wv = cwt2_wavelet(c.wavelet, c.p0, c.p1);
  for (int64_t r0 = 0; r0 < s.rows; r0 += R) {
    const int64_t nr = std::min<int64_t>(R, s.rows - r0);
    sp.r0 = r0;
    sp.rows = nr;
    hipLaunchKernelGGL((cwt_spectra_kernel<MAPS>), cwt_rows_grid(P, nr), dim3(kCwtThreads), 0, st, sp);
    SSQ_HIP(hipGetLastError());
    SSQ_HIP(fft_any_batched<double>(spec, pong, P, M * nr, +1, st));
    if (int rc = op(spec, r0, nr)) return rc;
  }
  return 0;
}

}  // namespace ssq
