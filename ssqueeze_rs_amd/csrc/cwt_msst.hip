// cwt_msst.hip -- multisynchrosqueezed CWT, `upstream.mssq_cwt` (the CWT counterpart of stft_msst.hip, Yu,
// Wang and Zhao 2019).  Upstream has no such transform: the definition is the project's own, restated in numpy by
// tests/helpers/msst_cwt_ref.py.  Per column, with na rows (scales ascending), w[i] the one-step frequency of row i in
// the call's dtype (order 2: ssq_cwt2's w2 with its fallback, order 1: |Im om1| / (2 pi dt); +inf where |W| < gamma),
// b[i] the one-step bin of w[i] (bin_rule.h's rule, unflipped; -1 where w is infinite) and rho[beta] the row nearest in
// log frequency to bin beta (the rows and the bins are different index sets; the host builds rho once per call):
//   r1[k] = k (kept k);   r(i+1)[k] = rho[b[ri[k]]] if b[rho[b[ri[k]]]] >= 0, else ri[k]        (i = 1 .. n_iter - 1)
//   w_n[k] = w[r_n[k]], +inf where k is not kept;   Tx = ssqueeze(Wx, w_n)
// A coefficient still moves along frequency only, with its own row weight, and keeps its phase: every column keeps its
// weighted sum.
//
//   cwt2 operator half    cwt_sst2.h's, with gamma_sq = +inf for order 1: Wx and w.
//   cwt_msst_walk_kernel  a workgroup owns a tile of C consecutive columns of one signal and all rows.  It stages rho in
//                         LDS, reads the tile's w along columns, bins it and stores the row -> row map G[r] = rho[b[r]]
//                         in LDS as 16-bit values (0xffff: b[r] < 0).  After one barrier every thread walks its elements
//                         n_iter - 1 steps in LDS (the tile is read-only: no barrier between steps; G[nx] == 0xffff is
//                         the "no map of its own" test; a chain ends early on it and on a fixed point).  Then it gathers
//                         w_n = w[r_n] into a plane of its own (never in place: other threads still read w), and, where
//                         asked, r_n and the one-step bins it computed.
//   cwt2 squeeze half     ssq_ssqueeze_w_exec, unchanged, on w_n: it bins w_n by the rule the walk kernel ran, so a
//                         coefficient lands on b[r_n[k]]; the flip is applied there and nowhere else.
// The head of the workspace is the plane of w_n (at every n_iter; n_iter = 1 leaves it unused); McwtPipe runs the three
// stages behind both doors.
#include <cmath>
#include <vector>

#include "../../include/ssq_hip.h"
#include "bin_rule.h"
#include "cwt_sst2.h"
#include "msst_tile.h"

namespace ssq {

template <typename T>
struct CwtWalkDev {
  const T* w;              // [batch][na][n_cols]: the one-step frequency, +inf where an element is not kept
  T* w_n;                  // the same shape, or nullptr (n_iter = 1: w itself is final)
  int* rows;               // r_n, -1 where not kept; may be nullptr
  int* bins;               // b, -1 where not kept; may be nullptr
  const int* row_of_bin;   // [na]: rho, every entry in 0 .. na - 1
  long long n_cols;
  int na, log_c, n_iter;
  BinRule<T> rule;         // unflipped
};

// grid (tiles, signals); na << log_c <= kWalkTileWords
template <typename T>
__global__ __launch_bounds__(kWalkThreads) void cwt_msst_walk_kernel(const CwtWalkDev<T> p) {
  __shared__ unsigned short tile[kWalkTileWords];
  __shared__ unsigned short rho[kWalkMaxRows + 1];
  const int log_c = p.log_c;
  const int cmask = (1 << log_c) - 1;
  const long long col0 = (long long)blockIdx.x << log_c;
  const long long left = p.n_cols - col0;
  const int nc = left < (long long)(cmask + 1) ? (int)left : cmask + 1;                 // the last tile of a signal is narrower
  const long long base = (long long)blockIdx.y * p.na * p.n_cols + col0;
  const int n_el = p.na << log_c;
  for (int i = threadIdx.x; i < p.na; i += kWalkThreads) rho[i] = (unsigned short)p.row_of_bin[i];
  __syncthreads();
  for (int e = threadIdx.x; e < n_el; e += kWalkThreads) {      // neighbouring lanes: neighbouring columns of a row
    const int r = e >> log_c, c = e & cmask;
    unsigned g = kWalkNoMap;
    if (c < nc) {
      const long long o = base + (long long)r * p.n_cols + c;
      const T wv = p.w[o];
      const int b = isinf(wv) ? -1 : bin_of(p.rule, wv);        // 0 .. na - 1 (NaN: bin 0, as ssqueeze has it)
      if (b >= 0) g = rho[b];
      if (p.bins) p.bins[o] = b;
    }
    tile[e] = (unsigned short)g;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n_el; e += kWalkThreads) {
    const int r = e >> log_c, c = e & cmask;
    if (c >= nc) continue;
    unsigned g = tile[e];                                       // G[cur]: cur always has a map of its own
    int cur = g == kWalkNoMap ? -1 : r;
    if (cur >= 0) {
      for (int i = 1; i < p.n_iter; ++i) {
        const unsigned nx = g;
        if (nx == (unsigned)cur) break;                         // a fixed point
        const unsigned gn = tile[(nx << log_c) + c];
        if (gn == kWalkNoMap) break;                            // the row pointed to has no map of its own
        cur = (int)nx;
        g = gn;
      }
    }
    const long long o = base + (long long)r * p.n_cols + c;
    if (p.w_n) p.w_n[o] = cur < 0 ? (T)INFINITY : p.w[base + (long long)cur * p.n_cols + c];
    if (p.rows) p.rows[o] = cur;
  }
}

// the walk of `nb` signals on device buffers (asynchronous on `st`)
template <typename T>
hipError_t cwt_walk_run(CwtWalkDev<T> p, int64_t nb, hipStream_t st) {
  p.log_c = walk_log_cols(p.na);
  const long long tiles = (p.n_cols + (1LL << p.log_c) - 1) >> p.log_c;
  if (p.na < 2 || p.na > kWalkMaxRows || tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t sig = (size_t)p.na * (size_t)p.n_cols;
  const CwtWalkDev<T> p0 = p;
  for (int64_t b0 = 0; b0 < nb; b0 += 65535) {
    const int64_t n1 = nb - b0 < 65535 ? nb - b0 : 65535;
    p.w = p0.w + sig * b0;
    p.w_n = p0.w_n ? p0.w_n + sig * b0 : nullptr;
    p.rows = p0.rows ? p0.rows + sig * b0 : nullptr;
    p.bins = p0.bins ? p0.bins + sig * b0 : nullptr;
    hipLaunchKernelGGL(cwt_msst_walk_kernel<T>, dim3((unsigned)tiles, (unsigned)n1), dim3(kWalkThreads), 0, st, p);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace ssq

using namespace ssq;

namespace {

// the head: the plane of w_n in front of the workspace of ssq_cwt2
constexpr CwtMapsKind kMcwtKind = {"mssq_cwt", "ssq_mssq_cwt_workspace_bytes", 16.0, 9.0e18, 1, 0, 0};

struct McwtCall : Cwt2Call {
  int order, n_iter;
  const int32_t* row_of_bin;
};

const char* mcwt_own_fail(int order, int n_iter, int64_t na) {
  if (order != 1 && order != 2) return "order must be 1 or 2";
  if (n_iter < 1 || n_iter > kWalkMaxIter) return "n_iter must be from 1 to 64";
  if (na > kWalkMaxRows) return "na must be from 2 to 2049";
  return nullptr;
}

int rho_check(const char* pre, const int32_t* row_of_bin, int64_t na) {
  if (!row_of_bin) SSQ_FAIL("NULL argument");
  for (int64_t i = 0; i < na; ++i)
    if (row_of_bin[i] < 0 || row_of_bin[i] >= na) SSQ_FAIL(std::string(pre) + ": row_of_bin holds a row outside 0 .. na - 1");
  return 0;
}

int mcwt_check(const McwtCall& c, CwtMapsShape* s) {
  if (int rc = cwt2_check(kMcwtKind, mcwt_own_fail(c.order, c.n_iter, c.na), c, s)) return rc;
  return rho_check("mssq_cwt", c.row_of_bin, c.na);
}

// mssq_cwt on device buffers (cwt_pipe_host, pipe_exec): the operator half, the walk, the squeeze half.  kernel_ms: three
// parts, the events after the operator half and after the walk.
template <typename T>
struct McwtPipe {
  static constexpr int kMid = 2;
  const McwtCall& c;
  const CwtMapsShape& s;
  DeviceBufs d;
  void *scales, *rc, *rho, *Tx, *Wx, *w, *work;
  CwtWalkDev<T> wk;
  int tables() {
    if (int r = cwt2_tables<T>(d, c, &scales, &rc)) return r;
    SSQ_HIP(d.upload(&rho, c.row_of_bin, sizeof(int32_t) * (size_t)c.na));
    return bin_rule<T>(c.f_asc, c.na, c.freq_kind, c.freq_transition, 0, wk.rule);
  }
  int bind(int64_t, void* const* outs /* Tx, Wx, w, rows, bins */, void* wkspace) {
    Tx = outs[0];
    Wx = outs[1];
    work = wkspace;
    if (!(w = outs[2])) SSQ_HIP(d.alloc(&w, sizeof(T) * (size_t)s.cells));     // (the host door without w: the walk reads it)
    wk.w = static_cast<const T*>(w);
    wk.w_n = c.n_iter > 1 ? cwt_head_at<T>(work, 0) : nullptr;                 // one step: w itself is final
    wk.rows = static_cast<int*>(outs[3]);
    wk.bins = static_cast<int*>(outs[4]);
    wk.row_of_bin = static_cast<const int*>(rho);
    wk.n_cols = c.N;
    wk.na = (int)c.na;
    wk.n_iter = c.n_iter;
    return 0;
  }
  int run(int64_t, const void* d_x, const hipEvent_t* mid) {
    const double gamma_sq = c.order == 1 ? (double)INFINITY : s.gamma * s.gamma;   // |D| > gamma_sq nowhere: |Im om1| / (2 pi dt)
    if (int r = cwt2_operator_run<T>(c, s, gamma_sq, d_x, scales, Wx, w, work)) return r;
    if (mid[0]) SSQ_HIP(hipEventRecord(mid[0], c.st));
    if (wk.w_n || wk.rows || wk.bins) SSQ_HIP(cwt_walk_run<T>(wk, c.batch, c.st));   // (else nothing asks for the walk)
    if (mid[1]) SSQ_HIP(hipEventRecord(mid[1], c.st));
    return cwt2_squeeze_run(c, Wx, wk.w_n ? (const void*)wk.w_n : w, rc, Tx);
  }
};

// the walk alone on the host's maps: host_sliced with no workspace, w in, rows, bins and w_n out
template <typename T>
int mcwt_walk_typed(const void* w, int64_t batch, int64_t na, int64_t n, const double* f_asc, int freq_kind,
                    int64_t freq_transition, const int32_t* row_of_bin, int n_iter, int32_t* rows, int32_t* bins, void* w_n) {
  DeviceBufs d;
  CwtWalkDev<T> wk{};
  if (int rc = bin_rule<T>(f_asc, na, freq_kind, freq_transition, 0, wk.rule)) return rc;
  void* d_rho;
  SSQ_HIP(d.upload(&d_rho, row_of_bin, sizeof(int32_t) * (size_t)na));
  wk.row_of_bin = static_cast<const int*>(d_rho);
  wk.n_cols = n;
  wk.na = (int)na;
  wk.n_iter = n_iter;
  const size_t sig = (size_t)na * (size_t)n;
  const HostOut outs[] = {{rows, sizeof(int32_t) * sig}, {bins, sizeof(int32_t) * sig}, {w_n, sizeof(T) * sig}};
  return host_sliced(
      batch, host_slice(batch, sizeof(T) * sig, outs, 0), w, sizeof(T) * sig, outs,
      [&](int64_t, void* const* o, void*) {
        wk.rows = static_cast<int*>(o[0]);
        wk.bins = static_cast<int*>(o[1]);
        wk.w_n = static_cast<T*>(o[2]);
        return 0;
      },
      [&](int64_t nb, const void* d_w) -> int {
        wk.w = static_cast<const T*>(d_w);
        SSQ_HIP(cwt_walk_run<T>(wk, nb, nullptr));
        return 0;
      });
}

}  // namespace

extern "C" {

int64_t ssq_mssq_cwt_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int64_t* min_bytes) {
  CwtMapsShape s;
  if (cwt_maps_shape(kMcwtKind, kCwt2Maps, mcwt_own_fail(2, 1, na), dtype, batch, n_signal, na, &s)) return -1;
  if (min_bytes) *min_bytes = s.min_bytes;
  return s.pref_bytes;
}

int ssq_mssq_cwt_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                      const double* scales, int64_t na, double dt, const double* row_const, const double* ssq_freqs_asc,
                      int freq_kind, int64_t freq_transition, int padtype, int squeezing, double gamma, int variant, int order,
                      int n_iter, const int32_t* row_of_bin, void* d_Tx, void* d_Wx, void* d_w, int32_t* d_rows,
                      int32_t* d_bins, void* d_workspace, int64_t workspace_bytes, void* stream, float* kernel_ms) {
  if (!d_x || !d_Tx || !d_Wx || !d_w || !d_workspace) SSQ_FAIL("NULL argument");
  const McwtCall c{{{dtype, wavelet, padtype, batch, n_signal, na, p0, p1, dt, gamma, scales, (hipStream_t)stream},
                    freq_kind, squeezing, variant, freq_transition, row_const, ssq_freqs_asc},
                   order, n_iter, row_of_bin};
  CwtMapsShape s;
  if (int rc = mcwt_check(c, &s)) return rc;
  if (int rc = cwt_exec_bytes(kMcwtKind, &s, workspace_bytes)) return rc;
  if (int rc = require_device()) return rc;
  void* const outs[] = {d_Tx, d_Wx, d_w, d_rows, d_bins};
  return dtype == SSQ_F32 ? pipe_exec<McwtPipe<float>>(c, s, d_x, outs, d_workspace, kernel_ms, &c.st)
                          : pipe_exec<McwtPipe<double>>(c, s, d_x, outs, d_workspace, kernel_ms, &c.st);
}

int ssq_mssq_cwt_host(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                      const double* scales, int64_t na, double dt, const double* row_const, const double* ssq_freqs_asc,
                      int freq_kind, int64_t freq_transition, int padtype, int squeezing, double gamma, int variant,
                      int64_t work_limit_bytes, int order, int n_iter, const int32_t* row_of_bin, void* Tx, void* Wx, void* w,
                      int32_t* rows, int32_t* bins) {
  if (!x || !Tx || !Wx) SSQ_FAIL("NULL argument");
  const McwtCall c{{{dtype, wavelet, padtype, batch, n_signal, na, p0, p1, dt, gamma, scales, nullptr},
                    freq_kind, squeezing, variant, freq_transition, row_const, ssq_freqs_asc},
                   order, n_iter, row_of_bin};
  CwtMapsShape s;
  if (int rc = mcwt_check(c, &s)) return rc;
  if (int rc = cwt_host_bytes(kMcwtKind, &s, batch, work_limit_bytes)) return rc;
  if (int rc = require_device()) return rc;
  const size_t el = (dtype == SSQ_F32 ? 4 : 8) * (size_t)s.plane, i32 = sizeof(int32_t) * (size_t)s.plane;
  const HostOut outs[] = {{Tx, 2 * el}, {Wx, 2 * el}, {w, el}, {rows, i32}, {bins, i32}};
  return dtype == SSQ_F32 ? cwt_pipe_host<McwtPipe<float>>(c, s, x, outs) : cwt_pipe_host<McwtPipe<double>>(c, s, x, outs);
}

int ssq_mssq_cwt_tile_cols(int64_t na) {
  if (na < 2 || na > kWalkMaxRows) {
    set_error("mssq_cwt_walk: na must be from 2 to 2049");
    return -1;
  }
  return 1 << walk_log_cols((int)na);
}

int ssq_mssq_cwt_walk_host(int dtype, const void* w, int64_t batch, int64_t na, int64_t n_cols, const double* ssq_freqs_asc,
                           int freq_kind, int64_t freq_transition, const int32_t* row_of_bin, int n_iter, int32_t* rows,
                           int32_t* bins, void* w_n) {
  if (!w || !ssq_freqs_asc || !row_of_bin || !rows || !bins || !w_n) SSQ_FAIL("NULL argument");
  if (dtype != SSQ_F32 && dtype != SSQ_F64) SSQ_FAIL("dtype must be SSQ_F32 or SSQ_F64");
  if (batch < 1) SSQ_FAIL("batch must be >= 1");
  if (na < 2 || na > kWalkMaxRows) SSQ_FAIL("mssq_cwt_walk: na must be from 2 to 2049");
  if (n_cols < 1 || n_cols > (1LL << 30)) SSQ_FAIL("mssq_cwt_walk: n_cols must be from 1 to 2^30");
  if (n_iter < 1 || n_iter > kWalkMaxIter) SSQ_FAIL("mssq_cwt_walk: n_iter must be from 1 to 64");
  if (freq_kind != SSQ_FREQS_LOG && freq_kind != SSQ_FREQS_LINEAR && freq_kind != SSQ_FREQS_LOG_PIECEWISE)
    SSQ_FAIL("mssq_cwt_walk: freq_kind must be SSQ_FREQS_LOG, _LINEAR or _LOG_PIECEWISE");
  if (freq_kind == SSQ_FREQS_LOG_PIECEWISE && (freq_transition < 2 || freq_transition > na - 1))
    SSQ_FAIL("mssq_cwt_walk: freq_transition must be 2 .. na-1 for SSQ_FREQS_LOG_PIECEWISE");
  for (int64_t i = 0; i < na; ++i)
    if (!std::isfinite(ssq_freqs_asc[i])) SSQ_FAIL("mssq_cwt_walk: ssq_freqs_asc must be finite");
  if (int rc = rho_check("mssq_cwt_walk", row_of_bin, na)) return rc;
  if (int rc = require_device()) return rc;
  return dtype == SSQ_F32 ? mcwt_walk_typed<float>(w, batch, na, n_cols, ssq_freqs_asc, freq_kind, freq_transition, row_of_bin,
                                                   n_iter, rows, bins, w_n)
                          : mcwt_walk_typed<double>(w, batch, na, n_cols, ssq_freqs_asc, freq_kind, freq_transition, row_of_bin,
                                                    n_iter, rows, bins, w_n);
}

}  // extern "C"
