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

constexpr CwtMapsKind kMcwtKind = {"mssq_cwt", "ssq_mssq_cwt_workspace_bytes", 16.0, 9.0e18, 0};   // no head

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

// the plane of w_n in front of the workspace of ssq_cwt2, to a multiple of 16 bytes
int64_t wn_bytes(int dtype, int64_t batch, int64_t na, int64_t N) {
  return ((dtype == SSQ_F32 ? 4 : 8) * batch * na * N + 15) / 16 * 16;
}

// The three stages on device buffers.  Synchronous.  kernel_ms (may be nullptr): pipeline + operator, walk, scatter.
template <typename T>
int mcwt_run(const Cwt2Call& c, const CwtMapsShape& s, int order, int n_iter, const int32_t* row_of_bin, const void* d_x,
             void* d_Tx, void* d_Wx, void* d_w, int* d_rows, int* d_bins, void* d_wn, void* d_work, int64_t work_bytes,
             hipStream_t st, float* kernel_ms) {
  DeviceBufs d;
  TimingEvents t;
  void *d_scales = nullptr, *d_rc = nullptr, *d_rho = nullptr;
  if (int rc = cwt2_tables<T>(d, c, &d_scales, &d_rc)) return rc;
  SSQ_HIP(d.upload(&d_rho, row_of_bin, sizeof(int32_t) * (size_t)c.m.na));
  CwtWalkDev<T> wk{};
  if (int rc = bin_rule<T>(c.f_asc, c.m.na, c.freq_kind, c.freq_transition, 0, wk.rule)) return rc;
  if (kernel_ms) SSQ_HIP(t.start(4, st));
  const double gamma_sq = order == 1 ? (double)INFINITY : s.gamma * s.gamma;   // |D| > gamma_sq nowhere: |Im om1| / (2 pi dt)
  if (int rc = cwt2_operator_run<T>(c, s, gamma_sq, d_x, d_scales, d_Wx, d_w, d_work, work_bytes, st)) return rc;
  if (kernel_ms) SSQ_HIP(hipEventRecord(t.ev[1], st));
  if (n_iter > 1 || d_rows || d_bins) {                        // (one step, nothing else asked for: w is final)
    wk.w = static_cast<const T*>(d_w);
    wk.w_n = n_iter > 1 ? static_cast<T*>(d_wn) : nullptr;
    wk.rows = d_rows;
    wk.bins = d_bins;
    wk.row_of_bin = static_cast<const int*>(d_rho);
    wk.n_cols = c.m.N;
    wk.na = (int)c.m.na;
    wk.n_iter = n_iter;
    SSQ_HIP(cwt_walk_run<T>(wk, c.m.batch, st));
  }
  if (kernel_ms) SSQ_HIP(hipEventRecord(t.ev[2], st));
  if (int rc = cwt2_squeeze_run(c, d_Wx, n_iter > 1 ? d_wn : d_w, d_rc, d_Tx, st)) return rc;
  if (kernel_ms) {
    SSQ_HIP(hipEventRecord(t.ev[3], st));
    SSQ_HIP(hipEventSynchronize(t.ev[3]));
    for (int i = 0; i < 3; ++i) SSQ_HIP(hipEventElapsedTime(&kernel_ms[i], t.ev[i], t.ev[i + 1]));
  }
  SSQ_HIP(hipStreamSynchronize(st));                           // (the tables above are freed on return)
  return 0;
}

template <typename T>
int mcwt_host_typed(const Cwt2Call& c, const CwtMapsShape& s, int order, int n_iter, const int32_t* row_of_bin, const void* x,
                    int64_t work_bytes, void* Tx, void* Wx, void* w, int32_t* rows, int32_t* bins) {
  DeviceBufs d;
  const size_t n = (size_t)s.rows * (size_t)c.m.N;
  void *d_x, *d_Tx, *d_Wx, *d_w, *d_wn = nullptr, *d_rows = nullptr, *d_bins = nullptr, *d_work;
  SSQ_HIP(d.upload(&d_x, x, sizeof(T) * (size_t)c.m.batch * (size_t)c.m.N));
  SSQ_HIP(d.alloc(&d_Tx, sizeof(cpx<T>) * n));
  SSQ_HIP(d.alloc(&d_Wx, sizeof(cpx<T>) * n));
  SSQ_HIP(d.alloc(&d_w, sizeof(T) * n));
  if (n_iter > 1) SSQ_HIP(d.alloc(&d_wn, sizeof(T) * n));
  if (rows) SSQ_HIP(d.alloc(&d_rows, sizeof(int32_t) * n));
  if (bins) SSQ_HIP(d.alloc(&d_bins, sizeof(int32_t) * n));
  SSQ_HIP(d.alloc(&d_work, (size_t)work_bytes));
  if (int rc = mcwt_run<T>(c, s, order, n_iter, row_of_bin, d_x, d_Tx, d_Wx, d_w, (int*)d_rows, (int*)d_bins, d_wn, d_work,
                           work_bytes, nullptr, nullptr))
    return rc;
  SSQ_HIP(hipMemcpy(Tx, d_Tx, sizeof(cpx<T>) * n, hipMemcpyDeviceToHost));
  SSQ_HIP(hipMemcpy(Wx, d_Wx, sizeof(cpx<T>) * n, hipMemcpyDeviceToHost));
  if (w) SSQ_HIP(hipMemcpy(w, d_w, sizeof(T) * n, hipMemcpyDeviceToHost));
  if (rows) SSQ_HIP(hipMemcpy(rows, d_rows, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  if (bins) SSQ_HIP(hipMemcpy(bins, d_bins, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  return 0;
}

template <typename T>
int mcwt_walk_typed(const void* w, int64_t batch, int64_t na, int64_t n, const double* f_asc, int freq_kind,
                    int64_t freq_transition, const int32_t* row_of_bin, int n_iter, int32_t* rows, int32_t* bins, void* w_n) {
  DeviceBufs d;
  CwtWalkDev<T> wk{};
  if (int rc = bin_rule<T>(f_asc, na, freq_kind, freq_transition, 0, wk.rule)) return rc;
  const size_t sig = (size_t)na * (size_t)n;
  const int64_t slice = slice_signals(batch, (double)sig * (2.0 * sizeof(T) + 2.0 * sizeof(int32_t)), 0.0, batch);
  void *d_w, *d_wn, *d_rows, *d_bins, *d_rho;
  SSQ_HIP(d.upload(&d_rho, row_of_bin, sizeof(int32_t) * (size_t)na));
  SSQ_HIP(d.alloc(&d_w, sizeof(T) * sig * slice));
  SSQ_HIP(d.alloc(&d_wn, sizeof(T) * sig * slice));
  SSQ_HIP(d.alloc(&d_rows, sizeof(int32_t) * sig * slice));
  SSQ_HIP(d.alloc(&d_bins, sizeof(int32_t) * sig * slice));
  wk.w = static_cast<const T*>(d_w);
  wk.w_n = static_cast<T*>(d_wn);
  wk.rows = static_cast<int*>(d_rows);
  wk.bins = static_cast<int*>(d_bins);
  wk.row_of_bin = static_cast<const int*>(d_rho);
  wk.n_cols = n;
  wk.na = (int)na;
  wk.n_iter = n_iter;
  for (int64_t b0 = 0; b0 < batch; b0 += slice) {
    const int64_t nb = batch - b0 < slice ? batch - b0 : slice;
    SSQ_HIP(hipMemcpy(d_w, (const T*)w + sig * b0, sizeof(T) * sig * nb, hipMemcpyHostToDevice));
    SSQ_HIP(cwt_walk_run<T>(wk, nb, nullptr));
    SSQ_HIP(hipMemcpy(rows + sig * b0, d_rows, sizeof(int32_t) * sig * nb, hipMemcpyDeviceToHost));
    SSQ_HIP(hipMemcpy(bins + sig * b0, d_bins, sizeof(int32_t) * sig * nb, hipMemcpyDeviceToHost));
    SSQ_HIP(hipMemcpy((T*)w_n + sig * b0, d_wn, sizeof(T) * sig * nb, hipMemcpyDeviceToHost));
  }
  return 0;
}

}  // namespace

extern "C" {

int64_t ssq_mssq_cwt_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int64_t* min_bytes) {
  CwtMapsShape s;
  if (cwt_maps_shape(kMcwtKind, kCwt2Maps, mcwt_own_fail(2, 1, na), dtype, batch, n_signal, na, &s)) return -1;
  const int64_t head = wn_bytes(dtype, batch, na, n_signal);
  if (min_bytes) *min_bytes = s.min_bytes + head;
  return s.pref_bytes + head;
}

int ssq_mssq_cwt_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                      const double* scales, int64_t na, double dt, const double* row_const, const double* ssq_freqs_asc,
                      int freq_kind, int64_t freq_transition, int padtype, int squeezing, double gamma, int variant, int order,
                      int n_iter, const int32_t* row_of_bin, void* d_Tx, void* d_Wx, void* d_w, int32_t* d_rows,
                      int32_t* d_bins, void* d_workspace, int64_t workspace_bytes, void* stream, float* kernel_ms) {
  if (!d_x || !d_Tx || !d_Wx || !d_w || !d_workspace) SSQ_FAIL("NULL argument");
  const Cwt2Call c{{dtype, wavelet, padtype, batch, n_signal, na, p0, p1, dt, gamma, scales},
                   freq_kind, squeezing, variant, freq_transition, row_const, ssq_freqs_asc};
  CwtMapsShape s;
  if (int rc = cwt2_check(kMcwtKind, mcwt_own_fail(order, n_iter, na), c, &s)) return rc;
  if (int rc = rho_check("mssq_cwt", row_of_bin, na)) return rc;
  const int64_t head = wn_bytes(dtype, batch, na, n_signal);
  if (int rc = cwt_exec_bytes(kMcwtKind, s, workspace_bytes - head)) return rc;
  if (int rc = require_device()) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  void* d_rest = static_cast<char*>(d_workspace) + head;       // w_n first, then the workspace of ssq_cwt2
  return dtype == SSQ_F32 ? mcwt_run<float>(c, s, order, n_iter, row_of_bin, d_x, d_Tx, d_Wx, d_w, d_rows, d_bins, d_workspace,
                                            d_rest, workspace_bytes - head, st, kernel_ms)
                          : mcwt_run<double>(c, s, order, n_iter, row_of_bin, d_x, d_Tx, d_Wx, d_w, d_rows, d_bins, d_workspace,
                                             d_rest, workspace_bytes - head, st, kernel_ms);
}

int ssq_mssq_cwt_host(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                      const double* scales, int64_t na, double dt, const double* row_const, const double* ssq_freqs_asc,
                      int freq_kind, int64_t freq_transition, int padtype, int squeezing, double gamma, int variant,
                      int64_t work_limit_bytes, int order, int n_iter, const int32_t* row_of_bin, void* Tx, void* Wx, void* w,
                      int32_t* rows, int32_t* bins) {
  if (!x || !Tx || !Wx) SSQ_FAIL("NULL argument");
  const Cwt2Call c{{dtype, wavelet, padtype, batch, n_signal, na, p0, p1, dt, gamma, scales},
                   freq_kind, squeezing, variant, freq_transition, row_const, ssq_freqs_asc};
  CwtMapsShape s;
  int64_t work = 0;
  if (int rc = cwt2_check(kMcwtKind, mcwt_own_fail(order, n_iter, na), c, &s)) return rc;
  if (int rc = rho_check("mssq_cwt", row_of_bin, na)) return rc;
  if (int rc = cwt_host_bytes(kMcwtKind, s, batch, work_limit_bytes, &work)) return rc;
  if (int rc = require_device()) return rc;
  return dtype == SSQ_F32 ? mcwt_host_typed<float>(c, s, order, n_iter, row_of_bin, x, work, Tx, Wx, w, rows, bins)
                          : mcwt_host_typed<double>(c, s, order, n_iter, row_of_bin, x, work, Tx, Wx, w, rows, bins);
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
