// cwt_lmsst.hip -- local maximum synchrosqueezed CWT, `upstream.lmssq_cwt`, and the window maximum alone,
// `upstream.lmsst_rows` (the CWT side of stft_lmsst.hip; Yu, Wang, Zhao and Liu 2019).
// Upstream has no such transform: the definition is the project's own, restated in numpy by tests/helpers/lmsst_ref.py.
// Per column, with na rows (scales ascending) and nu_hz[i] the rows' own frequencies in Hz, an argument:
//   A[i] = re^2 + im^2 of Wx[i] as the call reports it (rounded to the call's dtype), evaluated in fp64, the two products
//          and the sum rounded one by one (no fused multiply-add)
//   m[i] = the row of the maximum of A over max(0, i - delta) .. min(na - 1, i + delta), scanned ascending and taken only
//          where strictly greater: the lowest row wins a tie; rows that are not kept take part in the window
//   w[i] = nu_hz[m[i]] rounded once to the call's dtype, +inf where |W| < gamma on the fp64 coefficient (not kept)
//   Tx   = ssqueeze(Wx, w): a coefficient keeps its own row weight and phase
// No derivative of the wavelet: a map set of W alone, ONE inverse transform a row against ssq_cwt2's five.
//
//   cwt_lmsst_wx_kernel    the operator of the shared pipeline (cwt_maps64.h), per chunk of rows: Wx as cwt2_operator_kernel
//                          rounds it, and the keep rule on the fp64 coefficient left in the w plane (0: kept, +inf: not).
//   lmsst_rows_kernel      after the pipeline, over the finished Wx of ALL rows of a signal (chunks of rows end inside a
//                          signal, so the window cannot be formed in the per-chunk operator): one thread per column,
//                          lanes along time, rows ascending; a direct scan of the 2 delta + 1 rows of the column, whose
//                          loads are coalesced along time and stay in cache from one row to the next.  It overwrites the
//                          kept cells of w with nu_hz[m] and writes m where asked for.  `lmsst_rows` runs it alone on a
//                          real map the caller holds (a float32 map widened on load, which is exact).
//   cwt2 squeeze half      ssq_ssqueeze_w_exec, unchanged, on w.
// CwtLmsstPipe runs the three stages behind both doors.
#include <cmath>
#include <vector>

#include "../../include/ssq_hip.h"
#include "cwt_sst2.h"

namespace ssq {

constexpr int kLmsstMaxDelta = 256;       // a bound on work (the scan reads 2 delta + 1 rows a cell), not a measured number
constexpr int kLmsstMaxRows = 2049;

// re^2 + im^2 with the products and the sum rounded one by one
__device__ __forceinline__ double lmsst_energy(double re, double im) {
#pragma clang fp contract(off)
  const double a = re * re;
  const double b = im * im;
  return a + b;
}

template <typename O>
struct CwtLmsstWxDev {
  const cpx<double>* maps;   // [rows][1][P]: the unnormalised inverse transforms
  cpx<O>* Wx;                // [batch * na][N], at the chunk's first row
  O* w;                      // the same rows: 0 where the cell is kept, +inf where it is not
  long long P, N, n1, rows;
  double inv_P, gamma;
};

// grid (ceil(N / 256), min(rows, 65535)): thread = column j of row rl
template <typename O>
__global__ __launch_bounds__(kCwtThreads) void cwt_lmsst_wx_kernel(const CwtLmsstWxDev<O> p) {
  const long long j = (long long)blockIdx.x * kCwtThreads + threadIdx.x;
  if (j >= p.N) return;
  for (long long rl = blockIdx.y; rl < p.rows; rl += gridDim.y) {
    const cpx<double> W = cscale(p.maps[rl * p.P + p.n1 + j], p.inv_P);
    const long long o = rl * p.N + j;
    p.Wx[o] = {(O)W.x, (O)W.y};
    p.w[o] = hypot(W.x, W.y) < p.gamma ? (O)INFINITY : (O)0;
  }
}

// the value A of an element: of a complex coefficient in the call's dtype, or of a real map as it is
template <typename O>
struct LmsstSrcCoef {
  const cpx<O>* p;
  __device__ __forceinline__ double operator()(long long o) const {
    const cpx<O> v = p[o];
    return lmsst_energy((double)v.x, (double)v.y);
  }
};
template <typename I>
struct LmsstSrcMap {
  const I* p;
  __device__ __forceinline__ double operator()(long long o) const { return (double)p[o]; }
};

// src: [signals][n_rows][n_cols].  w (may be nullptr): in, +inf where a cell is not kept; out, nu[m] on the kept cells.
// rows_out (may be nullptr): m, -1 where not kept.  grid (ceil(n_cols / 256), min(signals, 65535))
template <typename Src, typename O>
__global__ __launch_bounds__(kCwtThreads) void lmsst_rows_kernel(const Src src, O* __restrict__ w, int* __restrict__ rows_out,
                                                                const O* __restrict__ nu, long long signals, int n_rows,
                                                                long long n_cols, int delta) {
  const long long j = (long long)blockIdx.x * kCwtThreads + threadIdx.x;
  if (j >= n_cols) return;
  for (long long b = blockIdx.y; b < signals; b += gridDim.y) {
    const long long base = b * n_rows * n_cols + j;
    for (int i = 0; i < n_rows; ++i) {
      const long long o = base + (long long)i * n_cols;
      const bool keep = w ? !isinf(w[o]) : true;
      int mb = -1;
      if (keep) {
        const int lo = i - delta < 0 ? 0 : i - delta, hi = i + delta > n_rows - 1 ? n_rows - 1 : i + delta;
        double best = src(base + (long long)lo * n_cols);
        mb = lo;
        for (int r = lo + 1; r <= hi; ++r) {                  // ascending, strictly greater only: the lowest row wins a tie
          const double a = src(base + (long long)r * n_cols);
          if (a > best) {
            best = a;
            mb = r;
          }
        }
        if (w) w[o] = nu[mb];
      }
      if (rows_out) rows_out[o] = mb;
    }
  }
}

template <typename Src, typename O>
hipError_t lmsst_rows_run(Src src, O* d_w, int* d_rows, const O* d_nu, int64_t signals, int n_rows, int64_t n_cols, int delta,
                          hipStream_t st) {
  hipLaunchKernelGGL((lmsst_rows_kernel<Src, O>), cwt_rows_grid(n_cols, signals), dim3(kCwtThreads), 0, st, src, d_w, d_rows,
                     d_nu, (long long)signals, n_rows, (long long)n_cols, delta);
  return hipGetLastError();
}

}  // namespace ssq

using namespace ssq;

namespace {

constexpr CwtMapsKind kCwtLmsstKind = {"lmssq_cwt", "ssq_lmssq_cwt_workspace_bytes", 16.0, 9.0e18, 0, 0, 0};   // no head
constexpr int kCwtLmsstMaps = cwt_map_count(kMapW);

struct CwtLmsstCall : Cwt2Call {
  int delta;
  const double* nu_hz;
};

const char* cwt_lmsst_rows_fail(int64_t na) { return na > kLmsstMaxRows ? "na must be from 2 to 2049" : nullptr; }

// Every argument check of the entry points and the shape they work on (sets the error and returns non-zero; nothing here
// touches the GPU): ssq_cwt2's checks, then the shape once more for a map set of W alone, then delta and the table.
int cwt_lmsst_check(const CwtLmsstCall& c, CwtMapsShape* s) {
  if (int rc = cwt2_check(kCwtLmsstKind, cwt_lmsst_rows_fail(c.na), c, s)) return rc;
  if (int rc = cwt_maps_shape(kCwtLmsstKind, kCwtLmsstMaps, nullptr, c.dtype, c.batch, c.N, c.na, s)) return rc;
  const int64_t top = c.na - 1 < kLmsstMaxDelta ? c.na - 1 : (int64_t)kLmsstMaxDelta;
  if (c.delta < 1 || c.delta > top) SSQ_FAIL("lmssq_cwt: delta must be from 1 to min(na - 1, 256)");
  if (!c.nu_hz) SSQ_FAIL("NULL argument");
  for (int64_t i = 0; i < c.na; ++i)
    if (!(c.nu_hz[i] > 0) || !std::isfinite(c.nu_hz[i])) SSQ_FAIL("lmssq_cwt: row_freqs_hz must be positive and finite");
  return 0;
}

// lmssq_cwt on device buffers (cwt_pipe_host, pipe_exec): the chunked maps of W alone, the plane kernel, the squeeze
// half.  kernel_ms: three parts, the events after the pipeline and after the plane kernel.
template <typename T>
struct CwtLmsstPipe {
  static constexpr int kMid = 2;
  const CwtLmsstCall& c;
  const CwtMapsShape& s;
  DeviceBufs d;
  void *scales, *rc, *nu, *work, *Tx, *Wx, *w, *rows;
  int tables() {
    if (int r = cwt2_tables<T>(d, c, &scales, &rc)) return r;
    const std::vector<T> n(c.nu_hz, c.nu_hz + c.na);                          // each frequency rounded once to the call's dtype
    SSQ_HIP(d.upload(&nu, n.data(), sizeof(T) * n.size()));
    return 0;
  }
  int bind(int64_t, void* const* outs /* Tx, Wx, w, rows */, void* wk) {
    work = wk;
    Tx = outs[0];
    Wx = outs[1];
    if (!(w = outs[2])) SSQ_HIP(d.alloc(&w, sizeof(T) * (size_t)s.cells));   // (the host door without w: the squeeze reads it)
    rows = outs[3];
    return 0;
  }
  int run(int64_t, const void* d_x, const hipEvent_t* mid) {
    const int64_t N = c.N;
    CwtLmsstWxDev<T> op{};
    op.P = s.P;
    op.N = N;
    op.n1 = s.n1;
    op.inv_P = 1.0 / (double)s.P;
    op.gamma = s.gamma;
    const auto launch_op = [&](const cpx<double>* maps, int64_t r0, int64_t nr) -> int {
      op.maps = maps;
      op.Wx = static_cast<cpx<T>*>(Wx) + r0 * N;
      op.w = static_cast<T*>(w) + r0 * N;
      op.rows = nr;
      hipLaunchKernelGGL((cwt_lmsst_wx_kernel<T>), cwt_rows_grid(N, nr), dim3(kCwtThreads), 0, c.st, op);
      SSQ_HIP(hipGetLastError());
      return 0;
    };
    if (int r = cwt_maps_chunks<T, kMapW>(c, s, d_x, scales, work, launch_op)) return r;
    if (mid[0]) SSQ_HIP(hipEventRecord(mid[0], c.st));
    SSQ_HIP(lmsst_rows_run(LmsstSrcCoef<T>{static_cast<const cpx<T>*>(Wx)}, static_cast<T*>(w), static_cast<int*>(rows),
                           static_cast<const T*>(nu), c.batch, (int)c.na, N, c.delta, c.st));
    if (mid[1]) SSQ_HIP(hipEventRecord(mid[1], c.st));
    return cwt2_squeeze_run(c, Wx, w, rc, Tx);
  }
};

// the plane kernel alone on the host's maps: host_sliced with no workspace, A in, m out
template <typename I>
int lmsst_rows_typed(const void* A, int64_t batch, int64_t n_rows, int64_t n_cols, int delta, int32_t* rows) {
  const size_t sig = (size_t)n_rows * (size_t)n_cols;
  const HostOut outs[] = {{rows, sizeof(int32_t) * sig}};
  int* d_rows = nullptr;
  return host_sliced(
      batch, host_slice(batch, sizeof(I) * sig, outs, 0), A, sizeof(I) * sig, outs,
      [&](int64_t, void* const* o, void*) {
        d_rows = static_cast<int*>(o[0]);
        return 0;
      },
      [&](int64_t nb, const void* d_A) -> int {
        SSQ_HIP(lmsst_rows_run(LmsstSrcMap<I>{static_cast<const I*>(d_A)}, (double*)nullptr, d_rows, (const double*)nullptr, nb,
                               (int)n_rows, n_cols, delta, nullptr));
        return 0;
      });
}

}  // namespace

extern "C" {

int64_t ssq_lmssq_cwt_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int64_t* min_bytes) {
  CwtMapsShape s;
  if (cwt_maps_shape(kCwtLmsstKind, kCwtLmsstMaps, cwt_lmsst_rows_fail(na), dtype, batch, n_signal, na, &s)) return -1;
  if (min_bytes) *min_bytes = s.min_bytes;
  return s.pref_bytes;
}

int ssq_lmssq_cwt_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                       const double* scales, int64_t na, double dt, const double* row_const, const double* ssq_freqs_asc,
                       int freq_kind, int64_t freq_transition, int padtype, int squeezing, double gamma, int variant, int delta,
                       const double* row_freqs_hz, void* d_Tx, void* d_Wx, void* d_w, int32_t* d_rows, void* d_workspace,
                       int64_t workspace_bytes, void* stream, float* kernel_ms) {
  if (!d_x || !d_Tx || !d_Wx || !d_w || !d_workspace) SSQ_FAIL("NULL argument");
  const CwtLmsstCall c{{{dtype, wavelet, padtype, batch, n_signal, na, p0, p1, dt, gamma, scales, (hipStream_t)stream},
                        freq_kind, squeezing, variant, freq_transition, row_const, ssq_freqs_asc},
                       delta, row_freqs_hz};
  CwtMapsShape s;
  if (int rc = cwt_lmsst_check(c, &s)) return rc;
  if (int rc = cwt_exec_bytes(kCwtLmsstKind, &s, workspace_bytes)) return rc;
  if (int rc = require_device()) return rc;
  void* const outs[] = {d_Tx, d_Wx, d_w, d_rows};
  return dtype == SSQ_F32 ? pipe_exec<CwtLmsstPipe<float>>(c, s, d_x, outs, d_workspace, kernel_ms, &c.st)
                          : pipe_exec<CwtLmsstPipe<double>>(c, s, d_x, outs, d_workspace, kernel_ms, &c.st);
}

int ssq_lmssq_cwt_host(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                       const double* scales, int64_t na, double dt, const double* row_const, const double* ssq_freqs_asc,
                       int freq_kind, int64_t freq_transition, int padtype, int squeezing, double gamma, int variant,
                       int64_t work_limit_bytes, int delta, const double* row_freqs_hz, void* Tx, void* Wx, void* w,
                       int32_t* rows) {
  if (!x || !Tx || !Wx) SSQ_FAIL("NULL argument");
  const CwtLmsstCall c{{{dtype, wavelet, padtype, batch, n_signal, na, p0, p1, dt, gamma, scales, nullptr},
                        freq_kind, squeezing, variant, freq_transition, row_const, ssq_freqs_asc},
                       delta, row_freqs_hz};
  CwtMapsShape s;
  if (int rc = cwt_lmsst_check(c, &s)) return rc;
  if (int rc = cwt_host_bytes(kCwtLmsstKind, &s, batch, work_limit_bytes)) return rc;
  if (int rc = require_device()) return rc;
  const size_t el = (dtype == SSQ_F32 ? 4 : 8) * (size_t)s.plane, i32 = sizeof(int32_t) * (size_t)s.plane;
  const HostOut outs[] = {{Tx, 2 * el}, {Wx, 2 * el}, {w, el}, {rows, i32}};
  return dtype == SSQ_F32 ? cwt_pipe_host<CwtLmsstPipe<float>>(c, s, x, outs) : cwt_pipe_host<CwtLmsstPipe<double>>(c, s, x, outs);
}

int ssq_lmsst_rows_host(int dtype, const void* A, int64_t batch, int64_t n_rows, int64_t n_cols, int delta, int32_t* rows) {
  if (!A || !rows) SSQ_FAIL("NULL argument");
  if (dtype != SSQ_F32 && dtype != SSQ_F64) SSQ_FAIL("dtype must be SSQ_F32 or SSQ_F64");
  if (batch < 1) SSQ_FAIL("batch must be >= 1");
  if (n_rows < 2 || n_rows > kLmsstMaxRows) SSQ_FAIL("lmsst_rows: n_rows must be from 2 to 2049");
  if (n_cols < 1 || n_cols > (1LL << 30)) SSQ_FAIL("lmsst_rows: n_cols must be from 1 to 2^30");
  const int64_t top = n_rows - 1 < kLmsstMaxDelta ? n_rows - 1 : (int64_t)kLmsstMaxDelta;
  if (delta < 1 || delta > top) SSQ_FAIL("lmsst_rows: delta must be from 1 to min(n_rows - 1, 256)");
  if (int rc = require_device()) return rc;
  return dtype == SSQ_F32 ? lmsst_rows_typed<float>(A, batch, n_rows, n_cols, delta, rows)
                          : lmsst_rows_typed<double>(A, batch, n_rows, n_cols, delta, rows);
}

}  // extern "C"
