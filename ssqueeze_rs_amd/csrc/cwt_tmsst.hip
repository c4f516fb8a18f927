// cwt_tmsst.hip -- time-reassigned multisynchrosqueezed CWT, `upstream.tmssq_cwt`, orders 1 and 2 (the
// iteration of Yu, Lin, Ma and He 2020 on the time map of tssq_cwt).  Upstream has no such transform: the definition is
// the project's own, restated in numpy by tests/helpers/tmssq_cwt_ref.py.  Everything up to the one-step target is
// tssq_cwt's (cwt_tsst.hip).  Per row, with t[j] the one-step target column of column j (-1 where |W| < gamma):
//   c1[j] = t[j];   c(k+1)[j] = t[ck[j]] if t[ck[j]] is kept, else ck[j]                        (k = 1 .. n_iter - 1)
//   Tx[i, c_n[j]] += Wx[i, j] exp(-2 pi i frac(nu_i (j - c_n[j])))                               kept j
// tssq_cwt clamps its offset to +-N, not to a window: a target may lie anywhere in the row, so a chain cannot be kept
// inside a staged halo as stft_tmsst.hip's is.
//
//   cwt_tsst_operator_kernel : cwt_tsst.hip's, as it is (cwtt_operator_run): Wx, tau and the int32 one-step plane.
//   cwt_tmsst_walk_kernel    : a workgroup of 256 owns a tile of kCwtWalkTile columns of one row and stages the one-step
//                              targets of the columns within kCwtWalkHalo of it in LDS, along time.  After one barrier
//                              every thread walks its columns n_iter - 1 steps: a step whose column lies inside the
//                              stage reads LDS, any other reads the one-step plane in device memory (read-only during
//                              the launch: no ordering is needed).  A chain ends early on a fixed point and on a column
//                              that is not kept.  Every read, LDS or global, is behind (unsigned)c < N.  Tiles read each
//                              other's entries, so the walk writes a SECOND int32 plane, never in place.
//   cwt_tsst_scatter_kernel, cwt_tsst_readout_kernel : cwt_tsst.hip's, as they are (cwtt_scatter_run), on the walked plane.
// The head of the workspace: tssq_cwt's (maxima, accumulators, the one-step plane) and the walked plane behind it.
// CwtTmPipe runs the three stages behind both doors.
#include <cmath>
#include <vector>

#include "cwt_tsst.h"

namespace ssq {

constexpr int kCwtWalkMaxIter = 64;
constexpr int kCwtWalkThreads = 256;
constexpr int kCwtWalkTile = 2048;         // columns of one workgroup
constexpr int kCwtWalkHalo = 256;          // columns staged on either side of the tile
constexpr int kCwtWalkStage = kCwtWalkTile + 2 * kCwtWalkHalo;        // 10 KB of int32

// in, out: [rows][n] int32 absolute targets (-1: not kept), rows = batch x na folded; grid (ceil(n / tile), rows <= 65535).
// A column c outside 0 .. n - 1 is never used as an index: the chain stops on it (the operator clips its targets and the
// host entry checks a caller's map, so it cannot happen on either).
__global__ __launch_bounds__(kCwtWalkThreads) void cwt_tmsst_walk_kernel(const int* __restrict__ in, int* __restrict__ out,
                                                                         int n, int n_iter) {
  __shared__ int tgt_s[kCwtWalkStage];
  const long long base = (long long)blockIdx.y * n;
  const int* __restrict__ row = in + base;
  const int t0 = (int)blockIdx.x * kCwtWalkTile;               // t0 < n <= 2^30
  const int t1 = n - t0 < kCwtWalkTile ? n : t0 + kCwtWalkTile;
  const int s0 = t0 > kCwtWalkHalo ? t0 - kCwtWalkHalo : 0;
  const int s1 = n - t1 < kCwtWalkHalo ? n : t1 + kCwtWalkHalo;
  const int ns = s1 - s0;                                     // <= kCwtWalkStage
  for (int i = threadIdx.x; i < ns; i += kCwtWalkThreads) tgt_s[i] = row[s0 + i];
  __syncthreads();
  for (int j = t0 + threadIdx.x; j < t1; j += kCwtWalkThreads) {
    int c = tgt_s[j - s0];
    if (c >= 0) {
      for (int i = 1; i < n_iter; ++i) {
        if ((unsigned)c >= (unsigned)n) break;
        const unsigned rel = (unsigned)(c - s0);               // (wraps above ns for c < s0)
        const int nxt = rel < (unsigned)ns ? tgt_s[rel] : row[c];
        if (nxt < 0 || nxt == c) break;                        // not kept, or a fixed point: the chain stops
        c = nxt;
      }
    } else {
      c = -1;
    }
    out[base + j] = c;
  }
}

// the walk of `rows` rows of n columns on device buffers, asynchronous on `st`
hipError_t cwt_tmsst_walk_run(const int* d_in, int* d_out, long long rows, long long n, int n_iter, hipStream_t st) {
  if (n < 1 || n > (1LL << 30) || rows < 1 || n_iter < 1) return hipErrorInvalidValue;
  const unsigned tiles = (unsigned)((n + kCwtWalkTile - 1) / kCwtWalkTile);
  for (long long r0 = 0; r0 < rows; r0 += 65535) {
    const long long n1 = rows - r0 < 65535 ? rows - r0 : 65535;
    hipLaunchKernelGGL(cwt_tmsst_walk_kernel, dim3(tiles, (unsigned)n1), dim3(kCwtWalkThreads), 0, st, d_in + r0 * n,
                       d_out + r0 * n, (int)n, n_iter);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace ssq

using namespace ssq;

namespace {

// the head: 16 bytes of accumulator and two int32 planes (the one-step targets, the walked ones) per cell
constexpr CwtMapsKind kCwtTmKind = {"tmssq_cwt", "ssq_tmssq_cwt_workspace_bytes", 24.0, 4.0e18, 0, 16, 2};

struct CwtTmCall : CwtTCall {
  int n_iter;
};

const char* cwttm_own_fail(int order, int n_iter) {
  if (const char* f = cwtt_order_fail(order)) return f;
  return n_iter < 1 || n_iter > kCwtWalkMaxIter ? "n_iter must be from 1 to 64" : nullptr;
}

// tmssq_cwt on device buffers (cwt_pipe_host, pipe_exec): the operator part, the walk, the scatter with its read-out.  At
// n_iter 1 there is no walk and the operator's plane is the final one: the caller's if given, else the head's first.
// Else the operator writes the head's first plane and the walk the caller's plane, or the head's second.  kernel_ms: four
// parts, the events after the operator part, after the walk and after the scatter kernel.
template <typename T>
struct CwtTmPipe {
  static constexpr int kMid = 3;
  const CwtTmCall& c;
  const CwtMapsShape& s;
  DeviceBufs d;
  void *scales, *nu, *work, *Tx, *Wx, *tau;
  int *one, *last;
  int tables() { return cwtt_tables(d, c, &scales, &nu); }
  int bind(int64_t, void* const* outs /* Tx, Wx, tau, mm */, void* wk) {
    work = wk;
    Tx = outs[0];
    Wx = outs[1];
    tau = outs[2];
    int* given = static_cast<int*>(outs[3]);
    int* head = cwt_head_at<int>(work, s.head.planes);
    one = c.n_iter == 1 && given ? given : head;
    last = c.n_iter == 1 ? one : (given ? given : head + s.cells);
    return 0;
  }
  int run(int64_t, const void* d_x, const hipEvent_t* mid) {
    if (int rc = cwtt_operator_run<T>(c, s, d_x, scales, nu, Wx, tau, one, work)) return rc;
    if (mid[0]) SSQ_HIP(hipEventRecord(mid[0], c.st));
    if (c.n_iter > 1) SSQ_HIP(cwt_tmsst_walk_run(one, last, (long long)s.rows, (long long)c.N, c.n_iter, c.st));
    if (mid[1]) SSQ_HIP(hipEventRecord(mid[1], c.st));
    return cwtt_scatter_run<T>(c, s, nu, Wx, last, work, Tx, mid[2]);
  }
};

}  // namespace

extern "C" {

int64_t ssq_tmssq_cwt_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int order, int64_t* min_bytes) {
  CwtMapsShape s;
  if (cwt_maps_shape(kCwtTmKind, cwt_tsst_maps(order), cwtt_order_fail(order), dtype, batch, n_signal, na, &s)) return -1;
  if (min_bytes) *min_bytes = s.min_bytes;
  return s.pref_bytes;
}

int ssq_tmssq_cwt_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                       const double* scales, const double* row_freqs, int64_t na, double dt, int padtype, int order,
                       double gamma, int n_iter, void* d_Tx, void* d_Wx, void* d_tau, void* d_mm, void* d_workspace,
                       int64_t workspace_bytes, void* stream, float* kernel_ms) {
  if (!d_x || !d_Tx || !d_Wx || !d_workspace) SSQ_FAIL("NULL argument");
  const CwtTmCall c{{{dtype, wavelet, padtype, batch, n_signal, na, p0, p1, dt, gamma, scales, (hipStream_t)stream},
                     order, row_freqs}, n_iter};
  CwtMapsShape s;
  if (int rc = cwtt_check(kCwtTmKind, cwttm_own_fail(order, n_iter), c, &s)) return rc;
  if (int rc = cwt_exec_bytes(kCwtTmKind, &s, workspace_bytes)) return rc;
  if (int rc = require_device()) return rc;
  void* const outs[] = {d_Tx, d_Wx, d_tau, d_mm};
  float part[4], *ms = kernel_ms ? part : nullptr;
  const int rc = dtype == SSQ_F32 ? pipe_exec<CwtTmPipe<float>>(c, s, d_x, outs, d_workspace, ms, &c.st)
                                  : pipe_exec<CwtTmPipe<double>>(c, s, d_x, outs, d_workspace, ms, &c.st);
  if (rc == 0 && kernel_ms) {
    kernel_ms[0] = part[0] + part[1] + part[2] + part[3];      // all the kernels
    for (int i = 0; i < 3; ++i) kernel_ms[1 + i] = part[i];    // the operator part, the walk, the scatter kernel
  }
  return rc;
}

int ssq_tmssq_cwt_host(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                       const double* scales, const double* row_freqs, int64_t na, double dt, int padtype, int order,
                       double gamma, int n_iter, int64_t work_limit_bytes, void* Tx, void* Wx, void* tau, void* mm) {
  if (!x || !Tx || !Wx) SSQ_FAIL("NULL argument");
  const CwtTmCall c{{{dtype, wavelet, padtype, batch, n_signal, na, p0, p1, dt, gamma, scales, nullptr},
                     order, row_freqs}, n_iter};
  CwtMapsShape s;
  if (int rc = cwtt_check(kCwtTmKind, cwttm_own_fail(order, n_iter), c, &s)) return rc;
  if (int rc = cwt_host_bytes(kCwtTmKind, &s, batch, work_limit_bytes)) return rc;
  if (int rc = require_device()) return rc;
  const size_t el = (dtype == SSQ_F32 ? 4 : 8) * (size_t)s.plane;
  const HostOut outs[] = {{Tx, 2 * el}, {Wx, 2 * el}, {tau, el}, {mm, sizeof(int32_t) * (size_t)s.plane}};
  return dtype == SSQ_F32 ? cwt_pipe_host<CwtTmPipe<float>>(c, s, x, outs) : cwt_pipe_host<CwtTmPipe<double>>(c, s, x, outs);
}

int ssq_tmssq_cwt_tile_cols(int* halo) {
  if (halo) *halo = kCwtWalkHalo;
  return kCwtWalkTile;
}

int ssq_tmssq_cwt_walk_host(const int32_t* targets_in, int64_t batch, int64_t n_rows, int64_t n_cols, int n_iter,
                            int32_t* targets_out) {
  if (!targets_in || !targets_out) SSQ_FAIL("NULL argument");
  if (batch < 1 || n_rows < 1) SSQ_FAIL("tmssq_cwt_walk: batch and n_rows must be >= 1");
  if (n_cols < 1 || n_cols > (1LL << 30)) SSQ_FAIL("tmssq_cwt_walk: n_cols must be from 1 to 2^30");
  if (n_iter < 1 || n_iter > kCwtWalkMaxIter) SSQ_FAIL("tmssq_cwt_walk: n_iter must be from 1 to 64");
  if ((double)batch * (double)n_rows * (double)n_cols > 1.0e18) SSQ_FAIL("tmssq_cwt_walk: map too large");
  const size_t map_sig = (size_t)n_rows * (size_t)n_cols;
  for (size_t i = 0; i < map_sig * (size_t)batch; ++i)
    if (targets_in[i] < -1 || targets_in[i] >= n_cols) SSQ_FAIL("tmssq_cwt_walk: a target lies outside -1 .. n_cols - 1");
  if (int rc = require_device()) return rc;
  const size_t map_bytes = sizeof(int32_t) * map_sig;
  const HostOut outs[] = {{targets_out, map_bytes}};
  int* d_out = nullptr;
  return host_sliced(                                          // no workspace: the map in, the walked map out
      batch, host_slice(batch, map_bytes, outs, 0), targets_in, map_bytes, outs,
      [&](int64_t, void* const* o, void*) {
        d_out = static_cast<int*>(o[0]);
        return 0;
      },
      [&](int64_t nb, const void* d_in) -> int {
        // (n_iter 1 too: the entry point runs the kernel, which then copies the map)
        SSQ_HIP(cwt_tmsst_walk_run((const int*)d_in, d_out, (long long)nb * n_rows, (long long)n_cols, n_iter, nullptr));
        return 0;
      });
}

}  // extern "C"
