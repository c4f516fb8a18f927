// cwt_extract.hip -- synchroextracting and transient-extracting CWT, `upstream.set_cwt` and `upstream.tet_cwt`, orders 1
// and 2 (the CWT side of stft_extract.hip).  Upstream has neither: the definition is the
// project's own, restated in numpy by tests/helpers/extract_cwt_ref.py.  Where the rest of the family MOVES a coefficient
// to where its estimate points, these KEEP it only where the estimate says it already sits on the ridge, and zero the
// rest.  dt enters at the end.  With the maps of cwt_maps64.h on columns n1 .. n1 + N - 1, a cell live unless |W| < gamma:
//   axis 0 (SET): w = |Im om2| / (2 pi dt) where order = 2, |D| > gamma^2 and Im om2 is finite, else |Im om1| / (2 pi dt)
//                 (cwt_sst2.hip's w2; order 1: |Im om1| / (2 pi dt) on every cell, from W and W1 alone), rounded once to
//                 the call's dtype, +inf where the cell is not live;  keep where e[i+1] <= w < e[i] in the call's dtype,
//                 e [na + 1] the rows' edges, an argument (+inf, the log midpoints of the rows' frequencies in Hz, 0)
//   axis 1 (TET): tau = cwt_tsst.hip's reported offset in seconds (order 2: d2 with its fallback to d1; order 1: d1, from
//                 W and Wt alone; clamped to +- N samples), +inf where the cell is not live;  r = rint(tau / dt) in the
//                 call's dtype, cwt_maps64.h's time rule BEFORE its clip to [0, N - 1];  keep where r == 0
//   Te[i, j] = Wx[i, j] where the cell is live and kept, else +0 + 0i
// The decision is local to a cell, so the whole transform is the operator of the shared pipeline:
//   cwt_extract_kernel<O, ORDER> : one thread per (row, column), lanes along time: the M values, 1 / P, the axis's
//                              operator with the expressions of cwt2_operator_kernel / cwt_tsst_operator_kernel written
//                              out in their order, the map value rounded to the call's dtype, the keep rule on the rounded
//                              value.  Te always, Wx and the real map where asked for.  Every cell is written exactly
//                              once: no head in the workspace, nothing cleared, no scatter, no maximum (a thread past N
//                              leaves at once).  The axis is uniform over the grid: one instantiation per (dtype, order)
//                              serves both axes, the second map of either order-1 set sitting in slot 1.
// CwtExtractPipe runs it behind both doors.
#include <cmath>
#include <vector>

#include "cwt_maps64.h"

namespace ssq {

template <typename O>
struct CwtExtractDev {
  const cpx<double>* maps;   // [rows][M][P]: the unnormalised inverse transforms
  const double* nu;          // [na]: the rows' frequencies, cycles/sample (axis 1, order 2)
  const O* edges;            // [na + 1]: the rows' edges in Hz, rounded once to the call's dtype (axis 0)
  cpx<O>* Te;                // [batch * na][N], these three at the chunk's first row
  cpx<O>* Wx;                // or nullptr
  O* map;                    // or nullptr: w (axis 0) or tau (axis 1)
  long long P, N, n1, r0, rows;
  int na, axis;
  double inv_P, gamma, gamma_sq;
  double unit;               // axis 0: 1 / (2 pi dt); axis 1: dt
  O dt_o;                    // dt in the call's dtype: the time rule runs on the tau the call reports
};

// grid (ceil(N / 256), min(rows, 65535)): thread = column j of row rl
template <typename O, int ORDER>
__global__ __launch_bounds__(kCwtThreads) void cwt_extract_kernel(const CwtExtractDev<O> p) {
  using T = double;
  constexpr int M = ORDER == 2 ? 5 : 2;
  const long long j = (long long)blockIdx.x * kCwtThreads + threadIdx.x;
  if (j >= p.N) return;
  for (long long rl = blockIdx.y; rl < p.rows; rl += gridDim.y) {
    const long long r = p.r0 + rl;
    const int i = (int)(r - (r / p.na) * p.na);                             // the row's scale: uniform over the workgroup
    const cpx<T>* __restrict__ in = p.maps + rl * M * p.P + p.n1 + j;
    const cpx<T> W = cscale(in[0], p.inv_P);
    const T den = W.x * W.x + W.y * W.y;
    const T inv_den = (T)1 / den;
    const bool live = !(hypot(W.x, W.y) < p.gamma);
    O mv = (O)INFINITY;
    bool keep = false;
    if (p.axis == 0) {
      // cwt2_operator_kernel's frequency
      const cpx<T> W1 = cscale(in[p.P], p.inv_P);
      const T im1 = (W1.y * W.x - W1.x * W.y) * inv_den;                    // Im(W1 / W)
      T im = im1;
      if constexpr (ORDER == 2) {
        const cpx<T> W2 = cscale(in[2 * p.P], p.inv_P), Wt = cscale(in[3 * p.P], p.inv_P),
                     Wt1 = cscale(in[4 * p.P], p.inv_P);
        const cpx<T> D = cmul(W, W) + cmul(Wt1, W) - cmul(Wt, W1);
        const cpx<T> num = cmul(W2, W) - cmul(W1, W1);
        const cpx<T> q = {(Wt.x * W.x + Wt.y * W.y) * inv_den, (Wt.y * W.x - Wt.x * W.y) * inv_den};    // Wt / W
        const cpx<T> nr = cmul(num, q);
        const T dd = D.x * D.x + D.y * D.y;
        const T inv_dd = (T)1 / dd;
        const T im2 = im1 - (nr.y * D.x - nr.x * D.y) * inv_dd;             // Im(om1 - c Wt / W)
        if (hypot(D.x, D.y) > p.gamma_sq && isfinite(im2)) im = im2;
      }
      const O e_hi = p.edges[i], e_lo = p.edges[i + 1];                     // (per row: scalar loads)
      if (live) {
        mv = (O)(fabs(im) * p.unit);
        keep = e_lo <= mv && mv < e_hi;                                     // (a NaN is kept nowhere; +inf: e[0] = +inf)
      }
    } else {
      // cwt_tsst_operator_kernel's offset
      const cpx<T> Wt = cscale(in[(ORDER == 2 ? 3 : 1) * p.P], p.inv_P);
      T off = (Wt.x * W.x + Wt.y * W.y) * inv_den;                          // d1 = Re(Wt / W)
      if constexpr (ORDER == 2) {
        const cpx<T> W1 = cscale(in[p.P], p.inv_P), W2 = cscale(in[2 * p.P], p.inv_P), Wt1 = cscale(in[4 * p.P], p.inv_P);
        const cpx<T> D = cmul(W, W) + cmul(Wt1, W) - cmul(Wt, W1);
        const cpx<T> num = cmul(W2, W) - cmul(W1, W1);
        const cpx<T> o = {(W1.x * W.x + W1.y * W.y) * inv_den, (W1.y * W.x - W1.x * W.y) * inv_den};   // W1 / W
        const cpx<T> z = {(T)6.283185307179586 * p.nu[i] - o.y, o.x};                                  // 2 pi nu + i W1 / W
        const T nn = num.x * num.x + num.y * num.y;
        const T inv_nn = (T)1 / nn;
        const cpx<T> g = {(D.x * num.x + D.y * num.y) * inv_nn, (D.y * num.x - D.x * num.y) * inv_nn};   // D / num
        const T d2 = off - (g.x * z.y + g.y * z.x);
        if (hypot(num.x, num.y) > p.gamma_sq && isfinite(d2) && fabs(d2) <= (T)p.N) off = d2;
      }
      if (live) {
        mv = (O)(clamp_keep_nan(off, (T)p.N) * p.unit);
        if (isinf(mv)) mv = (O)INFINITY;                                    // (an offset that overflows: not a target)
        keep = rint(mv / p.dt_o) == (O)0;                                   // (NaN and +inf fail)
      }
    }
    const cpx<O> Wo = {(O)W.x, (O)W.y};
    const long long o = rl * p.N + j;
    p.Te[o] = keep ? Wo : cpx<O>{(O)0, (O)0};
    if (p.Wx) p.Wx[o] = Wo;
    if (p.map) p.map[o] = mv;
  }
}

}  // namespace ssq

using namespace ssq;

namespace {

constexpr CwtMapsKind kCwtExtractKind = {"extract_cwt", "ssq_extract_cwt_workspace_bytes", 16.0, 9.0e18, 0, 0, 0};   // no head

struct CwtExtractCall : CwtMapsCall {
  int axis, order;
  const double *nu, *edges;
};

// the maps of a row: all five (order 2), or W with W1 (axis 0) or with Wt (axis 1)
constexpr int cwt_extract_maps(int order) { return order == 2 ? 5 : 2; }

const char* cwt_extract_order_fail(int order) { return order != 1 && order != 2 ? "order must be 1 or 2" : nullptr; }
const char* cwt_extract_own_fail(int axis, int order) {
  if (axis != 0 && axis != 1) return "axis must be 0 (frequency) or 1 (time)";
  return cwt_extract_order_fail(order);
}

// Every argument check of the entry points and the shape they work on (sets the error and returns non-zero; nothing here
// touches the GPU).  The table the axis uses is required, the other may be NULL; one that is given is checked.
int cwt_extract_check(const CwtExtractCall& c, CwtMapsShape* s) {
  const std::string pre = std::string(kCwtExtractKind.name) + ": ";
  const auto rows = [&]() -> int {
    if (!c.scales || (c.axis == 1 && !c.nu) || (c.axis == 0 && !c.edges)) SSQ_FAIL("NULL argument");
    for (int64_t i = 0; i < c.na; ++i) {
      if (!(c.scales[i] > 0) || !std::isfinite(c.scales[i])) SSQ_FAIL(pre + "scales must be positive and finite");
      if (c.nu && (!(c.nu[i] > 0) || !std::isfinite(c.nu[i]))) SSQ_FAIL(pre + "row_freqs must be positive and finite");
    }
    if (c.edges) {
      for (int64_t i = 0; i <= c.na; ++i)
        if (std::isnan(c.edges[i])) SSQ_FAIL(pre + "row_edges must not hold a NaN");
      if (!(c.edges[0] == INFINITY) || c.edges[c.na] != 0.0) SSQ_FAIL(pre + "row_edges must run from +inf to 0");
      for (int64_t i = 0; i < c.na; ++i)
        if (c.edges[i + 1] > c.edges[i]) SSQ_FAIL(pre + "row_edges must not increase");
    }
    return 0;
  };
  return cwt_maps_check(kCwtExtractKind, cwt_extract_maps(c.order), cwt_extract_own_fail(c.axis, c.order), c, rows, nullptr,
                        0, nullptr, s);
}

// set_cwt / tet_cwt on device buffers (cwt_pipe_host, pipe_exec): the chunked maps with ONE operator kernel a chunk.
// kernel_ms: one part.
template <typename T>
struct CwtExtractPipe {
  static constexpr int kMid = 0;
  const CwtExtractCall& c;
  const CwtMapsShape& s;
  DeviceBufs d;
  void *scales, *nu, *edges, *work, *Te, *Wx, *map;
  int tables() {
    nu = edges = nullptr;
    SSQ_HIP(d.upload(&scales, c.scales, sizeof(double) * (size_t)c.na));
    if (c.axis == 1) SSQ_HIP(d.upload(&nu, c.nu, sizeof(double) * (size_t)c.na));
    if (c.axis == 0) {
      const std::vector<T> e(c.edges, c.edges + c.na + 1);                  // each edge rounded once to the call's dtype
      SSQ_HIP(d.upload(&edges, e.data(), sizeof(T) * e.size()));
    }
    return 0;
  }
  int bind(int64_t, void* const* outs /* Te, Wx, map */, void* wk) {
    work = wk;
    Te = outs[0];
    Wx = outs[1];
    map = outs[2];
    return 0;
  }
  template <int ORDER, unsigned MAPS>
  int run_set(const void* d_x) {
    const int64_t N = c.N;
    CwtExtractDev<T> op{};
    op.nu = static_cast<const double*>(nu);
    op.edges = static_cast<const T*>(edges);
    op.P = s.P;
    op.N = N;
    op.n1 = s.n1;
    op.na = (int)c.na;
    op.axis = c.axis;
    op.inv_P = 1.0 / (double)s.P;
    op.gamma = s.gamma;
    op.gamma_sq = s.gamma * s.gamma;
    op.unit = c.axis == 0 ? 1.0 / (6.283185307179586 * c.dt) : c.dt;
    op.dt_o = (T)c.dt;
    const auto launch_op = [&](const cpx<double>* maps, int64_t r0, int64_t nr) -> int {
      op.maps = maps;
      op.Te = static_cast<cpx<T>*>(Te) + r0 * N;
      op.Wx = Wx ? static_cast<cpx<T>*>(Wx) + r0 * N : nullptr;
      op.map = map ? static_cast<T*>(map) + r0 * N : nullptr;
      op.r0 = r0;
      op.rows = nr;
      hipLaunchKernelGGL((cwt_extract_kernel<T, ORDER>), cwt_rows_grid(N, nr), dim3(kCwtThreads), 0, c.st, op);
      SSQ_HIP(hipGetLastError());
      return 0;
    };
    return cwt_maps_chunks<T, MAPS>(c, s, d_x, scales, work, launch_op);
  }
  int run(int64_t, const void* d_x, const hipEvent_t*) {
    if (c.order == 2) return run_set<2, kMapsAll>(d_x);
    return c.axis == 0 ? run_set<1, kMapW | kMapW1>(d_x) : run_set<1, kMapW | kMapWt>(d_x);
  }
};

}  // namespace

extern "C" {

int64_t ssq_extract_cwt_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int order,
                                        int64_t* min_bytes) {
  CwtMapsShape s;
  if (cwt_maps_shape(kCwtExtractKind, cwt_extract_maps(order), cwt_extract_order_fail(order), dtype, batch, n_signal, na, &s))
    return -1;
  if (min_bytes) *min_bytes = s.min_bytes;
  return s.pref_bytes;
}

int ssq_extract_cwt_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                         const double* scales, const double* row_freqs, const double* row_edges, int64_t na, double dt,
                         int padtype, int axis, int order, double gamma, void* d_Te, void* d_Wx, void* d_map,
                         void* d_workspace, int64_t workspace_bytes, void* stream, float* kernel_ms) {
  if (!d_x || !d_Te || !d_workspace) SSQ_FAIL("NULL argument");
  const CwtExtractCall c{{dtype, wavelet, padtype, batch, n_signal, na, p0, p1, dt, gamma, scales, (hipStream_t)stream},
                         axis, order, row_freqs, row_edges};
  CwtMapsShape s;
  if (int rc = cwt_extract_check(c, &s)) return rc;
  if (int rc = cwt_exec_bytes(kCwtExtractKind, &s, workspace_bytes)) return rc;
  if (int rc = require_device()) return rc;
  void* const outs[] = {d_Te, d_Wx, d_map};
  return dtype == SSQ_F32 ? pipe_exec<CwtExtractPipe<float>>(c, s, d_x, outs, d_workspace, kernel_ms, &c.st)
                          : pipe_exec<CwtExtractPipe<double>>(c, s, d_x, outs, d_workspace, kernel_ms, &c.st);
}

int ssq_extract_cwt_host(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                         const double* scales, const double* row_freqs, const double* row_edges, int64_t na, double dt,
                         int padtype, int axis, int order, double gamma, int64_t work_limit_bytes, void* Te, void* Wx,
                         void* map) {
  if (!x || !Te) SSQ_FAIL("NULL argument");
  const CwtExtractCall c{{dtype, wavelet, padtype, batch, n_signal, na, p0, p1, dt, gamma, scales, nullptr},
                         axis, order, row_freqs, row_edges};
  CwtMapsShape s;
  if (int rc = cwt_extract_check(c, &s)) return rc;
  if (int rc = cwt_host_bytes(kCwtExtractKind, &s, batch, work_limit_bytes)) return rc;
  if (int rc = require_device()) return rc;
  const size_t el = (dtype == SSQ_F32 ? 4 : 8) * (size_t)s.plane;
  const HostOut outs[] = {{Te, 2 * el}, {Wx, 2 * el}, {map, el}};
  return dtype == SSQ_F32 ? cwt_pipe_host<CwtExtractPipe<float>>(c, s, x, outs)
                          : cwt_pipe_host<CwtExtractPipe<double>>(c, s, x, outs);
}

}  // extern "C"
