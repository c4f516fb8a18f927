// cwt_sst2.hip -- second-order ("vertical") synchrosqueezed CWT, `upstream.ssq_cwt2` (Oberlin and Meignen
// 2017, restated for frequency-domain tables).  Upstream has no such transform: the definition is the project's own,
// restated in numpy by tests/helpers/cwt_sst2_ref.py.  dt enters at the end.  With the five maps of cwt_maps64.h:
//   D = W^2 + Wt1 W - Wt W1      c = (W2 W - W1^2) / D      om1 = W1 / W      om2 = om1 - c Wt / W
//   w2 = |Im om2| / (2 pi dt) where |D| > gamma^2 and Im om2 is finite, else |Im om1| / (2 pi dt) (ssq_cwt's w);
//   +inf where |W| < gamma (phase_one's rule, ssqueeze.hip).
// The pipeline up to the operator is cwt_maps64.h's.  Then:
//   cwt2_operator_kernel  one thread per (row, column), lanes along time: the five values, 1 / P, the operator with
//                         1 / |W|^2 and 1 / |D|^2 formed once, Wx and w2 out in the call's dtype.
//   ssq_ssqueeze_w_exec   the deterministic scatter of Wx under w2 (rows ascending, no atomics) into Tx.
// Wx and w2 are rounded once on store, the scatter runs in the call's dtype on the rounded values, so Tx is the scatter
// of what the call reports.  A first version with no time target (DESIGN 4.12 has the cost).  cwt_msst.hip (mssq_cwt)
// runs both halves of this file, the operator half and the squeeze half, through cwt_sst2.h, with its walk kernel
// between them; ssq_cwt2's pipe (Cwt2Pipe, behind both of its doors) runs the same two halves one after the other.
#include <cmath>
#include <vector>

#include "cwt_sst2.h"

namespace ssq {

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
__global__ __launch_bounds__(kCwtThreads) void cwt2_operator_kernel(const Cwt2OpDev<O> p) {
  using T = double;
  const long long j = (long long)blockIdx.x * kCwtThreads + threadIdx.x;
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

int cwt2_check(const CwtMapsKind& k, const char* own_fail, const Cwt2Call& c, CwtMapsShape* s) {
  const std::string pre = std::string(k.name) + ": ";
  const auto rows = [&]() -> int {
    if (!c.scales || !c.row_const || !c.f_asc) SSQ_FAIL("NULL argument");
    for (int64_t i = 0; i < c.na; ++i) {
      if (!(c.scales[i] > 0) || !std::isfinite(c.scales[i])) SSQ_FAIL(pre + "scales must be positive and finite");
      if (!std::isfinite(c.row_const[i])) SSQ_FAIL(pre + "row_const must be finite");
      if (!std::isfinite(c.f_asc[i])) SSQ_FAIL(pre + "ssq_freqs_asc must be finite");
    }
    return 0;
  };
  const bool sq_ok = c.squeezing == SSQ_SQUEEZE_SUM || c.squeezing == SSQ_SQUEEZE_LEBESGUE;
  return cwt_maps_check(k, kCwt2Maps, own_fail, c, rows, &c.freq_kind, c.freq_transition,
                        sq_ok ? nullptr : "squeezing must be 'sum' or 'lebesgue'", s);
}

template <typename T>
int cwt2_tables(DeviceBufs& d, const Cwt2Call& c, void** d_scales, void** d_rc) {
  SSQ_HIP(d.upload(d_scales, c.scales, sizeof(double) * (size_t)c.na));
  const std::vector<T> rc(c.row_const, c.row_const + c.na);
  SSQ_HIP(d.upload(d_rc, rc.data(), sizeof(T) * (size_t)c.na));
  return 0;
}

template <typename T>
int cwt2_operator_run(const Cwt2Call& c, const CwtMapsShape& s, double gamma_sq, const void* d_x, const void* d_scales,
                      void* d_Wx, void* d_w2, void* d_work) {
  const int64_t N = c.N;
  Cwt2OpDev<T> op{};
  op.P = s.P;
  op.N = N;
  op.n1 = s.n1;
  op.inv_P = 1.0 / (double)s.P;
  op.gamma = s.gamma;
  op.gamma_sq = gamma_sq;
  op.inv_two_pi_dt = 1.0 / (6.283185307179586 * c.dt);
  const auto launch_op = [&](const cpx<double>* maps, int64_t r0, int64_t nr) -> int {
    op.maps = maps;
    op.Wx = static_cast<cpx<T>*>(d_Wx) + r0 * N;
    op.w2 = static_cast<T*>(d_w2) + r0 * N;
    op.rows = nr;
    hipLaunchKernelGGL((cwt2_operator_kernel<T>), cwt_rows_grid(N, nr), dim3(kCwtThreads), 0, c.st, op);
    SSQ_HIP(hipGetLastError());
    return 0;
  };
  return cwt_maps_chunks<T, kMapsAll>(c, s, d_x, d_scales, d_work, launch_op);
}

int cwt2_squeeze_run(const Cwt2Call& c, const void* d_Wx, const void* d_w, const void* d_rc, void* d_Tx) {
  return ssq_ssqueeze_w_exec(c.dtype, d_Wx, d_w, c.batch, c.na, c.N, d_rc, c.f_asc, c.freq_kind, c.freq_transition,
                             c.squeezing, (c.variant & SSQ_VARIANT_FLIPUD) ? 1 : 0, d_Tx, c.st);
}

template int cwt2_tables<float>(DeviceBufs&, const Cwt2Call&, void**, void**);
template int cwt2_tables<double>(DeviceBufs&, const Cwt2Call&, void**, void**);
template int cwt2_operator_run<float>(const Cwt2Call&, const CwtMapsShape&, double, const void*, const void*, void*, void*,
                                      void*);
template int cwt2_operator_run<double>(const Cwt2Call&, const CwtMapsShape&, double, const void*, const void*, void*, void*,
                                       void*);

}  // namespace ssq

using namespace ssq;

namespace {

constexpr CwtMapsKind kCwt2Kind = {"ssq_cwt2", "ssq_ssq_cwt2_workspace_bytes", 16.0, 9.0e18, 0, 0, 0};   // no head

// ssq_cwt2 on device buffers (cwt_pipe_host, pipe_exec): the two halves, one after the other.  kernel_ms: one part.
template <typename T>
struct Cwt2Pipe {
  static constexpr int kMid = 0;
  const Cwt2Call& c;
  const CwtMapsShape& s;
  DeviceBufs d;
  void *scales, *rc, *Tx, *Wx, *w2, *work;
  int tables() { return cwt2_tables<T>(d, c, &scales, &rc); }
  int bind(int64_t, void* const* outs /* Tx, Wx, w2 */, void* wk) {
    Tx = outs[0];
    Wx = outs[1];
    work = wk;
    if (!(w2 = outs[2])) SSQ_HIP(d.alloc(&w2, sizeof(T) * (size_t)s.cells));   // (the host door without w2: the squeeze reads it)
    return 0;
  }
  int run(int64_t, const void* d_x, const hipEvent_t*) {
    if (int r = cwt2_operator_run<T>(c, s, s.gamma * s.gamma, d_x, scales, Wx, w2, work)) return r;
    return cwt2_squeeze_run(c, Wx, w2, rc, Tx);
  }
};

}  // namespace

extern "C" {

int64_t ssq_ssq_cwt2_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int64_t* min_bytes) {
  CwtMapsShape s;
  if (cwt_maps_shape(kCwt2Kind, kCwt2Maps, nullptr, dtype, batch, n_signal, na, &s)) return -1;
  if (min_bytes) *min_bytes = s.min_bytes;
  return s.pref_bytes;
}

int ssq_ssq_cwt2_tables(int wavelet, double p0, double p1, double scale, int64_t P, double* T0, double* T1) {
  if (!T0 || !T1) SSQ_FAIL("NULL argument");
  if (int rc = cwt_wavelet_check("ssq_cwt2: ", wavelet, p0, p1)) return rc;
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
  const Cwt2Call c{{dtype, wavelet, padtype, batch, n_signal, na, p0, p1, dt, gamma, scales, (hipStream_t)stream},
                   freq_kind, squeezing, variant, freq_transition, row_const, ssq_freqs_asc};
  CwtMapsShape s;
  if (int rc = cwt2_check(kCwt2Kind, nullptr, c, &s)) return rc;
  if (int rc = cwt_exec_bytes(kCwt2Kind, &s, workspace_bytes)) return rc;
  if (int rc = require_device()) return rc;
  void* const outs[] = {d_Tx, d_Wx, d_w2};
  return dtype == SSQ_F32 ? pipe_exec<Cwt2Pipe<float>>(c, s, d_x, outs, d_workspace, kernel_ms, &c.st)
                          : pipe_exec<Cwt2Pipe<double>>(c, s, d_x, outs, d_workspace, kernel_ms, &c.st);
}

int ssq_ssq_cwt2_host(int dtype, const void* x, int64_t batch, int64_t n_signal, int wavelet, double p0, double p1,
                      const double* scales, int64_t na, double dt, const double* row_const, const double* ssq_freqs_asc,
                      int freq_kind, int64_t freq_transition, int padtype, int squeezing, double gamma, int variant,
                      int64_t work_limit_bytes, void* Tx, void* Wx, void* w2) {
  if (!x || !Tx || !Wx) SSQ_FAIL("NULL argument");
  const Cwt2Call c{{dtype, wavelet, padtype, batch, n_signal, na, p0, p1, dt, gamma, scales, nullptr},
                   freq_kind, squeezing, variant, freq_transition, row_const, ssq_freqs_asc};
  CwtMapsShape s;
  if (int rc = cwt2_check(kCwt2Kind, nullptr, c, &s)) return rc;
  if (int rc = cwt_host_bytes(kCwt2Kind, &s, batch, work_limit_bytes)) return rc;
  if (int rc = require_device()) return rc;
  const size_t el = (dtype == SSQ_F32 ? 4 : 8) * (size_t)s.plane;
  const HostOut outs[] = {{Tx, 2 * el}, {Wx, 2 * el}, {w2, el}};
  return dtype == SSQ_F32 ? cwt_pipe_host<Cwt2Pipe<float>>(c, s, x, outs) : cwt_pipe_host<Cwt2Pipe<double>>(c, s, x, outs);
}

}  // extern "C"
