// cwt_conceft.hip -- ConceFT, the multitaper synchrosqueezed CWT, `upstream.conceft_cwt` (Daubechies, Wang
// and Wu 2016).  Upstream has no such transform: the definition is the project's own, restated in numpy by
// tests/helpers/conceft_ref.py.  With W_g, dW_g the transform and its derivative for the GMW of order k_g (g < J: the
// planes of `cwt_higher_order(..., average=False, derivative=True)`) and M unit vectors r_m in C^J, gauged by the caller
// so that c_m = sum_g r_mg C_{k_g} > 0 (C_k: the order's admittance, `upstream.gmw_adm_ssq`):
//   W^(m)  = sum_g r_mg W_g,  dW^(m) = sum_g r_mg dW_g      g ascending, in the call's dtype
//   k      = the bin of ssq_cwt's rule on (W^(m), dW^(m)): reassign_bin_upstream / _pw of cwt_bin.h, |W^(m)| > gamma
//   Tx[k, n] += W^(m)[i, n] row_const[i] C_0 / sum_m c_m
// Stage 1: the 2 J planes of a slice of signals through the plan of `cwt_higher_order` (ssq_cwt_plan_create_gmwk, J
// polynomial groups, one forward FFT per signal), into the caller's workspace.
// Stage 2, cwt_conceft_kernel: one thread owns a column of one signal (lanes along time: every load and store is
// coalesced) and is the only writer of that column of Tx; no atomics.  The draws go in chunks of kConceftDraws = 8.  For
// a chunk the thread walks the rows upward; per row it loads the 2 J coefficients once, forms the chunk's combinations in
// registers (the vectors are read with wave-uniform addresses: scalar loads), runs the bin rule of all the chunk's draws
// (side by side: eight independent chains) and then keeps a (current bin, complex sum) pair per draw: a run of rows that lands in one bin is summed in registers and added to Tx
// by one plain read-modify-write when that draw's bin changes, as cwt_reassign_rows_kernel combines runs.  The order of
// the additions into a cell is therefore fixed by the column alone: chunks ascending, rows ascending within a chunk,
// draws ascending within a row, each addition the finished run of one draw.  It depends neither on the batch, nor on
// the slices of the workspace, nor on the launch geometry.  More draws re-read the planes once per chunk (from L2 / the
// Infinity Cache: a slice's planes are what stage 1 just wrote); the arithmetic of the M phase transforms dominates.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ssq_hip.h"
#include "bin_rule.h"
#include "cwt_bin.h"
#include "cwt_kernels.h"
#include "dev_buffers.h"

namespace ssq {

// draws per register chunk (the register budget, profiles/conceft_resources.txt): 8 for both dtypes.
// float32: 89 VGPRs, 5 waves a SIMD; float64: 162 / 164 VGPRs, 3 waves a SIMD; no scratch.  4 draws in float64 (104
// VGPRs, 4 waves a SIMD) was measured 16 % SLOWER: the kernel is bound by the dependent arithmetic of the bin rule,
// which more draws side by side hide and more waves do not, and a smaller chunk re-reads the planes more often.
constexpr int kConceftDraws = 8;
constexpr int kConceftMaxOrders = 8;    // upstream.CONCEFT_MAX_ORDERS
constexpr int kConceftMaxDraws = 256;   // upstream.CONCEFT_MAX_DRAWS

template <typename T>
struct ConceftDev {
  const cpx<T>* W;       // [signals][J][na][N]
  const cpx<T>* dW;      // [signals][J][na][N]
  T* w;                  // [signals][M][na][N] or nullptr: the phase transform of every draw, +inf where not kept
  long long signals;
  int J, M;
  CwtSsqDev<T> q;        // N, na, the bin rule, gamma, flipud; Tx [signals][na][N], zero on entry
  CwtRowsDev<T> r;       // the log-piecewise segment (row_const: the kernel's own argument)
};

// One chunk of draws on one column: the walk up the rows.  FULL: the chunk holds kConceftDraws draws and the draw loops
// carry no guard.  Per row the bins of all the draws are formed first, free of the flushes' branches, so that the
// compiler interleaves the draws' independent chains of dependent arithmetic (the bin rule is one long chain: a
// hypot, an IEEE division and a log2); the run logic follows, draws ascending.
template <typename T, bool PW, bool FULL>
__device__ __forceinline__ void conceft_chunk(const ConceftDev<T>& p, const cpx<T>* __restrict__ vec,
                                              const T* __restrict__ row_const, const cpx<T>* __restrict__ Wb,
                                              const cpx<T>* __restrict__ dWb, cpx<T>* __restrict__ Tb,
                                              T* __restrict__ wb, int mc) {
  constexpr int MC = kConceftDraws;
  const long long N = p.q.N;
  const int na = p.q.na;
  const long long plane = (long long)na * N;
  int k_cur[MC];
  cpx<T> acc[MC];
#pragma unroll
  for (int m = 0; m < MC; ++m) {
    k_cur[m] = -1;
    acc[m] = {(T)0, (T)0};
  }
  auto flush = [&](int k, cpx<T> a) {
    if (k < 0) return;
    cpx<T>* d = Tb + (long long)k * N;
    cpx<T> t = *d;
    t.x += a.x;
    t.y += a.y;
    *d = t;
  };
  for (int i = 0; i < na; ++i) {
    cpx<T> Wm[MC], dWm[MC];
#pragma unroll
    for (int m = 0; m < MC; ++m) {
      Wm[m] = {(T)0, (T)0};
      dWm[m] = {(T)0, (T)0};
    }
    for (int g = 0; g < p.J; ++g) {
      const long long o = ((long long)g * na + i) * N;
      const cpx<T> a = Wb[o], d = dWb[o];
#pragma unroll
      for (int m = 0; m < MC; ++m) {
        if (FULL || m < mc) {                              // (wave-uniform: the last chunk may be short)
          const cpx<T> v = vec[m * p.J + g];               // four fused multiply-adds a product, g ascending
          Wm[m].x = fma(-v.y, a.y, fma(v.x, a.x, Wm[m].x));
          Wm[m].y = fma(v.y, a.x, fma(v.x, a.y, Wm[m].y));
          dWm[m].x = fma(-v.y, d.y, fma(v.x, d.x, dWm[m].x));
          dWm[m].y = fma(v.y, d.x, fma(v.x, d.y, dWm[m].y));
        }
      }
    }
    int kk[MC];
    T w[MC];
#pragma unroll
    for (int m = 0; m < MC; ++m) {
      kk[m] = -1;
      w[m] = (T)INFINITY;
      if (FULL || m < mc)
        kk[m] = PW ? reassign_bin_upstream_pw(p.q, p.r, Wm[m], dWm[m], w[m]) : reassign_bin_upstream(p.q, Wm[m], dWm[m], w[m]);
    }
    const T c = row_const[i];
#pragma unroll
    for (int m = 0; m < MC; ++m) {
      if (FULL || m < mc) {
        if (wb) wb[(long long)m * plane + (long long)i * N] = w[m];
        if (kk[m] != k_cur[m]) {
          flush(k_cur[m], acc[m]);
          k_cur[m] = kk[m];
          acc[m] = {(T)0, (T)0};
        }
        if (kk[m] >= 0) {
          acc[m].x += Wm[m].x * c;
          acc[m].y += Wm[m].y * c;
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MC; ++m)
    if (FULL || m < mc) flush(k_cur[m], acc[m]);
}

// grid (ceil(N / 64), min(signals, 65535)), block 64: thread = column j, the y blocks stride over the signals.
// vectors [M][J], the gauged unit vectors, and row_const [na] (times C_0 / sum c_m) are arguments of their own: const
// and restrict there, and indexed by wave-uniform values, so the compiler reads them through the scalar cache.
template <typename T, bool PW>
__global__ __launch_bounds__(64) void cwt_conceft_kernel(const ConceftDev<T> p, const cpx<T>* __restrict__ vectors,
                                                         const T* __restrict__ row_const) {
  constexpr int MC = kConceftDraws;
  const long long N = p.q.N;
  const long long j = (long long)blockIdx.x * 64 + threadIdx.x;
  if (j >= N) return;
  const long long plane = (long long)p.q.na * N;
  for (long long b = blockIdx.y; b < p.signals; b += gridDim.y) {
    const cpx<T>* __restrict__ Wb = p.W + b * p.J * plane + j;
    const cpx<T>* __restrict__ dWb = p.dW + b * p.J * plane + j;
    cpx<T>* __restrict__ Tb = p.q.Tx + b * plane + j;
    for (int m0 = 0; m0 < p.M; m0 += MC) {
      const int mc = (p.M - m0 < MC) ? p.M - m0 : MC;
      const cpx<T>* __restrict__ vec = vectors + (long long)m0 * p.J;
      T* __restrict__ wb = p.w ? p.w + (b * p.M + m0) * plane + j : nullptr;
      if (mc == MC) conceft_chunk<T, PW, true>(p, vec, row_const, Wb, dWb, Tb, wb, mc);
      else conceft_chunk<T, PW, false>(p, vec, row_const, Wb, dWb, Tb, wb, mc);
    }
  }
}

}  // namespace ssq

using namespace ssq;

namespace {

struct ConceftCall {
  int dtype;
  int64_t batch, N;
  double gmw_gamma, gmw_beta;
  const double* coeffs;       // [J][n_coeffs]
  int64_t n_coeffs, J;
  const double* vectors;      // [M][J] complex (interleaved)
  int64_t M;
  double scale;
  const double* scales;
  int64_t na;
  double dt;
  const double* row_const;
  const double* f_asc;
  int freq_kind;
  int64_t freq_transition;
  int padtype;
  double gamma;
  int variant;
  hipStream_t st;             // of the launches (the host door: the null stream)
  float* ms;                  // the exec door's kernel_ms (ConceftPipe), or nullptr
};

struct ConceftShape {
  int64_t plane;              // na N
  int64_t signal_bytes;       // the 2 J planes of one signal, to a multiple of 256 bytes
  int64_t min_bytes, pref_bytes;
  int64_t work_bytes = 0;     // of the workspace the call runs in (the doors set it): sets the signals per inner slice
  ssq_cwt_plan* plan = nullptr;   // conceft_plan's, the door's for the length of the call
  int64_t plan_bytes = 0;     // the plan's own workspace
};

constexpr int64_t kConceftPrefBytes = (int64_t)1 << 30;   // the preferred workspace: whole signals up to 1 GiB

int conceft_shape(int dtype, int64_t batch, int64_t N, int64_t na, int64_t J, ConceftShape* s) {
  if (dtype != SSQ_F32 && dtype != SSQ_F64) SSQ_FAIL("conceft_cwt: dtype must be SSQ_F32 or SSQ_F64");
  if (batch < 1) SSQ_FAIL("conceft_cwt: batch must be >= 1");
  if (N < 1 || N > INT32_MAX) SSQ_FAIL("conceft_cwt: n_signal must be in [1, 2^31)");
  if (na < 2) SSQ_FAIL("conceft_cwt: at least 2 scales");
  if (J < 1 || J > kConceftMaxOrders) SSQ_FAIL("conceft_cwt: n_orders must be 1 .. " + std::to_string(kConceftMaxOrders));
  if (na * J > 32767) SSQ_FAIL("conceft_cwt: na * n_orders above 32767 rows");
  const double csz = dtype == SSQ_F32 ? 8.0 : 16.0;
  if ((double)batch * (double)kConceftMaxDraws * (double)na * (double)N * csz > 9.0e18) SSQ_FAIL("conceft_cwt: transform too large");
  s->plane = na * N;
  s->signal_bytes = (2 * J * s->plane * (int64_t)csz + 255) / 256 * 256;
  s->min_bytes = s->signal_bytes;
  const int64_t fit = std::max<int64_t>(1, kConceftPrefBytes / s->signal_bytes);
  s->pref_bytes = s->signal_bytes * std::min(batch, fit);
  return 0;
}

int conceft_check(const ConceftCall& c, ConceftShape* s) {
  if (int rc = conceft_shape(c.dtype, c.batch, c.N, c.na, c.J, s)) return rc;
  if (!c.coeffs || !c.vectors || !c.scales || !c.row_const || !c.f_asc) SSQ_FAIL("conceft_cwt: NULL argument");
  if (c.M < 1 || c.M > kConceftMaxDraws) SSQ_FAIL("conceft_cwt: n_draws must be 1 .. " + std::to_string(kConceftMaxDraws));
  if (c.n_coeffs < 1 || c.n_coeffs > kGmwMaxOrder + 1)
    SSQ_FAIL("conceft_cwt: n_coeffs must be 1 .. " + std::to_string(kGmwMaxOrder + 1));
  if (!(c.gmw_gamma > 0) || !(c.gmw_beta > 0) || !std::isfinite(c.gmw_gamma) || !std::isfinite(c.gmw_beta))
    SSQ_FAIL("conceft_cwt: the GMW parameters must be positive and finite");
  if (!(c.dt > 0) || !std::isfinite(c.dt)) SSQ_FAIL("conceft_cwt: dt must be positive and finite");
  if (c.padtype < SSQ_PAD_REFLECT || c.padtype > SSQ_PAD_WRAP) SSQ_FAIL("conceft_cwt: padtype must be SSQ_PAD_* (0 .. 4)");
  if (c.gamma != c.gamma) SSQ_FAIL("conceft_cwt: gamma is NaN");
  if (!std::isfinite(c.scale) || !(c.scale > 0)) SSQ_FAIL("conceft_cwt: scale must be positive and finite");
  for (int64_t i = 0; i < c.n_coeffs * c.J; ++i)
    if (!std::isfinite(c.coeffs[i])) SSQ_FAIL("conceft_cwt: coefficients must be finite");
  for (int64_t i = 0; i < 2 * c.M * c.J; ++i)
    if (!std::isfinite(c.vectors[i])) SSQ_FAIL("conceft_cwt: vectors must be finite");
  for (int64_t i = 0; i < c.na; ++i) {
    if (!(c.scales[i] > 0) || !std::isfinite(c.scales[i])) SSQ_FAIL("conceft_cwt: scales must be positive and finite");
    if (!std::isfinite(c.row_const[i])) SSQ_FAIL("conceft_cwt: row_const must be finite");
    if (!std::isfinite(c.f_asc[i])) SSQ_FAIL("conceft_cwt: ssq_freqs_asc must be finite");
  }
  BinRule<double> r;                                         // the checks of the frequency grid
  return bin_rule<double>(c.f_asc, c.na, c.freq_kind, c.freq_transition, 0, r);
}

struct PlanHolder {                     // the plan's tables are freed once the stream has drained
  ssq_cwt_plan* pl = nullptr;
  hipStream_t st = nullptr;
  ~PlanHolder() {
    if (!pl) return;
    (void)hipStreamSynchronize(st);
    ssq_cwt_plan_destroy(pl);
  }
};

// the plan of `cwt_higher_order` that stage 1 runs through.  The door makes it, behind its argument checks: the host door
// sizes its slices beside the plan's workspace, which only the plan knows.
int conceft_plan(const ConceftCall& c, PlanHolder* ph, ConceftShape* s) {
  ph->st = c.st;
  if (int rc = ssq_cwt_plan_create_gmwk(&ph->pl, c.dtype, c.N, c.gmw_gamma, c.gmw_beta, c.coeffs, c.n_coeffs, c.J, c.scales,
                                        c.na, c.dt, c.padtype, SSQ_VARIANT_UPSTREAM))
    return rc;
  s->plan = ph->pl;
  s->plan_bytes = ssq_cwt_plan_workspace_bytes(ph->pl, 1);
  return 0;
}

// conceft_cwt on device buffers (pipe_host, pipe_exec).  A call's workspace of s.work_bytes >= s.min_bytes is fixed by the
// call, not by the signals of a host slice: run() walks its signals in inner slices of work_bytes / signal_bytes whole
// signals, the plan's transforms and the squeeze kernel alternating.  kernel_ms is therefore the pipe's own (c.ms, one
// float: the squeeze kernel alone, summed over the inner slices), not run_timed's.
template <typename T>
struct ConceftPipe {
  static constexpr int kMid = 0;
  const ConceftCall& c;
  const ConceftShape& s;
  DeviceBufs d;
  TimingEvents t;
  ConceftDev<T> p;
  const cpx<T>* vec;
  const T* rcs;               // row_const * scale
  void* plan_work;
  int64_t slice;              // signals of an inner slice
  cpx<T>*Tx, *Wx, *work;
  T* w;
  int tables() {
    const int64_t na = c.na, J = c.J, M = c.M;
    SSQ_HIP(d.alloc(&plan_work, (size_t)s.plan_bytes));
    std::vector<cpx<T>> v((size_t)(M * J));
    for (int64_t i = 0; i < M * J; ++i) v[(size_t)i] = {(T)c.vectors[2 * i], (T)c.vectors[2 * i + 1]};
    SSQ_HIP(d.upload(&vec, v));
    std::vector<T> rc((size_t)na);
    for (int64_t i = 0; i < na; ++i) rc[(size_t)i] = (T)(c.row_const[i] * c.scale);
    SSQ_HIP(d.upload(&rcs, rc));
    BinRule<T> r;
    const int flipud = (c.variant & SSQ_VARIANT_FLIPUD) ? 1 : 0;
    if (int e = bin_rule<T>(c.f_asc, na, c.freq_kind, c.freq_transition, flipud, r)) return e;
    std::memset(&p, 0, sizeof(p));
    p.J = (int)J;
    p.M = (int)M;
    p.q.N = c.N;
    p.q.na = (int)na;
    p.q.s_end = (int)na;
    p.q.is_log = c.freq_kind != SSQ_FREQS_LINEAR ? 1 : 0;
    p.q.flipud = flipud;
    p.q.bin_min = r.bin_min;
    p.q.bin_step = r.bin_step;
    p.q.inv_bin_step = (T)1 / r.bin_step;
    p.q.gamma = (T)(c.gamma < 0 ? 10.0 * (sizeof(T) == 8 ? 2.2204460492503131e-16 : 1.1920928955078125e-07) : c.gamma);
    p.q.variant = 1;
    p.r.piecewise = c.freq_kind == SSQ_FREQS_LOG_PIECEWISE ? 1 : 0;
    p.r.idx1 = r.idx1;
    p.r.vlmin1 = r.vlmin1;
    p.r.dvl1 = r.dvl1;
    return 0;
  }
  int bind(int64_t cap, void* const* outs /* Tx, Wx, w */, void* wk) {
    Tx = (cpx<T>*)outs[0];
    Wx = (cpx<T>*)outs[1];
    w = (T*)outs[2];
    work = (cpx<T>*)wk;
    slice = std::min<int64_t>(cap, s.work_bytes / s.signal_bytes);
    if (c.ms) {
      *c.ms = 0.0f;
      SSQ_HIP(t.start(2, c.st));
    }
    return 0;
  }
  int run(int64_t nb_run, const void* d_x, const hipEvent_t*) {
    const int64_t N = c.N, M = c.M;
    const int64_t planes = c.J * s.plane;                      // coefficients of one signal's W (or dW)
    const hipStream_t st = c.st;
    SSQ_HIP(hipMemsetAsync(Tx, 0, (size_t)(nb_run * s.plane) * sizeof(cpx<T>), st));
    for (int64_t b0 = 0; b0 < nb_run; b0 += slice) {
      const int64_t nb = std::min(slice, nb_run - b0);
      cpx<T>* W = work;
      cpx<T>* dW = W + nb * planes;
      if (int e = ssq_cwt_plan_exec_cwt(s.plan, static_cast<const T*>(d_x) + b0 * N, nb, 1, 0, W, dW, plan_work, s.plan_bytes, st))
        return e;
      if (Wx)
        SSQ_HIP(hipMemcpyAsync(Wx + b0 * planes, W, (size_t)(nb * planes) * sizeof(cpx<T>), hipMemcpyDeviceToDevice, st));
      p.W = W;
      p.dW = dW;
      p.w = w ? w + b0 * M * s.plane : nullptr;
      p.q.Tx = Tx + b0 * s.plane;
      p.signals = nb;
      const dim3 grid((unsigned)((N + 63) / 64), (unsigned)std::min<int64_t>(nb, 65535));
      if (c.ms) SSQ_HIP(hipEventRecord(t.ev[0], st));
      if (p.r.piecewise)
        hipLaunchKernelGGL((cwt_conceft_kernel<T, true>), grid, dim3(64), 0, st, p, vec, rcs);
      else
        hipLaunchKernelGGL((cwt_conceft_kernel<T, false>), grid, dim3(64), 0, st, p, vec, rcs);
      SSQ_HIP(hipGetLastError());
      if (c.ms) {
        float ms = 0.0f;
        SSQ_HIP(hipEventRecord(t.ev[1], st));
        SSQ_HIP(hipEventSynchronize(t.ev[1]));
        SSQ_HIP(hipEventElapsedTime(&ms, t.ev[0], t.ev[1]));
        *c.ms += ms;
      }
    }
    return 0;
  }
};

}  // namespace

extern "C" {

int64_t ssq_conceft_cwt_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t na, int64_t n_orders,
                                        int64_t* min_bytes) {
  ConceftShape s;
  if (conceft_shape(dtype, batch, n_signal, na, n_orders, &s)) return -1;
  if (min_bytes) *min_bytes = s.min_bytes;
  return s.pref_bytes;
}

int ssq_conceft_cwt_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, double gmw_gamma, double gmw_beta,
                         const double* coeffs, int64_t n_coeffs, int64_t n_orders, const double* vectors, int64_t n_draws,
                         double scale, const double* scales, int64_t na, double dt, const double* row_const,
                         const double* ssq_freqs_asc, int freq_kind, int64_t freq_transition, int padtype, double gamma,
                         int variant, void* d_Tx, void* d_Wx, void* d_w, void* d_workspace, int64_t workspace_bytes,
                         void* stream, float* kernel_ms) {
  if (!d_x || !d_Tx || !d_workspace) SSQ_FAIL("conceft_cwt: NULL argument");
  const ConceftCall c{dtype, batch, n_signal, gmw_gamma, gmw_beta, coeffs, n_coeffs, n_orders, vectors, n_draws, scale,
                      scales, na, dt, row_const, ssq_freqs_asc, freq_kind, freq_transition, padtype, gamma, variant,
                      static_cast<hipStream_t>(stream), kernel_ms};
  ConceftShape s;
  if (int rc = conceft_check(c, &s)) return rc;
  if (workspace_bytes < s.min_bytes)
    SSQ_FAIL("conceft_cwt: workspace too small (" + std::to_string(workspace_bytes) + " < " + std::to_string(s.min_bytes) +
             " bytes: ssq_conceft_cwt_workspace_bytes)");
  if (int rc = require_device()) return rc;
  s.work_bytes = workspace_bytes;
  PlanHolder ph;
  if (int rc = conceft_plan(c, &ph, &s)) return rc;
  void* const outs[] = {d_Tx, d_Wx, d_w};
  return dtype == SSQ_F32 ? pipe_exec<ConceftPipe<float>>(c, s, d_x, outs, d_workspace, nullptr, &c.st)
                          : pipe_exec<ConceftPipe<double>>(c, s, d_x, outs, d_workspace, nullptr, &c.st);
}

int ssq_conceft_cwt_host(int dtype, const void* x, int64_t batch, int64_t n_signal, double gmw_gamma, double gmw_beta,
                         const double* coeffs, int64_t n_coeffs, int64_t n_orders, const double* vectors, int64_t n_draws,
                         double scale, const double* scales, int64_t na, double dt, const double* row_const,
                         const double* ssq_freqs_asc, int freq_kind, int64_t freq_transition, int padtype, double gamma,
                         int variant, int64_t work_limit_bytes, void* Tx, void* Wx, void* w) {
  if (!x || !Tx) SSQ_FAIL("conceft_cwt: NULL argument");
  const ConceftCall c{dtype, batch, n_signal, gmw_gamma, gmw_beta, coeffs, n_coeffs, n_orders, vectors, n_draws, scale,
                      scales, na, dt, row_const, ssq_freqs_asc, freq_kind, freq_transition, padtype, gamma, variant,
                      nullptr, nullptr};
  ConceftShape s;
  if (int rc = conceft_check(c, &s)) return rc;
  if (work_limit_bytes < 0 || (work_limit_bytes > 0 && work_limit_bytes < s.min_bytes))
    SSQ_FAIL("conceft_cwt: work_limit_bytes must be 0 or at least " + std::to_string(s.min_bytes) + " bytes");
  s.work_bytes = work_limit_bytes ? std::min(work_limit_bytes, s.pref_bytes) : s.pref_bytes;
  if (int rc = require_device()) return rc;
  PlanHolder ph;
  if (int rc = conceft_plan(c, &ph, &s)) return rc;
  const size_t el = dtype == SSQ_F32 ? 4 : 8, map_el = (size_t)s.plane * el;
  const HostOut outs[] = {{Tx, 2 * map_el}, {Wx, 2 * map_el * (size_t)n_orders}, {w, map_el * (size_t)n_draws}};
  // the signals that fit beside the call's workspace and the plan's; the workspace holds no more of them than a slice has
  const int64_t slice = slice_signals(batch, host_signal_bytes(el * (size_t)n_signal, outs),
                                      (double)s.work_bytes + (double)s.plan_bytes, batch);
  s.work_bytes = std::min(s.work_bytes, slice * s.signal_bytes);
  const HostSlice sl{slice, (size_t)s.work_bytes};
  return dtype == SSQ_F32 ? pipe_host<ConceftPipe<float>>(c, s, x, el * (size_t)n_signal, outs, sl)
                          : pipe_host<ConceftPipe<double>>(c, s, x, el * (size_t)n_signal, outs, sl);
}

}  // extern "C"
