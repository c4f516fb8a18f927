// ridge.hip -- ridge extraction: upstream ssqueezepy.extract_ridges (old/ssqueezepy/ridge_extraction.py:11-233).
//
// Per (signal, ridge):  energy |Tf|^2 (:121) -> cost -log(e / max_col(e) + eps) (:132-133) -> forward min-plus DP
// pen[f, t] += min_j (pen[j, t-1] + P[f, j]) (:169-175) -> first argmin per column mod N (:164-165) -> serial backward
// trace, last f within eps (:206-215) -> band removal energy[int(r - bw):int(r + bw), t] = 0 (:141-143).
// Layout: energy [B][F][N] (as Tf), cost_t and pen time-major [B][N][F] so that the DP and the backward trace read
// whole columns.  The forward DP is one workgroup per signal walking t, the previous column in LDS; the backward
// trace one wave per signal.  No FMA contraction anywhere in this file: `penalty * d*d` and `+ pen` are separate
// roundings in upstream, and the DP must equal numpy bitwise.
#pragma clang fp contract(off)

#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/ssq_hip.h"
#include "dev_buffers.h"

using namespace ssq;

namespace {

constexpr int kFwdThreads = 1024;   // 16 waves: 4 lanes per DP row, 256 rows per pass
constexpr int kLanesPerRow = 4;

template <typename PT>
__host__ __device__ constexpr PT eps_of() {   // utils/common.py EPS32 / EPS64 = np.finfo(..).eps
  return sizeof(PT) == 4 ? (PT)1.1920928955078125e-07 : (PT)2.220446049250313e-16;
}

template <typename E>
__device__ __forceinline__ E qnan() {
  return std::numeric_limits<E>::quiet_NaN();
}

template <typename E>
__device__ __forceinline__ bool is_nan(E v) {
  return v != v;
}

// |Tf|^2: np.abs(z) is hypot (npy_cabs), then squared; a real input squares its magnitude.  fp32 hypot in fp64
// (both squares exact, one rounding of the sum, one of the root), as the host libm's hypotf does
__device__ __forceinline__ float cabs_up(float re, float im) {
  return (float)sqrt((double)re * (double)re + (double)im * (double)im);
}
__device__ __forceinline__ double cabs_up(double re, double im) { return hypot(re, im); }

template <typename E, bool CPLX>
__global__ void ridge_energy_kernel(const E* __restrict__ x, long long n, E* __restrict__ energy) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    E a;
    if (CPLX) a = cabs_up(x[2 * i], x[2 * i + 1]);
    else a = fabs(x[i]);
    energy[i] = a * a;
  }
}

// One 64-column tile of one signal: src [F][N] (energy, or a caller's cost) -> cost, written time-major into cost_t
// and pen (the DP starts from pen = cost, :160) and, when asked, f-major into cost_out.  From energy the column max
// is np.max (NaN propagates), the cost -log(e / emax + eps) in E with eps of the parameter dtype (:113-116, :132-133).
template <typename E, typename PT, bool FROM_ENERGY>
__global__ __launch_bounds__(256) void ridge_cost_kernel(const E* __restrict__ src, int F, long long N,
                                                         E* __restrict__ cost_t, E* __restrict__ pen,
                                                         E* __restrict__ cost_out, long long cost_out_bstride) {
  __shared__ E tile[64][65];
  __shared__ E red[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long long t0 = (long long)blockIdx.x * 64, t = t0 + tx;
  const long long b = blockIdx.y;
  const E* sb = src + b * F * N;
  E emax = (E)1;
  if (FROM_ENERGY) {
    E m = -std::numeric_limits<E>::infinity();
    bool nan = false;
    if (t < N)
      for (int f = ty; f < F; f += 4) {
        const E v = sb[(long long)f * N + t];
        nan |= is_nan(v);
        m = v > m ? v : m;
      }
    red[ty][tx] = nan ? qnan<E>() : m;
    __syncthreads();
    emax = red[0][tx];
    for (int k = 1; k < 4; ++k) {
      const E v = red[k][tx];
      emax = is_nan(emax) ? emax : (is_nan(v) || v > emax ? v : emax);
    }
  }
  const E eps = (E)eps_of<PT>();
  for (int f0 = 0; f0 < F; f0 += 64) {
    for (int fy = ty; fy < 64; fy += 4) {
      const int f = f0 + fy;
      if (f < F && t < N) {
        const E v = sb[(long long)f * N + t];
        const E c = FROM_ENERGY ? -log(v / emax + eps) : v;
        tile[fy][tx] = c;
        if (cost_out) cost_out[b * cost_out_bstride + (long long)f * N + t] = c;
      }
    }
    __syncthreads();
    for (int k = ty; k < 64; k += 4) {
      const long long tt = t0 + k;
      const int f = f0 + tx;
      if (tt < N && f < F) {
        const E c = tile[tx][k];
        const long long o = (b * N + tt) * F + f;
        cost_t[o] = c;
        pen[o] = c;
      }
    }
    __syncthreads();
  }
}

// NaN-propagating min of two partial row minima (np.amin returns NaN if any candidate is NaN)
template <typename E>
__device__ __forceinline__ E min_nan(E a, E b) {
  return is_nan(a) ? a : (is_nan(b) ? b : fmin(a, b));
}

// min_j (prev[j] + P[f, j]) over this lane's share j = (c * V + v), c = sub, sub + 4, ...  with
// P[f, j] = penalty * ((s_f - s_j) * (s_f - s_j)) in the parameter dtype (:89), widened to E for the add (:174).
// CHECK_NAN: the P row may hold non-finite values, so a candidate can be NaN although the previous column has none;
// test every candidate.  Otherwise a NaN-free previous column gives NaN-free candidates and fmin is exact.
template <typename E, typename PT, int V, bool CHECK_NAN>
__device__ __forceinline__ E row_min(const E* prev, const PT* met, PT sf, PT penalty, int F, int sub) {
  const int nchunk = (F + V - 1) / V;
  E m = std::numeric_limits<E>::infinity();
  bool nan = false;
  for (int c = sub; c < nchunk; c += kLanesPerRow) {
    E pv[V];
    PT mv[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      pv[v] = prev[c * V + v];
      mv[v] = met[c * V + v];
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const PT d = sf - mv[v];
      const PT p = penalty * (d * d);
      const E cand = pv[v] + (E)p;
      if (CHECK_NAN) {
        if (c * V + v < F) {
          nan |= is_nan(cand);
          m = fmin(m, cand);
        }
      } else {
        m = fmin(m, cand);
      }
    }
  }
  return nan ? qnan<E>() : m;
}

// Forward pass of one signal (one workgroup, sequential in t).  SMEM: the previous column (double-buffered) and the
// metric live in LDS, padded to a multiple of the vector width with pen = +inf / s = 0; otherwise (a column too big
// for LDS) both are read from global memory, the previous column being pen's own row t-1.  A column holding NaN
// makes every later column NaN (:174 amin), tracked by a flag per column parity.
template <typename E, typename PT, bool SMEM>
__global__ __launch_bounds__(kFwdThreads) void ridge_forward_kernel(E* __restrict__ pen, const PT* __restrict__ metric,
                                                                    PT penalty, int F, long long N) {
  constexpr int V = SMEM ? 16 / (int)sizeof(E) : 1;
  extern __shared__ __align__(16) unsigned char ridge_smem[];
  __shared__ int s_nan[2];
  __shared__ int s_pfinite;
  const int tid = threadIdx.x;
  const int sub = tid & (kLanesPerRow - 1);
  const int rows = kFwdThreads / kLanesPerRow;
  const int Fp = (F + V - 1) / V * V;
  E* pb = pen + (long long)blockIdx.x * N * F;
  E* buf0 = reinterpret_cast<E*>(ridge_smem);
  E* buf1 = buf0 + Fp;
  PT* lmet = reinterpret_cast<PT*>(buf1 + Fp);
  if (tid == 0) {
    s_nan[0] = 0;
    s_nan[1] = 0;
    s_pfinite = 1;
  }
  __syncthreads();
  if (SMEM) {
    for (int f = tid; f < Fp; f += kFwdThreads) {
      buf0[f] = f < F ? pb[f] : std::numeric_limits<E>::infinity();
      buf1[f] = std::numeric_limits<E>::infinity();
      lmet[f] = f < F ? metric[f] : (PT)0;
    }
  }
  bool nan0 = false;
  for (int f = tid; f < F; f += kFwdThreads) nan0 |= is_nan(pb[f]);
  if (nan0) s_nan[0] = 1;
  bool pfin = true;
  for (unsigned k = tid; k < (unsigned)F * (unsigned)F; k += kFwdThreads) {   // F <= 32767: F * F < 2^31
    const PT d = metric[k / (unsigned)F] - metric[k % (unsigned)F];
    const PT p = penalty * (d * d);
    pfin &= std::isfinite(p);
  }
  if (!pfin) s_pfinite = 0;
  __syncthreads();
  const bool pfinite = s_pfinite != 0;
  const PT* met = SMEM ? lmet : metric;
  const int fend = (F + rows - 1) / rows * rows;   // the 4 lanes of a row stay together through the shuffles
  for (long long t = 1; t < N; ++t) {
    const E* prev = SMEM ? ((t - 1) & 1 ? buf1 : buf0) : pb + (t - 1) * F;
    E* next = (t & 1) ? buf1 : buf0;
    const bool colnan = s_nan[(t - 1) & 1] != 0;
    bool wrote_nan = false;
    for (int f = tid / kLanesPerRow; f < fend; f += rows) {
      const bool live = f < F;
      E c = 0;
      if (live && sub == 0) c = pb[t * F + f];
      E m = qnan<E>();
      if (live && !colnan) {
        const PT sf = met[f];
        m = pfinite ? row_min<E, PT, V, false>(prev, met, sf, penalty, F, sub)
                    : row_min<E, PT, V, true>(prev, met, sf, penalty, F, sub);
      }
      m = min_nan(m, __shfl_xor(m, 1, kLanesPerRow));
      m = min_nan(m, __shfl_xor(m, 2, kLanesPerRow));
      if (live && sub == 0) {
        const E v = c + m;                                   // pen[f, t] += amin(..)  (:173-175)
        pb[t * F + f] = v;
        if (SMEM) next[f] = v;
        wrote_nan |= is_nan(v);
      }
    }
    if (wrote_nan) s_nan[t & 1] = 1;
    __syncthreads();
  }
}

// np.argmin over one pen column (first minimum; the first NaN if any), then unravel_index(.., (F, N))[1] = idx mod N
// (:164-165).  One wave per (signal, column).
template <typename E>
__device__ __forceinline__ bool argmin_before(E a, int ia, E b, int ib) {
  if (ib < 0) return ia >= 0;
  if (ia < 0) return false;
  const bool an = is_nan(a), bn = is_nan(b);
  if (an != bn) return an;
  if (!an) {
    if (a < b) return true;
    if (b < a) return false;
  }
  return ia < ib;
}

template <typename E>
__global__ __launch_bounds__(256) void ridge_argmin_kernel(const E* __restrict__ pen, int F, long long N,
                                                           long long cols, int* __restrict__ ridge) {
  const long long col = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (col >= cols) return;
  const E* row = pen + col * F;
  E bv = 0;
  int bi = -1;
  for (int f = lane; f < F; f += 64) {
    const E v = row[f];
    if (argmin_before(v, f, bv, bi)) {
      bv = v;
      bi = f;
    }
  }
  for (int off = 32; off >= 1; off >>= 1) {
    const E ov = __shfl_xor(bv, off);
    const int oi = __shfl_xor(bi, off);
    if (argmin_before(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if (lane == 0) ridge[col] = (int)(bi % N);
}

// Serial backward trace (:206-215) of one signal in one wave: for t = N-2 .. 0 with r = ridge[t+1] (already updated),
// val = pen[r, t+1] - cost[r, t+1]; the LAST f with |val - (pen[f, t] + P[r, f])| < eps becomes ridge[t], else the
// forward index stays.  The ballot over each 64-row slice keeps its highest set lane.
template <typename E, typename PT>
__global__ __launch_bounds__(64) void ridge_backward_kernel(const E* __restrict__ pen, const E* __restrict__ cost_t,
                                                            const PT* __restrict__ metric, PT penalty, int F,
                                                            long long N, int* __restrict__ ridge) {
  const int lane = threadIdx.x;
  const long long b = blockIdx.x;
  const E* pb = pen + b * N * F;
  const E* cb = cost_t + b * N * F;
  int* rb = ridge + b * N;
  const E eps = (E)eps_of<PT>();
  int r = rb[N - 1];
  for (long long t = N - 2; t >= 0; --t) {
    const E* prow = pb + t * F;
    const E val = pb[(t + 1) * F + r] - cb[(t + 1) * F + r];
    const PT sr = metric[r];
    const int fwd = rb[t];
    int last = -1;
    for (int f0 = 0; f0 < F; f0 += 64) {
      const int f = f0 + lane;
      bool hit = false;
      if (f < F) {
        const PT d = sr - metric[f];
        const PT p = penalty * (d * d);
        hit = fabs(val - (prow[f] + (E)p)) < eps;
      }
      const unsigned long long bal = __ballot(hit);
      if (bal) last = f0 + 63 - __clzll((long long)bal);
    }
    r = last >= 0 ? last : fwd;
    if (lane == 0) rb[t] = r;
  }
}

// ridge_idxs[:, i], ridge_f = scales_orig[idx], ridge_e = energy[idx, t] before this ridge's band goes (:137-139), then
// energy[int(r - bw):int(r + bw), t] = 0 with Python slice normalisation (negative start counts from the end) (:141-143)
__device__ __forceinline__ long long py_slice_bound(long long i, int F) {
  if (i < 0) {
    i += F;
    return i < 0 ? 0 : i;
  }
  return i > F ? F : i;
}

template <typename E, typename PT>
__global__ void ridge_band_kernel(E* __restrict__ energy, const int* __restrict__ ridge, const PT* __restrict__ scales,
                                  int F, long long N, long long cols, double bw, int i, int n_ridges,
                                  long long* __restrict__ idx_out, PT* __restrict__ f_out, PT* __restrict__ e_out) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= cols) return;
  const long long b = k / N, t = k % N;
  const int r = ridge[k];
  E* col = energy + b * F * N + t;
  const long long o = k * n_ridges + i;
  idx_out[o] = r;
  if (f_out) f_out[o] = scales[r];
  if (e_out) e_out[o] = (PT)col[(long long)r * N];
  const long long lo = py_slice_bound((long long)((double)r - bw), F);
  const long long hi = py_slice_bound((long long)((double)r + bw), F);
  for (long long f = lo; f < hi; ++f) col[f * N] = (E)0;
}

size_t align_up(size_t n) { return (n + 255) & ~(size_t)255; }

struct RidgeWs {
  void* energy;
  void* cost_t;
  void* pen;
  int* ridge;
};

size_t ws_bytes(int dtype, int64_t batch, int64_t F, int64_t N) {
  const size_t es = dtype == SSQ_F64 ? 8 : 4;
  const size_t mat = align_up(es * (size_t)(batch * F * N));
  return 3 * mat + align_up(sizeof(int) * (size_t)(batch * N));
}

RidgeWs ws_carve(void* base, int dtype, int64_t batch, int64_t F, int64_t N) {
  const size_t es = dtype == SSQ_F64 ? 8 : 4;
  const size_t mat = align_up(es * (size_t)(batch * F * N));
  char* p = static_cast<char*>(base);
  return {p, p + mat, p + 2 * mat, reinterpret_cast<int*>(p + 3 * mat)};
}

int check_shape(int dtype, int param_dtype, int64_t batch, int64_t F, int64_t N) {
  if (dtype != SSQ_F32 && dtype != SSQ_F64) SSQ_FAIL("dtype must be SSQ_F32 or SSQ_F64");
  if (param_dtype != SSQ_F32 && param_dtype != SSQ_F64) SSQ_FAIL("param_dtype must be SSQ_F32 or SSQ_F64");
  if (dtype == SSQ_F32 && param_dtype == SSQ_F64) SSQ_FAIL("an fp32 cost takes fp32 parameters (:113-116)");
  if (batch < 1) SSQ_FAIL("batch must be >= 1");
  if (F < 1 || F > 32767) SSQ_FAIL("n_freqs must be in [1, 32767]");
  if (N < 1) SSQ_FAIL("n_time must be >= 1");
  if (batch > 65535) SSQ_FAIL("batch must be <= 65535");
  return 0;
}

// forward DP, forward argmin, backward trace on pen (holding the cost) and cost_t; ridge: [B][N]
template <typename E, typename PT>
int track_typed(E* pen, const E* cost_t, const PT* metric, PT penalty, int64_t batch, int F, int64_t N, int* ridge,
                hipStream_t st) {
  int dev = 0, max_lds = 0;
  SSQ_HIP(hipGetDevice(&dev));
  SSQ_HIP(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  constexpr int V = 16 / (int)sizeof(E);
  const size_t Fp = (size_t)(F + V - 1) / V * V;
  const size_t lds = 2 * Fp * sizeof(E) + Fp * sizeof(PT);
  if (N > 1) {
    if (lds + 64 <= (size_t)max_lds) {
      auto k = ridge_forward_kernel<E, PT, true>;
      SSQ_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(k, dim3((unsigned)batch), dim3(kFwdThreads), lds, st, pen, metric, penalty, F, (long long)N);
    } else {
      hipLaunchKernelGGL((ridge_forward_kernel<E, PT, false>), dim3((unsigned)batch), dim3(kFwdThreads), 0, st, pen,
                         metric, penalty, F, (long long)N);
    }
    SSQ_HIP(hipGetLastError());
  }
  const long long cols = (long long)batch * N;
  hipLaunchKernelGGL(ridge_argmin_kernel<E>, dim3((unsigned)((cols + 3) / 4)), dim3(256), 0, st, pen, F, (long long)N,
                     cols, ridge);
  SSQ_HIP(hipGetLastError());
  if (N > 1) {
    hipLaunchKernelGGL((ridge_backward_kernel<E, PT>), dim3((unsigned)batch), dim3(64), 0, st, pen, cost_t, metric,
                       penalty, F, (long long)N, ridge);
    SSQ_HIP(hipGetLastError());
  }
  return 0;
}

template <typename E, typename PT>
int exec_typed(int is_complex, const void* Tf, int64_t batch, int F, int64_t N, const void* metric, const void* scales,
               double penalty, int64_t n_ridges, double bw, int64_t* idx_out, void* f_out, void* e_out, void* cost_out,
               void* workspace, hipStream_t st) {
  RidgeWs w = ws_carve(workspace, sizeof(E) == 8 ? SSQ_F64 : SSQ_F32, batch, F, N);
  E* energy = static_cast<E*>(w.energy);
  const long long n = (long long)batch * F * N;
  const unsigned eb = (unsigned)std::min<long long>((n + 255) / 256, 1 << 20);
  if (is_complex)
    hipLaunchKernelGGL((ridge_energy_kernel<E, true>), dim3(eb), dim3(256), 0, st, static_cast<const E*>(Tf), n, energy);
  else
    hipLaunchKernelGGL((ridge_energy_kernel<E, false>), dim3(eb), dim3(256), 0, st, static_cast<const E*>(Tf), n, energy);
  SSQ_HIP(hipGetLastError());
  const long long cols = (long long)batch * N;
  const dim3 cgrid((unsigned)((N + 63) / 64), (unsigned)batch);
  for (int64_t i = 0; i < n_ridges; ++i) {
    E* co = cost_out ? static_cast<E*>(cost_out) + i * (int64_t)F * N : nullptr;
    hipLaunchKernelGGL((ridge_cost_kernel<E, PT, true>), cgrid, dim3(256), 0, st, energy, F, (long long)N,
                       static_cast<E*>(w.cost_t), static_cast<E*>(w.pen), co, (long long)(n_ridges * F * N));
    SSQ_HIP(hipGetLastError());
    const int rc = track_typed<E, PT>(static_cast<E*>(w.pen), static_cast<const E*>(w.cost_t),
                                      static_cast<const PT*>(metric), (PT)penalty, batch, F, N, w.ridge, st);
    if (rc) return rc;
    hipLaunchKernelGGL((ridge_band_kernel<E, PT>), dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, st, energy,
                       w.ridge, static_cast<const PT*>(scales), F, (long long)N, cols, bw, (int)i, (int)n_ridges,
                       (long long*)idx_out, static_cast<PT*>(f_out), static_cast<PT*>(e_out));
    SSQ_HIP(hipGetLastError());
  }
  return 0;
}

}  // namespace

extern "C" {

int64_t ssq_ridges_workspace_bytes(int dtype, int64_t batch, int64_t n_freqs, int64_t n_time) {
  if (check_shape(dtype, dtype == SSQ_F64 ? SSQ_F64 : SSQ_F32, batch, n_freqs, n_time)) return -1;
  return (int64_t)ws_bytes(dtype, batch, n_freqs, n_time);
}

int ssq_ridges_exec(int dtype, int param_dtype, int is_complex, const void* d_Tf, int64_t batch, int64_t n_freqs,
                    int64_t n_time, const void* d_metric, const void* d_scales, double penalty, int64_t n_ridges,
                    double bw, int64_t* d_ridge_idxs, void* d_ridge_f, void* d_ridge_e, void* d_cost_out,
                    void* d_workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_shape(dtype, param_dtype, batch, n_freqs, n_time)) return rc;
  if (!d_Tf || !d_metric || !d_ridge_idxs || !d_workspace) SSQ_FAIL("NULL argument");
  if (d_ridge_f && !d_scales) SSQ_FAIL("ridge_f needs scales");
  if (n_ridges < 1) SSQ_FAIL("n_ridges must be >= 1");
  if (!(bw >= 0.0) || !std::isfinite(bw)) SSQ_FAIL("bw must be finite and >= 0");
  if (workspace_bytes < (int64_t)ws_bytes(dtype, batch, n_freqs, n_time)) SSQ_FAIL("workspace too small");
  bw = std::min(bw, 1e15);   // int(r - bw) only matters through the slice clamp at [0, F]
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int F = (int)n_freqs;
  if (dtype == SSQ_F32)
    return exec_typed<float, float>(is_complex, d_Tf, batch, F, n_time, d_metric, d_scales, penalty, n_ridges, bw,
                                    d_ridge_idxs, d_ridge_f, d_ridge_e, d_cost_out, d_workspace, st);
  if (param_dtype == SSQ_F32)
    return exec_typed<double, float>(is_complex, d_Tf, batch, F, n_time, d_metric, d_scales, penalty, n_ridges, bw,
                                     d_ridge_idxs, d_ridge_f, d_ridge_e, d_cost_out, d_workspace, st);
  return exec_typed<double, double>(is_complex, d_Tf, batch, F, n_time, d_metric, d_scales, penalty, n_ridges, bw,
                                    d_ridge_idxs, d_ridge_f, d_ridge_e, d_cost_out, d_workspace, st);
}

int ssq_extract_ridges_host(int dtype, int param_dtype, int is_complex, const void* Tf, int64_t batch, int64_t n_freqs,
                            int64_t n_time, const void* metric, const void* scales, double penalty, int64_t n_ridges,
                            double bw, int64_t* ridge_idxs, void* ridge_f, void* ridge_e, void* cost_out) {
  if (int rc = check_shape(dtype, param_dtype, batch, n_freqs, n_time)) return rc;
  if (!Tf || !metric || !ridge_idxs) SSQ_FAIL("NULL argument");
  if (ridge_f && !scales) SSQ_FAIL("ridge_f needs scales");
  if (n_ridges < 1) SSQ_FAIL("n_ridges must be >= 1");
  if (int rc = require_device()) return rc;
  const size_t es = dtype == SSQ_F64 ? 8 : 4, ps = param_dtype == SSQ_F64 ? 8 : 4;
  const size_t n = (size_t)(batch * n_freqs * n_time), outs = (size_t)(batch * n_time * n_ridges);
  DeviceBufs d;
  void *dT, *dm, *ds = nullptr, *di, *df = nullptr, *de = nullptr, *dc = nullptr, *dw;
  const int64_t wsb = (int64_t)ws_bytes(dtype, batch, n_freqs, n_time);
  SSQ_HIP(d.upload(&dT, Tf, n * es * (is_complex ? 2 : 1)));
  SSQ_HIP(d.upload(&dm, metric, (size_t)n_freqs * ps));
  if (scales) SSQ_HIP(d.upload(&ds, scales, (size_t)n_freqs * ps));
  SSQ_HIP(d.alloc(&di, outs * sizeof(int64_t)));
  if (ridge_f) SSQ_HIP(d.alloc(&df, outs * ps));
  if (ridge_e) SSQ_HIP(d.alloc(&de, outs * ps));
  if (cost_out) SSQ_HIP(d.alloc(&dc, n * (size_t)n_ridges * es));
  SSQ_HIP(d.alloc(&dw, (size_t)wsb));
  if (int rc = ssq_ridges_exec(dtype, param_dtype, is_complex, dT, batch, n_freqs, n_time, dm, ds, penalty, n_ridges, bw,
                               static_cast<int64_t*>(di), df, de, dc, dw, wsb, nullptr))
    return rc;
  SSQ_HIP(hipMemcpy(ridge_idxs, di, outs * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (ridge_f) SSQ_HIP(hipMemcpy(ridge_f, df, outs * ps, hipMemcpyDeviceToHost));
  if (ridge_e) SSQ_HIP(hipMemcpy(ridge_e, de, outs * ps, hipMemcpyDeviceToHost));
  if (cost_out) SSQ_HIP(hipMemcpy(cost_out, dc, n * (size_t)n_ridges * es, hipMemcpyDeviceToHost));
  return 0;
}

int ssq_ridge_track_host(int dtype, int param_dtype, const void* cost, int64_t batch, int64_t n_freqs, int64_t n_time,
                         const void* metric, double penalty, int64_t* ridge_idxs, void* pen_out) {
  if (int rc = check_shape(dtype, param_dtype, batch, n_freqs, n_time)) return rc;
  if (!cost || !metric || !ridge_idxs) SSQ_FAIL("NULL argument");
  if (int rc = require_device()) return rc;
  const size_t es = dtype == SSQ_F64 ? 8 : 4, ps = param_dtype == SSQ_F64 ? 8 : 4;
  const int64_t F = n_freqs, N = n_time;
  const size_t n = (size_t)(batch * F * N);
  DeviceBufs d;
  void *dsrc, *dct, *dpen, *dm, *dr;
  SSQ_HIP(d.upload(&dsrc, cost, n * es));
  SSQ_HIP(d.alloc(&dct, n * es));
  SSQ_HIP(d.alloc(&dpen, n * es));
  SSQ_HIP(d.upload(&dm, metric, (size_t)F * ps));
  SSQ_HIP(d.alloc(&dr, (size_t)(batch * N) * sizeof(int)));
  const dim3 cgrid((unsigned)((N + 63) / 64), (unsigned)batch);
  int rc = 0;
  if (dtype == SSQ_F32) {
    hipLaunchKernelGGL((ridge_cost_kernel<float, float, false>), cgrid, dim3(256), 0, nullptr,
                       static_cast<const float*>(dsrc), (int)F, (long long)N, static_cast<float*>(dct),
                       static_cast<float*>(dpen), (float*)nullptr, 0LL);
    SSQ_HIP(hipGetLastError());
    rc = track_typed<float, float>(static_cast<float*>(dpen), static_cast<const float*>(dct),
                                   static_cast<const float*>(dm), (float)penalty, batch, (int)F, N,
                                   static_cast<int*>(dr), nullptr);
  } else {
    hipLaunchKernelGGL((ridge_cost_kernel<double, double, false>), cgrid, dim3(256), 0, nullptr,
                       static_cast<const double*>(dsrc), (int)F, (long long)N, static_cast<double*>(dct),
                       static_cast<double*>(dpen), (double*)nullptr, 0LL);
    SSQ_HIP(hipGetLastError());
    rc = param_dtype == SSQ_F32
             ? track_typed<double, float>(static_cast<double*>(dpen), static_cast<const double*>(dct),
                                          static_cast<const float*>(dm), (float)penalty, batch, (int)F, N,
                                          static_cast<int*>(dr), nullptr)
             : track_typed<double, double>(static_cast<double*>(dpen), static_cast<const double*>(dct),
                                           static_cast<const double*>(dm), penalty, batch, (int)F, N,
                                           static_cast<int*>(dr), nullptr);
  }
  if (rc) return rc;
  std::vector<int> r((size_t)(batch * N));
  SSQ_HIP(hipMemcpy(r.data(), dr, r.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (size_t k = 0; k < r.size(); ++k) ridge_idxs[k] = r[k];
  if (pen_out) {   // time-major on the device -> [B][F][N]
    std::vector<unsigned char> h(n * es);
    SSQ_HIP(hipMemcpy(h.data(), dpen, n * es, hipMemcpyDeviceToHost));
    unsigned char* o = static_cast<unsigned char*>(pen_out);
    for (int64_t b = 0; b < batch; ++b)
      for (int64_t t = 0; t < N; ++t)
        for (int64_t f = 0; f < F; ++f)
          std::memcpy(o + ((b * F + f) * N + t) * es, h.data() + ((b * N + t) * F + f) * es, es);
  }
  return 0;
}

}  // extern "C"
