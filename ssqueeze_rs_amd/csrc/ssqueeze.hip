// ssqueeze.hip -- upstream ssqueezepy's synchrosqueezing step on a transform the caller already holds:
// `phase_cwt` / `phase_stft` (old/ssqueezepy/algos.py:706-857) and `ssqueeze` (ssqueezing.py:13-245) from a phase
// transform `w` (algos.py:153-252, `indexed_sum_onfly`) or from `dWx` (algos.py:126-150, `ssqueeze_fast`).
//
//   phase_kernel           elementwise, one thread per element: w = |(B C - A D) / ((C^2 + D^2) 2 pi)| (STFT:
//                          |Sfs[row] - ...|), inf where |Wx| < gamma; plain IEEE division as reassign_bin_upstream
//                          (cwt_bin.h) and phase_bin_upstream (stft_kernels.h) compute it, so w agrees with the fused
//                          ssq_cwt / ssq_stft get_w output.
//   ssqueeze_w_kernel      one thread per column walks the rows in order (deterministic, no atomics), skipping inf w;
//                          runs of rows landing in one bin are summed in registers and added to Tx once, as
//                          cwt_reassign_rows_kernel does with w derived from dWx.
//   from dWx               the fused paths' own kernels, driven through their parameter blocks: cwt_reassign_rows_kernel
//                          (CwtSsqDev + CwtRowsDev, every scale grid) and reassign_cols_kernel (StftDev, upstream rule).
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/ssq_hip.h"
#include "bin_rule.h"
#include "cwt_kernels.h"
#include "dev_buffers.h"
#include "stft_kernels.h"

using namespace ssq;

namespace {

constexpr int kPhaseBlock = 256;
constexpr int kMaxGridY = 65535;

// w of one element: algos.py:721-729 (CWT, sfs == 0 and unused) / :795-804 (STFT)
template <typename T, bool STFT>
__device__ __forceinline__ T phase_one(cpx<T> Wv, cpx<T> dW, T sfs, T gamma) {
  const T A = dW.x, B = dW.y, C = Wv.x, D = Wv.y;
  if (hypot(C, D) < gamma) return (T)INFINITY;
  const T q = (B * C - A * D) / ((C * C + D * D) * (T)6.283185307179586);
  return STFT ? fabs(sfs - q) : fabs(q);
}

// Wx, dWx [planes][cols] interleaved complex, w [planes][cols] real; plane p is row p % rows of its signal.
// grid (ceil(cols / 256), min(planes, 65535)), the y blocks stride over the planes.
template <typename T, bool STFT>
__global__ __launch_bounds__(kPhaseBlock) void phase_kernel(const cpx<T>* __restrict__ Wx, const cpx<T>* __restrict__ dWx,
                                                            const T* __restrict__ Sfs, long long planes, int rows,
                                                            long long cols, T gamma, T* __restrict__ w) {
  const long long j = (long long)blockIdx.x * kPhaseBlock + threadIdx.x;
  if (j >= cols) return;
  for (long long pl = blockIdx.y; pl < planes; pl += gridDim.y) {
    const long long o = pl * cols + j;
    const T sfs = STFT ? Sfs[pl % rows] : (T)0;
    w[o] = phase_one<T, STFT>(Wx[o], dWx[o], sfs, gamma);
  }
}

// Tx[k, j] += Wx[i, j] * row_const[i] for every row i with finite w[i, j] (algos.py:173-252).  SQ: SSQ_SQUEEZE_SUM
// (complex Tx), _LEBESGUE (Wx not read: 1/rows per row, ssqueezing.py:183-184), _ABS (|Wx|, real Tx).  Tx zero on
// entry.  grid (ceil(cols / 64), min(batch, 65535)), block 64; the y blocks stride over the signals.
template <typename T, int SQ>
__global__ __launch_bounds__(64) void ssqueeze_w_kernel(const cpx<T>* __restrict__ Wx, const T* __restrict__ w,
                                                        const T* __restrict__ row_const, long long batch, int rows,
                                                        long long cols, BinRule<T> r, T leb_val, void* Tx_) {
  constexpr int UN = 8;
  using Out = typename std::conditional<SQ == SSQ_SQUEEZE_ABS, T, cpx<T>>::type;
  const long long j = (long long)blockIdx.x * 64 + threadIdx.x;
  if (j >= cols) return;
  const long long plane = (long long)rows * cols;
  for (long long b = blockIdx.y; b < batch; b += gridDim.y) {
    const cpx<T>* __restrict__ Wp = Wx + b * plane + j;
    const T* __restrict__ wp = w + b * plane + j;
    Out* __restrict__ Tp = static_cast<Out*>(Tx_) + b * plane + j;
    int k_cur = -1;
    cpx<T> acc = {(T)0, (T)0};
    auto flush = [&]() {
      if (k_cur < 0) return;
      Out* d = Tp + (long long)k_cur * cols;
      if constexpr (SQ == SSQ_SQUEEZE_ABS) {
        *d += acc.x;
      } else {
        cpx<T> t = *d;
        t.x += acc.x;
        t.y += acc.y;
        *d = t;
      }
    };
    for (int i0 = 0; i0 < rows; i0 += UN) {
      T wb[UN];
      cpx<T> Wb[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int ii = (i0 + u < rows) ? i0 + u : rows - 1;
        wb[u] = wp[(long long)ii * cols];
        if constexpr (SQ != SSQ_SQUEEZE_LEBESGUE) Wb[u] = Wp[(long long)ii * cols];
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int i = i0 + u;
        if (i >= rows) break;
        const int kk = isinf(wb[u]) ? -1 : bin_of(r, wb[u]);
        if (kk != k_cur) {
          flush();
          k_cur = kk;
          acc = {(T)0, (T)0};
        }
        if (kk >= 0) {
          const T c = row_const[i];
          if constexpr (SQ == SSQ_SQUEEZE_LEBESGUE) {
            acc.x += leb_val * c;
          } else if constexpr (SQ == SSQ_SQUEEZE_ABS) {
            acc.x += hypot(Wb[u].x, Wb[u].y) * c;
          } else {
            acc.x += Wb[u].x * c;
            acc.y += Wb[u].y * c;
          }
        }
      }
    }
    flush();
  }
}

int check_shape(int dtype, int64_t batch, int64_t rows, int64_t cols) {
  if (dtype != SSQ_F32 && dtype != SSQ_F64) SSQ_FAIL("dtype must be SSQ_F32 or SSQ_F64");
  if (batch < 1) SSQ_FAIL("batch must be >= 1");
  if (rows < 1 || rows > 32767) SSQ_FAIL("rows must be in [1, 32767]");
  if (cols < 1 || cols > INT32_MAX) SSQ_FAIL("cols must be in [1, 2^31)");
  if ((double)batch * (double)rows * (double)cols * 16.0 > 9.0e18) SSQ_FAIL("transform too large");
  return 0;
}

template <typename T>
int phase_typed(const void* Wx, const void* dWx, const void* Sfs, int64_t batch, int64_t rows, int64_t cols,
                double gamma, void* w, hipStream_t st) {
  const long long planes = (long long)batch * rows;
  const dim3 grid((unsigned)((cols + kPhaseBlock - 1) / kPhaseBlock), (unsigned)std::min<long long>(planes, kMaxGridY));
  const cpx<T>* W = static_cast<const cpx<T>*>(Wx);
  const cpx<T>* dW = static_cast<const cpx<T>*>(dWx);
  if (Sfs)
    hipLaunchKernelGGL((phase_kernel<T, true>), grid, dim3(kPhaseBlock), 0, st, W, dW, static_cast<const T*>(Sfs),
                       planes, (int)rows, (long long)cols, (T)gamma, static_cast<T*>(w));
  else
    hipLaunchKernelGGL((phase_kernel<T, false>), grid, dim3(kPhaseBlock), 0, st, W, dW, (const T*)nullptr, planes,
                       (int)rows, (long long)cols, (T)gamma, static_cast<T*>(w));
  SSQ_HIP(hipGetLastError());
  return 0;
}

template <typename T>
int squeeze_w_typed(const void* Wx, const void* w, int64_t batch, int64_t rows, int64_t cols, const void* row_const,
                    const double* f, int kind, int64_t idx, int squeezing, int flipud, void* Tx, hipStream_t st) {
  BinRule<T> r;
  if (int rc = bin_rule<T>(f, rows, kind, idx, flipud, r)) return rc;
  const size_t out_elem = squeezing == SSQ_SQUEEZE_ABS ? sizeof(T) : sizeof(cpx<T>);
  SSQ_HIP(hipMemsetAsync(Tx, 0, (size_t)(batch * rows * cols) * out_elem, st));
  const dim3 grid((unsigned)((cols + 63) / 64), (unsigned)std::min<int64_t>(batch, kMaxGridY));
  const cpx<T>* W = static_cast<const cpx<T>*>(Wx);
  const T* wv = static_cast<const T*>(w);
  const T* c = static_cast<const T*>(row_const);
  const T leb = (T)(1.0 / (double)rows);
  if (squeezing == SSQ_SQUEEZE_SUM)
    hipLaunchKernelGGL((ssqueeze_w_kernel<T, SSQ_SQUEEZE_SUM>), grid, dim3(64), 0, st, W, wv, c, (long long)batch,
                       (int)rows, (long long)cols, r, leb, Tx);
  else if (squeezing == SSQ_SQUEEZE_LEBESGUE)
    hipLaunchKernelGGL((ssqueeze_w_kernel<T, SSQ_SQUEEZE_LEBESGUE>), grid, dim3(64), 0, st, W, wv, c,
                       (long long)batch, (int)rows, (long long)cols, r, leb, Tx);
  else
    hipLaunchKernelGGL((ssqueeze_w_kernel<T, SSQ_SQUEEZE_ABS>), grid, dim3(64), 0, st, W, wv, c, (long long)batch,
                       (int)rows, (long long)cols, r, leb, Tx);
  SSQ_HIP(hipGetLastError());
  return 0;
}

// from dWx: CWT through cwt_reassign_rows_kernel, one launch per signal (its grid spans one [rows][cols] plane);
// STFT through reassign_cols_kernel, the batch over grid.y
template <typename T>
int squeeze_dwx_typed(const void* Wx, const void* dWx, const void* Sfs, int64_t batch, int64_t rows, int64_t cols,
                      const void* row_const, const double* f, int kind, int64_t idx, int squeezing, int flipud,
                      double gamma, void* Tx, hipStream_t st) {
  BinRule<T> r;
  if (int rc = bin_rule<T>(f, rows, kind, idx, flipud, r)) return rc;
  const long long plane = (long long)rows * cols;
  if (Sfs) {
    if (kind != SSQ_FREQS_LINEAR) SSQ_FAIL("STFT: freq_kind must be SSQ_FREQS_LINEAR");
    if (batch > kMaxGridY) SSQ_FAIL("STFT: batch must be <= 65535");
    StftDev<T> p;
    std::memset(&p, 0, sizeof(p));
    p.out = static_cast<cpx<T>*>(Tx);
    p.ssq_freqs = static_cast<const T*>(Sfs);   // Sfs[i] in the phase, Sfs[0] as the first bin (= ssq_freqs[0])
    p.n_frames = (int)cols;
    p.n_freqs = (int)rows;
    p.out_kind = SSQ_OUT_TX;
    p.squeezing = squeezing;
    p.dw = (T)(f[1] - f[0]);                    // ssqueezing.py:129-130: the weight and the bin width
    p.inv_dw = (T)(1.0 / (f[1] - f[0]));
    p.gamma = (T)gamma;
    p.variant = SSQ_VARIANT_UPSTREAM | (flipud ? SSQ_VARIANT_FLIPUD : 0);
    p.leb_val = (T)((1.0 / (double)rows) * (f[1] - f[0]));
    SSQ_HIP(hipMemsetAsync(Tx, 0, (size_t)(batch * plane) * sizeof(cpx<T>), st));
    SSQ_HIP(launch_reassign_cols<T>(p, static_cast<const cpx<T>*>(Wx), static_cast<const cpx<T>*>(dWx), batch, st));
    return 0;
  }
  CwtSsqDev<T> q;
  std::memset(&q, 0, sizeof(q));
  q.N = cols;
  q.na = (int)rows;
  q.s_begin = 0;
  q.s_end = (int)rows;
  q.is_log = kind != SSQ_FREQS_LINEAR ? 1 : 0;
  q.squeezing = squeezing;
  q.flipud = flipud ? 1 : 0;
  q.bin_min = r.bin_min;
  q.bin_step = r.bin_step;
  q.inv_bin_step = (T)1 / r.bin_step;
  q.gamma = (T)gamma;
  q.leb_val = (T)(1.0 / (double)rows);
  q.variant = 1;
  CwtRowsDev<T> rw{};
  rw.row_const = static_cast<const T*>(row_const);
  rw.piecewise = kind == SSQ_FREQS_LOG_PIECEWISE ? 1 : 0;
  rw.idx1 = r.idx1;
  rw.vlmin1 = r.vlmin1;
  rw.dvl1 = r.dvl1;
  for (int64_t b = 0; b < batch; ++b) {
    q.Wx = static_cast<const cpx<T>*>(Wx) + b * plane;
    q.dWx = static_cast<const cpx<T>*>(dWx) + b * plane;
    q.Tx = static_cast<cpx<T>*>(Tx) + b * plane;
    SSQ_HIP(launch_cwt_reassign<T>(q, st, true, &rw));
  }
  return 0;
}

int upload_row_const(DeviceBufs& d, int dtype, const double* row_const, int64_t rows, void** out) {
  if (!row_const) SSQ_FAIL("row_const is NULL");
  for (int64_t i = 0; i < rows; ++i)
    if (!std::isfinite(row_const[i])) SSQ_FAIL("row_const must be finite");
  if (dtype == SSQ_F32) {
    const std::vector<float> c32(row_const, row_const + rows);
    SSQ_HIP(d.upload(out, c32.data(), (size_t)rows * sizeof(float)));
  } else {
    SSQ_HIP(d.upload(out, row_const, (size_t)rows * sizeof(double)));
  }
  return 0;
}

}  // namespace

extern "C" {

int ssq_phase_exec(int dtype, const void* d_Wx, const void* d_dWx, const void* d_Sfs, int64_t batch, int64_t rows,
                   int64_t cols, double gamma, void* d_w, void* stream) {
  if (int rc = check_shape(dtype, batch, rows, cols)) return rc;
  if (!d_Wx || !d_dWx || !d_w) SSQ_FAIL("NULL argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dtype == SSQ_F64 ? phase_typed<double>(d_Wx, d_dWx, d_Sfs, batch, rows, cols, gamma, d_w, st)
                          : phase_typed<float>(d_Wx, d_dWx, d_Sfs, batch, rows, cols, gamma, d_w, st);
}

int ssq_phase_host(int dtype, const void* Wx, const void* dWx, const void* Sfs, int64_t batch, int64_t rows,
                   int64_t cols, double gamma, void* w) {
  if (int rc = check_shape(dtype, batch, rows, cols)) return rc;
  if (!Wx || !dWx || !w) SSQ_FAIL("NULL argument");
  if (int rc = require_device()) return rc;
  const size_t esz = dtype == SSQ_F64 ? 8 : 4, n = (size_t)(batch * rows * cols);
  DeviceBufs d;
  void *dW = nullptr, *ddW = nullptr, *dS = nullptr, *dw = nullptr;
  SSQ_HIP(d.upload(&dW, Wx, n * 2 * esz));
  SSQ_HIP(d.upload(&ddW, dWx, n * 2 * esz));
  if (Sfs) SSQ_HIP(d.upload(&dS, Sfs, (size_t)rows * esz));
  SSQ_HIP(d.alloc(&dw, n * esz));
  if (int rc = ssq_phase_exec(dtype, dW, ddW, dS, batch, rows, cols, gamma, dw, nullptr)) return rc;
  SSQ_HIP(hipMemcpy(w, dw, n * esz, hipMemcpyDeviceToHost));
  return 0;
}

int ssq_ssqueeze_w_exec(int dtype, const void* d_Wx, const void* d_w, int64_t batch, int64_t rows, int64_t cols,
                        const void* d_row_const, const double* ssq_freqs_asc, int freq_kind, int64_t freq_transition,
                        int squeezing, int flipud, void* d_Tx, void* stream) {
  if (int rc = check_shape(dtype, batch, rows, cols)) return rc;
  if (squeezing != SSQ_SQUEEZE_SUM && squeezing != SSQ_SQUEEZE_LEBESGUE && squeezing != SSQ_SQUEEZE_ABS)
    SSQ_FAIL("squeezing must be SSQ_SQUEEZE_SUM, _LEBESGUE or _ABS");
  if ((!d_Wx && squeezing != SSQ_SQUEEZE_LEBESGUE) || !d_w || !d_row_const || !d_Tx) SSQ_FAIL("NULL argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dtype == SSQ_F64
             ? squeeze_w_typed<double>(d_Wx, d_w, batch, rows, cols, d_row_const, ssq_freqs_asc, freq_kind,
                                       freq_transition, squeezing, flipud, d_Tx, st)
             : squeeze_w_typed<float>(d_Wx, d_w, batch, rows, cols, d_row_const, ssq_freqs_asc, freq_kind,
                                      freq_transition, squeezing, flipud, d_Tx, st);
}

int ssq_ssqueeze_w_host(int dtype, const void* Wx, const void* w, int64_t batch, int64_t rows, int64_t cols,
                        const double* row_const, const double* ssq_freqs_asc, int freq_kind, int64_t freq_transition,
                        int squeezing, int flipud, void* Tx) {
  if (int rc = check_shape(dtype, batch, rows, cols)) return rc;
  if ((!Wx && squeezing != SSQ_SQUEEZE_LEBESGUE) || !w || !Tx) SSQ_FAIL("NULL argument");
  if (int rc = require_device()) return rc;
  const size_t esz = dtype == SSQ_F64 ? 8 : 4, n = (size_t)(batch * rows * cols);
  const size_t tx_bytes = n * (squeezing == SSQ_SQUEEZE_ABS ? esz : 2 * esz);
  DeviceBufs d;
  void *dW = nullptr, *dw = nullptr, *dc = nullptr, *dT = nullptr;
  if (squeezing != SSQ_SQUEEZE_LEBESGUE) SSQ_HIP(d.upload(&dW, Wx, n * 2 * esz));
  SSQ_HIP(d.upload(&dw, w, n * esz));
  if (int rc = upload_row_const(d, dtype, row_const, rows, &dc)) return rc;
  SSQ_HIP(d.alloc(&dT, tx_bytes));
  if (int rc = ssq_ssqueeze_w_exec(dtype, dW, dw, batch, rows, cols, dc, ssq_freqs_asc, freq_kind, freq_transition,
                                   squeezing, flipud, dT, nullptr))
    return rc;
  SSQ_HIP(hipMemcpy(Tx, dT, tx_bytes, hipMemcpyDeviceToHost));
  return 0;
}

int ssq_ssqueeze_dwx_exec(int dtype, const void* d_Wx, const void* d_dWx, const void* d_Sfs, int64_t batch,
                          int64_t rows, int64_t cols, const void* d_row_const, const double* ssq_freqs_asc,
                          int freq_kind, int64_t freq_transition, int squeezing, int flipud, double gamma, void* d_Tx,
                          void* stream) {
  if (int rc = check_shape(dtype, batch, rows, cols)) return rc;
  if (squeezing != SSQ_SQUEEZE_SUM && squeezing != SSQ_SQUEEZE_LEBESGUE)
    SSQ_FAIL("squeezing must be SSQ_SQUEEZE_SUM or _LEBESGUE");
  if (!d_Wx || !d_dWx || !d_Tx || (!d_Sfs && !d_row_const)) SSQ_FAIL("NULL argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dtype == SSQ_F64
             ? squeeze_dwx_typed<double>(d_Wx, d_dWx, d_Sfs, batch, rows, cols, d_row_const, ssq_freqs_asc, freq_kind,
                                         freq_transition, squeezing, flipud, gamma, d_Tx, st)
             : squeeze_dwx_typed<float>(d_Wx, d_dWx, d_Sfs, batch, rows, cols, d_row_const, ssq_freqs_asc, freq_kind,
                                        freq_transition, squeezing, flipud, gamma, d_Tx, st);
}

int ssq_ssqueeze_dwx_host(int dtype, const void* Wx, const void* dWx, const void* Sfs, int64_t batch, int64_t rows,
                          int64_t cols, const double* row_const, const double* ssq_freqs_asc, int freq_kind,
                          int64_t freq_transition, int squeezing, int flipud, double gamma, void* Tx) {
  if (int rc = check_shape(dtype, batch, rows, cols)) return rc;
  if (!Wx || !dWx || !Tx || !ssq_freqs_asc) SSQ_FAIL("NULL argument");
  const size_t esz = dtype == SSQ_F64 ? 8 : 4, n = (size_t)(batch * rows * cols);
  if (Sfs) {                                    // reassign_cols_kernel bins from Sfs[0]
    const double s0 = dtype == SSQ_F64 ? static_cast<const double*>(Sfs)[0] : (double)static_cast<const float*>(Sfs)[0];
    const double f0 = dtype == SSQ_F64 ? ssq_freqs_asc[0] : (double)(float)ssq_freqs_asc[0];
    if (s0 != f0) SSQ_FAIL("STFT from dSx: ssq_freqs_asc[0] must equal Sfs[0]");
  }
  if (int rc = require_device()) return rc;
  DeviceBufs d;
  void *dW = nullptr, *ddW = nullptr, *dS = nullptr, *dc = nullptr, *dT = nullptr;
  SSQ_HIP(d.upload(&dW, Wx, n * 2 * esz));
  SSQ_HIP(d.upload(&ddW, dWx, n * 2 * esz));
  if (Sfs) SSQ_HIP(d.upload(&dS, Sfs, (size_t)rows * esz));
  else if (int rc = upload_row_const(d, dtype, row_const, rows, &dc)) return rc;
  SSQ_HIP(d.alloc(&dT, n * 2 * esz));
  if (int rc = ssq_ssqueeze_dwx_exec(dtype, dW, ddW, dS, batch, rows, cols, dc, ssq_freqs_asc, freq_kind,
                                     freq_transition, squeezing, flipud, gamma, dT, nullptr))
    return rc;
  SSQ_HIP(hipMemcpy(Tx, dT, n * 2 * esz, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
