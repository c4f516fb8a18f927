// api_upstream.hip -- the inverses and the host-side constants of the upstream-parity mode.
// Follows the vendored upstream /root/reference/old/ssqueezepy (the Python library the Rust crate was derived from):
//   istft        _stft.py:196-254, utils/stft_utils.py:141-191
//   issq_stft    _ssq_stft.py:139-198            issq_cwt   _ssq_cwt.py:313-378      (full inverses)
//   adm_ssq/cwt  utils/cwt_utils.py:28-63, :583-627   center_frequency('peak')  wavelets.py:691-716   p2up  common.py:32-51
// The forward transforms of the mode live beside the Rust-variant ones (api_stft.hip, api_cwt.hip: *_v entry points).
#include <cmath>
#include <complex>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/ssq_hip.h"
#include "dev_buffers.h"
#include "fft_generic.h"
#include "host_math.h"
#include "istft_fused.h"

using namespace ssq;

namespace {

// Sx [n_freqs][n_frames] -> Hermitian rows Z [n_frames][n] as numpy.irfft reads them: bins above n/2 are the
// conjugates, the imaginary parts of DC and (even n) Nyquist are ignored
template <typename T>
__global__ void istft_expand_kernel(const cpx<T>* __restrict__ Sx, int n, int n_frames, cpx<T>* __restrict__ Z) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_frames) return;
  for (int k = blockIdx.y; k < n; k += gridDim.y) {          // (grid.y is capped at 65535; n_fft may be larger)
    const int kk = k <= n / 2 ? k : n - k;
    cpx<T> v = Sx[(long long)kk * n_frames + f];
    if (k > n / 2) v.y = -v.y;
    if (k == 0 || (n % 2 == 0 && k == n / 2)) v.y = (T)0;
    Z[(long long)f * n + k] = v;
  }
}

// overlap-add of the windowed frames, window-norm division and unpadding in one gather per output sample
// (utils/stft_utils.py:178-191; _stft.py:238-252)
template <typename T>
__global__ void istft_ola_kernel(const cpx<T>* __restrict__ Y, int n, int n_frames, int hop, long long N, int modulated,
                                 const double* __restrict__ wpow, const double* __restrict__ wnorm, T* __restrict__ x) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const long long p = i + n / 2;                           // position in the padded signal (x[n_fft//2 : ...])
  long long f_lo = p - n + 1 <= 0 ? 0 : (p - n + 1 + hop - 1) / hop;
  long long f_hi = p / hop;
  if (f_hi > n_frames - 1) f_hi = n_frames - 1;
  const int sh = n - n / 2;                                // fftshift: xbuf[m] = y[(m + n - n//2) mod n]
  const double inv_n = 1.0 / (double)n;
  double acc = 0.0, wn = 0.0;
  for (long long f = f_lo; f <= f_hi; ++f) {
    const int m = (int)(p - f * hop);
    int src = modulated ? m + sh : m;
    if (src >= n) src -= n;
    acc += (double)Y[f * n + src].x * inv_n * wpow[m];
    wn += wnorm[m];
  }
  const double tiny = sizeof(T) == 4 ? 1.1754943508222875e-38 : 2.2250738585072014e-308;
  x[i] = (T)(wn > tiny ? acc / wn : acc);
}

// x[b][j] = scale * sum_r Re Tx[b][r][j] * row_scale[r] (row_scale NULL: 1), one signal per blockIdx.y, accumulated in
// fp64 with the rows in order
template <typename T>
__global__ void issq_colsum_batch_kernel(const cpx<T>* __restrict__ Tx_all, long long rows, long long cols, double scale,
                                         const double* __restrict__ row_scale, T* __restrict__ x_all) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cols) return;
  const cpx<T>* __restrict__ Tx = Tx_all + (long long)blockIdx.y * rows * cols;
  T* __restrict__ x = x_all + (long long)blockIdx.y * cols;
  double acc = 0.0;
  if (row_scale) {
    for (long long r = 0; r < rows; ++r) acc += (double)Tx[r * cols + j].x * row_scale[r];
  } else {
    for (long long r = 0; r < rows; ++r) acc += (double)Tx[r * cols + j].x;
  }
  x[j] = (T)(acc * scale);
}

// the three kernels of one signal on device buffers: d_Z [n_frames][n], d_work fft_work_elems(n, n_frames) elements
template <typename T>
hipError_t istft_three_dev(const cpx<T>* d_S, int64_t n_frames, const double* d_wp, const double* d_wn, int64_t n, int64_t hop,
                           int64_t N, int modulated, cpx<T>* d_Z, cpx<T>* d_work, T* d_x) {
  hipLaunchKernelGGL(istft_expand_kernel<T>, dim3((unsigned)((n_frames + 255) / 256), (unsigned)(n < 65535 ? n : 65535)), dim3(256), 0,
                     nullptr,
                     d_S, (int)n, (int)n_frames, d_Z);
  hipError_t e = fft_any_batched<T>(d_Z, d_work, n, n_frames, +1, nullptr);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(istft_ola_kernel<T>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, nullptr, d_Z, (int)n,
                     (int)n_frames, (int)hop, (long long)N, modulated, d_wp, d_wn, d_x);
  return hipGetLastError();
}

template <typename T>
int istft_typed(const void* Sx, int64_t n_frames, const std::vector<double>& wpow, const std::vector<double>& wnorm,
                int64_t n, int64_t hop, int64_t N, int modulated, void* x_out) {
  const int64_t nf = n / 2 + 1;
  const long long we = fft_work_elems(n, n_frames);
  DeviceBufs d;
  void *d_S, *d_Z, *d_work, *d_wp, *d_wn, *d_x;
  SSQ_HIP(d.upload(&d_S, Sx, sizeof(cpx<T>) * nf * n_frames));
  SSQ_HIP(d.alloc(&d_Z, sizeof(cpx<T>) * n * n_frames));
  SSQ_HIP(d.alloc(&d_work, sizeof(cpx<T>) * (we > 0 ? we : 1)));
  SSQ_HIP(d.upload(&d_wp, wpow.data(), sizeof(double) * n));
  SSQ_HIP(d.upload(&d_wn, wnorm.data(), sizeof(double) * n));
  SSQ_HIP(d.alloc(&d_x, sizeof(T) * N));
  SSQ_HIP(istft_three_dev<T>((const cpx<T>*)d_S, n_frames, (const double*)d_wp, (const double*)d_wn, n, hop, N, modulated,
                             (cpx<T>*)d_Z, (cpx<T>*)d_work, (T*)d_x));
  SSQ_HIP(hipMemcpy(x_out, d_x, sizeof(T) * N, hipMemcpyDeviceToHost));
  return 0;
}

// exp(-2 pi i k / n), k < n: the twiddle table of the fused inverse
template <typename T>
std::vector<cpx<T>> istft_twiddles(int64_t n) {
  std::vector<cpx<T>> tw((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const long double ang = 2.0L * 3.14159265358979323846264338327950288L * (long double)i / (long double)n;
    tw[i] = {(T)cosl(ang), (T)(-sinl(ang))};
  }
  return tw;
}

// Device bytes of the fused path for `slice` signals: Sx in, x out and the three tables
template <typename T>
double istft_fused_bytes(const IstftPlan& pl, long long slice, long long N, bool with_sx) {
  const double nf = (double)(pl.n / 2 + 1);
  double per = (double)sizeof(T) * (double)N;
  if (with_sx) per += (double)sizeof(cpx<T>) * nf * (double)pl.n_frames;
  return per * (double)slice + (double)pl.n * (16.0 + (double)sizeof(cpx<T>));
}

template <typename T>
int istft_batch_fused(const IstftPlan& pl, const void* Sx, int64_t batch, const std::vector<double>& wpow,
                      const std::vector<double>& wnorm, int64_t N, int modulated, void* x_out) {
  const int64_t n = pl.n, nf = n / 2 + 1, n_frames = pl.n_frames;
  const long long slice = slice_signals(batch, istft_fused_bytes<T>(pl, 1, N, true) - istft_fused_bytes<T>(pl, 0, N, true),
                                        istft_fused_bytes<T>(pl, 0, N, true), 65535);
  const std::vector<cpx<T>> tw = istft_twiddles<T>(n);
  const size_t sx_sig = sizeof(cpx<T>) * (size_t)nf * (size_t)n_frames;
  DeviceBufs d;
  void *d_S, *d_x, *d_tw, *d_wp, *d_wn;
  SSQ_HIP(d.alloc(&d_S, sx_sig * slice));
  SSQ_HIP(d.alloc(&d_x, sizeof(T) * (size_t)N * slice));
  SSQ_HIP(d.upload(&d_tw, tw.data(), sizeof(cpx<T>) * n));
  SSQ_HIP(d.upload(&d_wp, wpow.data(), sizeof(double) * n));
  SSQ_HIP(d.upload(&d_wn, wnorm.data(), sizeof(double) * n));
  for (int64_t b0 = 0; b0 < batch; b0 += slice) {
    const int64_t nb = batch - b0 < slice ? batch - b0 : slice;
    SSQ_HIP(hipMemcpy(d_S, (const char*)Sx + sx_sig * b0, sx_sig * nb, hipMemcpyHostToDevice));
    SSQ_HIP(launch_istft_fused<T>(pl, (const cpx<T>*)d_S, nb, N, modulated, (const cpx<T>*)d_tw, (const double*)d_wp,
                                  (const double*)d_wn, (T*)d_x, nullptr));
    SSQ_HIP(hipMemcpy((char*)x_out + sizeof(T) * (size_t)N * b0, d_x, sizeof(T) * (size_t)N * nb, hipMemcpyDeviceToHost));
  }
  return 0;
}

template <typename T>
int issq_batch_typed(const void* Tx, int64_t batch, int64_t rows, int64_t cols, double scale, const double* row_scale,
                     void* x_out) {
  const size_t map_b = sizeof(cpx<T>) * (size_t)rows * (size_t)cols;
  const long long slice = slice_signals(batch, (double)map_b + (double)sizeof(T) * (double)cols, 8.0 * (double)rows, 65535);
  DeviceBufs d;
  void *d_T, *d_x, *d_r = nullptr;
  SSQ_HIP(d.alloc(&d_T, map_b * slice));
  SSQ_HIP(d.alloc(&d_x, sizeof(T) * (size_t)cols * slice));
  if (row_scale) SSQ_HIP(d.upload(&d_r, row_scale, sizeof(double) * rows));
  for (int64_t b0 = 0; b0 < batch; b0 += slice) {
    const int64_t nb = batch - b0 < slice ? batch - b0 : slice;
    SSQ_HIP(hipMemcpy(d_T, (const char*)Tx + map_b * b0, map_b * nb, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(issq_colsum_batch_kernel<T>, dim3((unsigned)((cols + 255) / 256), (unsigned)nb), dim3(256), 0, nullptr,
                       (const cpx<T>*)d_T, (long long)rows, (long long)cols, scale, (const double*)d_r, (T*)d_x);
    SSQ_HIP(hipGetLastError());
    SSQ_HIP(hipMemcpy((char*)x_out + sizeof(T) * (size_t)cols * b0, d_x, sizeof(T) * (size_t)cols * nb, hipMemcpyDeviceToHost));
  }
  return 0;
}

// The inverse of a batch that already lives on the device (d_Sx, d_x), by the path asked for; the kernels' own time
// (HIP events around the launches, tables and workspace set up before) goes to *kernel_ms when it is not NULL.
template <typename T>
int istft_batch_exec_typed(const void* d_Sx, int64_t batch, int64_t n_frames, const std::vector<double>& wpow,
                           const std::vector<double>& wnorm, int64_t n, int64_t hop, int64_t N, int modulated, bool fused,
                           const IstftPlan& pl, void* d_x_out, float* kernel_ms) {
  const int64_t nf = n / 2 + 1;
  const cpx<T>* d_S = (const cpx<T>*)d_Sx;
  T* d_x = (T*)d_x_out;
  DeviceBufs d;
  void *d_wp, *d_wn, *d_tw = nullptr, *d_Z = nullptr, *d_work = nullptr;
  SSQ_HIP(d.upload(&d_wp, wpow.data(), sizeof(double) * n));
  SSQ_HIP(d.upload(&d_wn, wnorm.data(), sizeof(double) * n));
  if (fused) {
    const std::vector<cpx<T>> tw = istft_twiddles<T>(n);
    SSQ_HIP(d.upload(&d_tw, tw.data(), sizeof(cpx<T>) * n));
  } else {
    const long long we = fft_work_elems(n, n_frames);
    SSQ_HIP(d.alloc(&d_Z, sizeof(cpx<T>) * n * n_frames));
    SSQ_HIP(d.alloc(&d_work, sizeof(cpx<T>) * (we > 0 ? we : 1)));
  }
  return run_timed(kernel_ms, 0, nullptr, [&](const hipEvent_t*) -> int {
    if (fused) {
      for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
        const int64_t nb = batch - b0 < 65535 ? batch - b0 : 65535;
        SSQ_HIP(launch_istft_fused<T>(pl, d_S + b0 * nf * n_frames, nb, N, modulated, (const cpx<T>*)d_tw, (const double*)d_wp,
                                      (const double*)d_wn, d_x + b0 * N, nullptr));
      }
    } else {
      for (int64_t b = 0; b < batch; ++b)
        SSQ_HIP(istft_three_dev<T>(d_S + b * nf * n_frames, n_frames, (const double*)d_wp, (const double*)d_wn, n, hop, N,
                                   modulated, (cpx<T>*)d_Z, (cpx<T>*)d_work, d_x + b * N));
    }
    return 0;
  });
}

// The argument checks the three ssq_istft_* entry points share, in their order (batch: 1 for the single-signal form)
int istft_args(int dtype, const void* Sx, int64_t batch, int64_t n_frames, const double* window, int64_t n_fft, int64_t hop,
               int64_t n_signal, int win_exp, const void* x_out) {
  if (!Sx || !window || !x_out) SSQ_FAIL("NULL argument");
  if (dtype != SSQ_F32 && dtype != SSQ_F64) SSQ_FAIL("dtype must be SSQ_F32 or SSQ_F64");
  if (batch < 1) SSQ_FAIL("batch must be >= 1");
  if (n_fft < 1 || hop < 1 || n_frames < 1 || n_signal < 1 || win_exp < 0) SSQ_FAIL("bad istft shape");
  if (n_fft > (1 << 24)) SSQ_FAIL("n_fft too large");
  if ((n_signal - 1) / hop + 1 != n_frames) SSQ_FAIL("Sx has the wrong number of frames for (N, hop_len)");
  return 0;
}

// The window's two tables, built once every check has passed: wpow = window^win_exp (utils/stft_utils.py:159-162),
// wnorm = window^(win_exp+1) (:186)
void istft_window_tables(const double* window, int64_t n_fft, int win_exp, std::vector<double>& wpow, std::vector<double>& wnorm) {
  wpow.resize((size_t)n_fft);
  wnorm.resize((size_t)n_fft);
  for (int64_t i = 0; i < n_fft; ++i) {
    wpow[i] = win_exp == 0 ? 1.0 : std::pow(window[i], (double)win_exp);
    wnorm[i] = std::pow(window[i], (double)(win_exp + 1));
  }
}

// Which path a shape takes: the fused kernel where it takes the shape and the signal has enough tiles to fill the device.
// SSQ_ISTFT_FUSED in the environment (A/B): 0 never, 1 wherever the kernel takes the shape.
bool istft_use_fused(int64_t n, int64_t hop, int64_t n_frames, IstftPlan* pl) {
  if (!istft_fused_plan(n, hop, n_frames, pl)) return false;
  if (const char* e = std::getenv("SSQ_ISTFT_FUSED")) return std::atoi(e) != 0;
  return pl->preferred;
}

// ---- upstream wavelets in fp64 (host) ----
double gmw_l1(double w, double gamma, double beta) {             // _gmw.py:204-210
  if (!(w >= 0.0)) return 0.0;
  const double wc = std::exp((1.0 / gamma) * (std::log(beta) - std::log(gamma)));   // _gmw.py:611-657 morsefreq
  const double wcl = std::log(wc);
  if (w == 0.0) return 0.0;                                        // exp(beta * log 0) = exp(-inf)
  return 2.0 * std::exp(-beta * wcl + std::pow(wc, gamma) + beta * std::log(w) - std::pow(w, gamma));
}
double morlet_up(double w, double mu) {                          // wavelets.py:497-523
  const double cs = std::pow(1.0 + std::exp(-mu * mu) - 2.0 * std::exp(-0.75 * mu * mu), -0.5);
  const double ks = std::exp(-0.5 * mu * mu);
  return std::sqrt(2.0) * cs * std::pow(M_PI, 0.25) * (std::exp(-0.5 * (w - mu) * (w - mu)) - ks * std::exp(-0.5 * w * w));
}
double psih_up(int wavelet, double p0, double p1, double w) {
  return wavelet == SSQ_WAVELET_MORLET ? morlet_up(w, p0) : gmw_l1(w, p0, p1);
}

double trapz(const std::vector<double>& y, const std::vector<double>& t, size_t n) {
  double s = 0.0;
  for (size_t i = 1; i < n; ++i) s += 0.5 * (y[i] + y[i - 1]) * (t[i] - t[i - 1]);
  return s;
}

// utils/cwt_utils.py:583-627 for a real, non-negative integrand
double integrate_analytic(int wavelet, double p0, double p1, bool squared) {
  auto fn = [&](double w) {
    const double v = psih_up(wavelet, p0, p1, w);
    return (squared ? v * v : v) / w;
  };
  std::vector<double> t0(1000), a0(1000);
  for (int i = 0; i < 1000; ++i) {                                 // np.logspace(-15, -1, 1000)
    t0[i] = std::pow(10.0, -15.0 + 14.0 * (double)i / 999.0);
    a0[i] = fn(t0[i]);
  }
  const double int_nz = trapz(a0, t0, 1000);
  const int ms[4] = {1, 1, 4, 8};
  const double lims[4] = {1, 20, 80, 160};
  std::vector<double> t, arr;
  size_t keep = 0;
  for (int c = 0; c < 4; ++c) {
    const size_t n = (size_t)10000 * ms[c];
    t.assign(n, 0.0);
    arr.assign(n, 0.0);
    const double step = (0.1 - lims[c]) / (double)n;               // np.linspace(mxlim, .1, n, endpoint=False)[::-1]
    for (size_t i = 0; i < n; ++i) t[n - 1 - i] = lims[c] + (double)i * step;
    size_t mi = 0;
    double sum_abs = 0.0;
    for (size_t i = 0; i < n; ++i) {
      arr[i] = fn(t[i]);
      sum_abs += std::fabs(arr[i]);
      if (arr[i] > arr[mi]) mi = i;
    }
    size_t idx = n - 1 - mi;                                       // algos.py:616-622 on |arr[mi:]|, th = 1e-15
    for (size_t i = mi; i < n; ++i)
      if (std::fabs(arr[i]) < 1e-15) {
        idx = i - mi;
        break;
      }
    keep = idx + mi;
    if ((n - keep > (size_t)1000 * ms[c]) && sum_abs > 1e-5) break;
  }
  return trapz(arr, t, keep) + int_nz;
}

}  // namespace

extern "C" {

int ssq_istft_host(int dtype, const void* Sx, int64_t n_frames, const double* window, int64_t n_fft, int64_t hop,
                   int64_t n_signal, int modulated, int win_exp, void* x_out) {
  if (int rc = istft_args(dtype, Sx, 1, n_frames, window, n_fft, hop, n_signal, win_exp, x_out)) return rc;
  if (int rc = require_device()) return rc;
  std::vector<double> wpow, wnorm;
  istft_window_tables(window, n_fft, win_exp, wpow, wnorm);
  return dtype == SSQ_F32 ? istft_typed<float>(Sx, n_frames, wpow, wnorm, n_fft, hop, n_signal, modulated, x_out)
                          : istft_typed<double>(Sx, n_frames, wpow, wnorm, n_fft, hop, n_signal, modulated, x_out);
}

int ssq_istft_batch_host(int dtype, const void* Sx, int64_t batch, int64_t n_frames, const double* window, int64_t n_fft,
                         int64_t hop, int64_t n_signal, int modulated, int win_exp, void* x_out) {
  if (int rc = istft_args(dtype, Sx, batch, n_frames, window, n_fft, hop, n_signal, win_exp, x_out)) return rc;
  if (int rc = require_device()) return rc;
  std::vector<double> wpow, wnorm;
  istft_window_tables(window, n_fft, win_exp, wpow, wnorm);
  IstftPlan pl;
  if (istft_use_fused(n_fft, hop, n_frames, &pl))
    return dtype == SSQ_F32 ? istft_batch_fused<float>(pl, Sx, batch, wpow, wnorm, n_signal, modulated, x_out)
                            : istft_batch_fused<double>(pl, Sx, batch, wpow, wnorm, n_signal, modulated, x_out);
  // every other length: the three-kernel path, one signal at a time (its [n_frames][n_fft] workspace is per signal)
  const size_t esz = dtype == SSQ_F32 ? 4 : 8;
  const size_t sx_sig = 2 * esz * (size_t)(n_fft / 2 + 1) * (size_t)n_frames;
  for (int64_t b = 0; b < batch; ++b) {
    const void* S = (const char*)Sx + sx_sig * b;
    void* xo = (char*)x_out + esz * (size_t)n_signal * b;
    const int rc = dtype == SSQ_F32 ? istft_typed<float>(S, n_frames, wpow, wnorm, n_fft, hop, n_signal, modulated, xo)
                                    : istft_typed<double>(S, n_frames, wpow, wnorm, n_fft, hop, n_signal, modulated, xo);
    if (rc) return rc;
  }
  return 0;
}

int ssq_istft_batch_exec(int dtype, const void* d_Sx, int64_t batch, int64_t n_frames, const double* window, int64_t n_fft,
                         int64_t hop, int64_t n_signal, int modulated, int win_exp, int path, void* d_x, float* kernel_ms) {
  if (int rc = istft_args(dtype, d_Sx, batch, n_frames, window, n_fft, hop, n_signal, win_exp, d_x)) return rc;
  if (path < -1 || path > 1) SSQ_FAIL("path must be -1 (as ssq_istft_batch_host chooses), 0 (three kernels) or 1 (fused)");
  if (int rc = require_device()) return rc;
  IstftPlan pl;
  const bool can = istft_fused_plan(n_fft, hop, n_frames, &pl);
  if (path == 1 && !can) SSQ_FAIL("the fused istft kernel does not take this (n_fft, hop_len)");
  std::vector<double> wpow, wnorm;
  istft_window_tables(window, n_fft, win_exp, wpow, wnorm);
  const bool fused = path == 1 || (path == -1 && istft_use_fused(n_fft, hop, n_frames, &pl));
  return dtype == SSQ_F32
             ? istft_batch_exec_typed<float>(d_Sx, batch, n_frames, wpow, wnorm, n_fft, hop, n_signal, modulated, fused, pl, d_x, kernel_ms)
             : istft_batch_exec_typed<double>(d_Sx, batch, n_frames, wpow, wnorm, n_fft, hop, n_signal, modulated, fused, pl, d_x, kernel_ms);
}

int64_t ssq_istft_batch_workspace_bytes(int dtype, int64_t batch, int64_t n_frames, int64_t n_fft, int64_t hop,
                                        int64_t n_signal, int* fused) {
  if (fused) *fused = 0;
  if ((dtype != SSQ_F32 && dtype != SSQ_F64) || batch < 1 || n_fft < 1 || n_fft > (1 << 24) || hop < 1 || n_frames < 1 ||
      n_signal < 1) {
    set_error("bad istft shape");
    return -1;
  }
  const double csz = dtype == SSQ_F32 ? 8.0 : 16.0;
  IstftPlan pl;
  if (istft_use_fused(n_fft, hop, n_frames, &pl)) {
    if (fused) *fused = 1;
    return (int64_t)(dtype == SSQ_F32 ? istft_fused_bytes<float>(pl, batch, n_signal, false)
                                      : istft_fused_bytes<double>(pl, batch, n_signal, false));
  }
  const long long we = fft_work_elems(n_fft, n_frames);
  return (int64_t)(csz * ((double)n_fft * (double)n_frames + (double)(we > 0 ? we : 1)) + 16.0 * (double)n_fft +
                   0.5 * csz * (double)n_signal);
}

int ssq_issq_batch_host(int dtype, const void* Tx, int64_t batch, int64_t rows, int64_t cols, double scale,
                        const double* row_scale, void* x_out) {
  if (!Tx || !x_out) SSQ_FAIL("NULL argument");
  if (dtype != SSQ_F32 && dtype != SSQ_F64) SSQ_FAIL("dtype must be SSQ_F32 or SSQ_F64");
  if (batch < 1) SSQ_FAIL("batch must be >= 1");
  if (rows < 1 || cols < 1) SSQ_FAIL("empty Tx");
  if (int rc = require_device()) return rc;
  return dtype == SSQ_F32 ? issq_batch_typed<float>(Tx, batch, rows, cols, scale, row_scale, x_out)
                          : issq_batch_typed<double>(Tx, batch, rows, cols, scale, row_scale, x_out);
}

int ssq_issq_host(int dtype, const void* Tx, int64_t rows, int64_t cols, double scale, const double* row_scale,
                  void* x_out) {
  if (!Tx || !x_out) SSQ_FAIL("NULL argument");
  if (dtype != SSQ_F32 && dtype != SSQ_F64) SSQ_FAIL("dtype must be SSQ_F32 or SSQ_F64");
  if (rows < 1 || cols < 1) SSQ_FAIL("empty Tx");
  if (int rc = require_device()) return rc;
  return dtype == SSQ_F32 ? issq_batch_typed<float>(Tx, 1, rows, cols, scale, row_scale, x_out)   // one signal: a batch of one
                          : issq_batch_typed<double>(Tx, 1, rows, cols, scale, row_scale, x_out);
}

int ssq_upstream_adm(int wavelet, double p0, double p1, int which_cwt, double* out) {
  if (!out) SSQ_FAIL("out is NULL");
  if (wavelet != SSQ_WAVELET_GMW && wavelet != SSQ_WAVELET_MORLET) SSQ_FAIL("unknown wavelet");
  *out = integrate_analytic(wavelet, p0, p1, which_cwt != 0);
  return 0;
}

int ssq_upstream_center_frequency(int wavelet, double p0, double p1, double scale, int64_t n, double* wc) {
  if (!wc || n < 2) SSQ_FAIL("bad arguments");
  if (wavelet != SSQ_WAVELET_GMW && wavelet != SSQ_WAVELET_MORLET) SSQ_FAIL("unknown wavelet");
  const double h = (2.0 * M_PI) / (double)n;
  auto xi = [&](int64_t i) { return i <= n / 2 ? (double)i * h : (double)(i - n) * h; };   // wavelets.py:473-483
  // grid order of wavelets.py:950-962 (aifftshift), first maximum wins like np.argmax
  double best = -1.0, best_w = 0.0;
  auto visit = [&](int64_t i) {
    const double w = xi(i);
    const double v = psih_up(wavelet, p0, p1, scale * w);
    if (v * v > best) {
      best = v * v;
      best_w = w;
    }
  };
  if (n % 2 == 0) {
    for (int64_t i = n / 2 + 1; i < n; ++i) visit(i);
    for (int64_t i = 0; i <= n / 2; ++i) visit(i);
  } else {
    for (int64_t i = n / 2; i < n; ++i) visit(i);           // np.fft.ifftshift for odd n: starts at n//2
    for (int64_t i = 0; i < n / 2; ++i) visit(i);
  }
  *wc = best_w;
  return 0;
}

int ssq_upstream_psih(int wavelet, double p0, double p1, const double* w, int64_t n, double* out) {
  if (!w || !out || n < 0) SSQ_FAIL("bad arguments");
  if (wavelet != SSQ_WAVELET_GMW && wavelet != SSQ_WAVELET_MORLET) SSQ_FAIL("unknown wavelet");
  for (int64_t i = 0; i < n; ++i) out[i] = psih_up(wavelet, p0, p1, w[i]);
  return 0;
}

int ssq_upstream_p2up(int64_t n_signal, int64_t* n_up, int64_t* n1, int64_t* n2) {
  if (n_signal < 1 || !n_up || !n1 || !n2) SSQ_FAIL("bad arguments");
  host::p2up(n_signal, n_up, n1, n2);
  return 0;
}

}  // extern "C"
