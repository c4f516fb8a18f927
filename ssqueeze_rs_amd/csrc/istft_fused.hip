// istft_fused.hip -- ssqueezepy.istft as one streaming kernel (old/ssqueezepy/_stft.py:196-254,
// utils/stft_utils.py:141-191).  A workgroup of 256 lanes owns a tile of consecutive frames of one signal.  Per round it
// loads the n/2+1 bins of 256 / (n/16) frames from the frequency-major Sx, extends them Hermitian in registers
// (istft_expand_kernel's rule), runs the inverse FFT of fft_core.h, leaves the real parts in LDS and gathers them,
// windowed, into an fp64 LDS accumulator in ascending frame order.  Finished samples are divided by the window norm,
// unpadded and stored.  A tile after the first starts (n - 1) / hop frames early (the halo: every frame that reaches into
// its samples) and stores only its own samples, so that every sample is one sum over its frames in ascending order --
// the order of istft_ola_kernel and of upstream's loop -- whatever the tiling.  No atomics, no scratch.
#include "fft_core.h"
#include "istft_fused.h"

namespace ssq {

template <typename T>
struct IstftDev {
  const cpx<T>* Sx;
  const cpx<T>* tw;
  const double* wpow;
  const double* wnorm;
  T* x;
  long long n_frames, n_signal, tiles;
  int hop, keep, halo, rf, tf, modulated;
};

// one finished sample of the padded signal: window-norm division (the covering frames in ascending order) and unpadding
template <typename T, int N>
__device__ __forceinline__ void istft_emit(const IstftDev<T>& p, T* __restrict__ x, long long pp, double a) {
  const long long i = pp - N / 2;
  if (i < 0 || i >= p.n_signal) return;
  const long long f_lo = pp - N + 1 <= 0 ? 0 : (pp - N + p.hop) / p.hop;
  long long f_hi = pp / p.hop;
  if (f_hi > p.n_frames - 1) f_hi = p.n_frames - 1;
  double wn = 0.0;
  for (long long f = f_lo; f <= f_hi; ++f) wn += p.wnorm[pp - f * p.hop];
  const double tiny = sizeof(T) == 4 ? 1.1754943508222875e-38 : 2.2250738585072014e-308;
  x[i] = (T)(wn > tiny ? a / wn : a);
}

template <typename T, int LOGN>
__global__ __launch_bounds__(kIstftThreads) void istft_fused_kernel(const IstftDev<T> p) {
  constexpr int N = 1 << LOGN, L = N / 16, FPR = kIstftThreads / L, ROW = N + N / 16, NP = N + 1;
  constexpr bool MULTI = L > 64;
  static_assert(FPR * NP * sizeof(T) <= FPR * ROW * sizeof(cpx<T>), "the real rows reuse the exchange rows");
  __shared__ double acc[kIstftAcc];
  __shared__ __attribute__((aligned(16))) cpx<T> exch_all[FPR * ROW];
  T* ybuf = reinterpret_cast<T*>(exch_all);               // [FPR][N + 1] real parts of a round's frames

  const int tid = threadIdx.x;
  int g, t;                                                // frame slot of the round, lane inside the frame
  if constexpr (MULTI) {
    t = tid % L;
    g = tid / L;
  } else {                                                 // a wave's frames interleaved: neighbouring lanes load
    constexpr int FPW = 64 / L;                            // neighbouring frames of one bin
    g = (tid >> 6) * FPW + (tid & 63) % FPW;
    t = (tid & 63) / FPW;
  }
  cpx<T>* exch = exch_all + g * ROW;

  const long long tile = blockIdx.x, b = blockIdx.y;
  const long long nfr = p.n_frames;
  const cpx<T>* __restrict__ Sx = p.Sx + b * (long long)(N / 2 + 1) * nfr;
  T* __restrict__ x = p.x + b * p.n_signal;
  const int hop = p.hop, keep = p.keep, rf = p.rf;
  const long long f_tile = tile * p.tf;
  const long long f_end = f_tile + p.tf < nfr ? f_tile + p.tf : nfr;
  const bool last = tile == p.tiles - 1;
  const long long f_begin = f_tile > p.halo ? f_tile - p.halo : 0;
  const int sh = N - N / 2;                                // fftshift: xbuf[m] = y[(m + n - n//2) mod n]
  const double inv_n = 1.0 / (double)N;
  const cpx<T> no_regs[3][16] = {};

  for (int i = tid; i < kIstftAcc; i += kIstftThreads) acc[i] = 0.0;
  __syncthreads();

  for (long long fc = f_begin; fc < f_end; fc += rf) {     // a chunk: the accumulator's span
    const int nch = (int)(f_end - fc < rf ? f_end - fc : rf);
    for (int r0 = 0; r0 < nch; r0 += FPR) {                // a round: FPR frames transformed side by side
      const bool valid = r0 + g < nch;
      const long long f = fc + r0 + g;
      cpx<T> v[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int idx = t + L * q;
        const int kk = idx <= N / 2 ? idx : N - idx;
        cpx<T> s = {(T)0, (T)0};
        if (valid) s = Sx[(long long)kk * nfr + f];
        if (idx > N / 2) s.y = -s.y;
        if (idx == 0 || idx == N / 2) s.y = (T)0;
        v[q] = s;
      }
      fft_pass<T, LOGN, 0, true, false, MULTI>(v, exch, no_regs, p.tw, t);
      __syncthreads();                                     // every frame is out of its exchange row
#pragma unroll
      for (int q = 0; q < 16; ++q) ybuf[g * NP + t + L * q] = v[q].x;
      __syncthreads();
      const int nr = nch - r0 < FPR ? nch - r0 : FPR;
      const int s0 = r0 * hop, cnt = (nr - 1) * hop + N;
      for (int j = tid; j < cnt; j += kIstftThreads) {
        int g_hi = j / hop;
        if (g_hi > nr - 1) g_hi = nr - 1;
        const int g_lo = j - N + 1 <= 0 ? 0 : (j - N + hop) / hop;
        double a = acc[s0 + j];
        for (int gg = g_lo; gg <= g_hi; ++gg) {
          const int m = j - gg * hop;
          int src = p.modulated ? m + sh : m;
          if (src >= N) src -= N;
          a += (double)ybuf[gg * NP + src] * inv_n * p.wpow[m];
        }
        acc[s0 + j] = a;
      }
      __syncthreads();
    }
    // ---- the chunk's finished samples: [0, nch * hop), and the rest of the last frame at the end of the signal ----
    const bool last_chunk = fc + rf >= f_end;
    const int body = (last_chunk && last) ? (nch - 1) * hop + N : nch * hop;
    const long long p0 = fc * hop, pt = f_tile * hop;
    for (int s = tid; s < body; s += kIstftThreads) {
      const long long pp = p0 + s;
      if (pp >= pt) istft_emit<T, N>(p, x, pp, acc[s]);         // below: the halo, the tile before stores those
    }
    if (!last_chunk) {                                             // carry the unfinished n - hop samples to the front
      __syncthreads();
      double carry[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int j = tid + kIstftThreads * u;
        carry[u] = j < keep ? acc[rf * hop + j] : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int j = tid + kIstftThreads * u;
        if (j < keep) acc[j] = carry[u];
      }
      for (int j = keep + tid; j < rf * hop + keep; j += kIstftThreads) acc[j] = 0.0;
      __syncthreads();
    }
  }
}

bool istft_fused_plan(long long n, long long hop, long long n_frames, IstftPlan* pl) {
  int logn = 0;
  while ((1LL << logn) < n) ++logn;
  if (n < 16 || n > 4096 || (1LL << logn) != n || hop < 1 || hop > n || n_frames < 1 || n_frames > (1LL << 30)) return false;
  pl->logn = logn;
  pl->n = (int)n;
  pl->hop = (int)hop;
  pl->keep = (int)(n - hop);
  pl->fpr = kIstftThreads / (int)(n / 16);
  const int per = (kIstftAcc - pl->keep) / (pl->fpr * pl->hop);        // >= 1: (fpr - 1) * hop + n <= 4096
  pl->rf = pl->fpr * (per > 1 ? per : 1);
  pl->halo = (int)((n - 1) / hop);                                       // the earlier frames that reach into a tile
  long long tf_min = 2LL * pl->halo;                                     // at most a third of a tile's frames are halo
  if (tf_min < 16) tf_min = 16;                                          // and a tile reads whole 128-byte runs of a bin
  long long tf = 16 * ((tf_min + 15) / 16);                              // (a tile may be shorter than a chunk)
  const long long grow = ((n_frames + tf - 1) / tf) / 1024;              // long signals: at most ~2000 longer tiles (less halo)
  if (grow > 1) tf *= grow;
  pl->tf = (int)tf;
  pl->n_frames = n_frames;
  pl->tiles = (n_frames + tf - 1) / tf;
  // Fewer workgroups than CUs per signal: the three-kernel path, which spreads the frames over the whole device, is
  // faster (profiles/inverse_batch.txt: 0.5 - 0.9 x at 64 and 128 tiles, 2 - 3 x at 256).  Decided per signal, not per
  // batch, so that a signal's bits do not depend on the batch it is in.
  pl->preferred = pl->tiles >= kIstftMinTiles;
  return true;
}

template <typename T, int LOGN>
static hipError_t launch_one(const IstftDev<T>& p, long long batch, hipStream_t stream) {
  hipLaunchKernelGGL((istft_fused_kernel<T, LOGN>), dim3((unsigned)p.tiles, (unsigned)batch), dim3(kIstftThreads), 0, stream, p);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_istft_fused(const IstftPlan& pl, const cpx<T>* d_Sx, long long batch, long long n_signal, int modulated,
                              const cpx<T>* d_tw, const double* d_wpow, const double* d_wnorm, T* d_x,
                              hipStream_t stream) {
  if (batch < 1 || batch > 65535 || pl.tiles > 65535) return hipErrorInvalidValue;
  if ((long long)pl.rf * pl.hop + pl.keep > kIstftAcc) return hipErrorInvalidValue;
  IstftDev<T> p;
  p.Sx = d_Sx;
  p.tw = d_tw;
  p.wpow = d_wpow;
  p.wnorm = d_wnorm;
  p.x = d_x;
  p.n_frames = pl.n_frames;
  p.n_signal = n_signal;
  p.tiles = pl.tiles;
  p.hop = pl.hop;
  p.keep = pl.keep;
  p.halo = pl.halo;
  p.rf = pl.rf;
  p.tf = pl.tf;
  p.modulated = modulated;
  // samples no frame covers (hop > n/2 at the end of the signal) stay zero, as the gather of the three-kernel path leaves them
  hipError_t e = hipMemsetAsync(d_x, 0, sizeof(T) * (size_t)batch * (size_t)n_signal, stream);
  if (e != hipSuccess) return e;
  switch (pl.logn) {
    case 4: return launch_one<T, 4>(p, batch, stream);
    case 5: return launch_one<T, 5>(p, batch, stream);
    case 6: return launch_one<T, 6>(p, batch, stream);
    case 7: return launch_one<T, 7>(p, batch, stream);
    case 8: return launch_one<T, 8>(p, batch, stream);
    case 9: return launch_one<T, 9>(p, batch, stream);
    case 10: return launch_one<T, 10>(p, batch, stream);
    case 11: return launch_one<T, 11>(p, batch, stream);
    case 12: return launch_one<T, 12>(p, batch, stream);
  }
  return hipErrorInvalidValue;
}

template hipError_t launch_istft_fused<float>(const IstftPlan&, const cpx<float>*, long long, long long, int, const cpx<float>*,
                                              const double*, const double*, float*, hipStream_t);
template hipError_t launch_istft_fused<double>(const IstftPlan&, const cpx<double>*, long long, long long, int,
                                               const cpx<double>*, const double*, const double*, double*, hipStream_t);

}  // namespace ssq
