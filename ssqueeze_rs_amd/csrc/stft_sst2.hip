// stft_sst2.hip -- second-order ("vertical") synchrosqueezed STFT, `upstream.ssq_stft2` (Oberlin, Meignen
// and Perrier 2015; Behera, Meignen and Oberlin 2018).  Upstream has no such transform: the definition is the project's
// own, restated in numpy by tests/helpers/sst2_ref.py.  Per-sample units, fs enters at the end.  With n = n_fft,
// u[j] = j - n/2 and the five windows g, g1 = g', g2 = g'', tg = u g, tg1 = u g1 (spectral derivatives, host_math.h):
//   V, V1, V2, Vt, Vt1 = the STFTs of x with them (padding, hop and `modulated` rotation of upstream's stft)
//   w1 = k/n - (V1/V)/(2 pi i)      D = Vt V1 - Vt1 V      q = (V2 V - V1^2)/(2 pi i D)      w2 = w1 - q Vt/V
//   reported: fs |Re w2| where |D| > gamma^2 and Re w2 is finite, else fs |Re w1|; a bin is kept where |V| > gamma.
//
//   sst2_operator_kernel : a workgroup of 256 lanes owns a tile of consecutive frames of one signal; a frame is held by
//                          n/16 lanes, 256/(n/16) frames side by side (fft_core.h; frames of 2048 points and more span
//                          several waves).  Per frame: the padded samples once (index map, no padded copy), three
//                          forward transforms x (g + i g1), x tg, x (tg1 + i g2), the packed pairs split into their two
//                          real-input spectra through the frame's exchange row, the operator per bin, and Sx and the
//                          map (w2, bin or -1) out through an LDS transpose, so that global stores run along frames.
//                          Transforms and operator run in fp64 for float32 calls too (sst2_widen_kernel widens the
//                          signals first; Sx and w2 are rounded on store and the bin taken from the rounded w2 in
//                          the call's dtype).
//   sst2_scatter_kernel  : one thread per time column, rows ascending (reassign_cols_kernel's order), no atomics:
//                          the result does not depend on batch size or tiling.
#include <cmath>
#include <vector>

#include "../../include/ssq_hip.h"
#include "dev_buffers.h"
#include "fft_core.h"
#include "host_math.h"
#include "stft_kernels.h"

namespace ssq {

constexpr int kSst2Threads = 256;
constexpr int kSst2RoundsPerTile = 4;      // store tiles one workgroup walks

// O: the dtype of the call (float or double: x in, Sx / map / Tx / w2 out).  The transforms and the operator always run
// in fp64: the operator is a quotient of two differences of products, and with fp32 transforms of 1024 points and more
// over one strong bin in a thousand lands in another bin than the fp64 result.
template <typename O>
struct Sst2Dev {
  const double* x;         // [batch][n_signal], widened by sst2_widen_kernel for a float32 call
  const cpx<double>* tw;   // the passes' twiddle tables [m][k] = exp(-2 pi i k m / (NS R)), passes 1, 2, .. back to back
  const cpx<double>* wa;   // (g, g1 a1)          by frame sample j; a*: powers of two that level the channels
  const double* wb;        // tg at
  const cpx<double>* wc;   // (tg1 at1, g2 a2)
  cpx<O>* Sx;              // [batch][F][n_frames]
  cpx<O>* map;             // [batch][F][n_frames]  (w2 or inf, bin or -1)
  long long n_signal, n_frames;
  int hop, pad_left, padtype, rot, flip, tile_frames;
  double gamma, gamma_sq, fs;
  O dw;                    // Sfs[1] - Sfs[0] in the call's dtype: the bin rule runs on the w2 the call reports
  double h1, it, ht1, h2;  // 0.5 / a1, 1 / at, 0.5 / at1, 0.5 / a2
};

// frames per round = per store tile (and the tile's padded pitch in the LDS stage) of one transform length
template <int LOGN>
struct Sst2Cfg {
  static constexpr int N = 1 << LOGN, L = N / 16, FPR = kSst2Threads / L, ROW = N + N / 16, F = N / 2 + 1;
  static constexpr bool MULTI = L > 64;
  static constexpr int TFS = FPR, SP = TFS >= 8 ? TFS + 1 : TFS;
};

__device__ __forceinline__ int sst2_opaque_zero() {
  int z;
  asm volatile("s_mov_b32 %0, 0" : "=s"(z));
  return z;
}

// The 16 samples of a lane: transform input t + L q is frame sample j (rotated by n/2 when modulated).  A frame inside
// the signal reads them directly.  An edge frame goes through the pad index map in a ROLLED loop, one sample at a time
// through the lane's own slots of the frame's idle exchange row (the lane reads back what it wrote: no ordering point):
// unrolled, the sixteen 64-bit index chains of the five pad types were the kernel's register peak.
template <typename O, int LOGN>
__device__ __forceinline__ void sst2_samples(const Sst2Dev<O>& p, const double* __restrict__ xs, long long pos0, int t,
                                             bool valid, bool interior, double* row, double (&xv)[16]) {
  constexpr int N = 1 << LOGN, L = N / 16;
  if (interior) {
#pragma unroll
    for (int q = 0; q < 16; ++q) xv[q] = xs[pos0 + ((t + L * q + p.rot) & (N - 1))];
  } else {
#pragma unroll 1
    for (int q = 0; q < 16; ++q)
      row[t + L * q] = load_padded_flat(xs, pos0 + ((t + L * q + p.rot) & (N - 1)), p.n_signal, p.padtype, valid);
#pragma unroll
    for (int q = 0; q < 16; ++q) xv[q] = row[t + L * q];
  }
}

// Z = A + i B of two real-input spectra -> A[k] h_a, B[k] h_b (h: half the inverse channel scale) for the lane's bins
// t + L q, q <= 8, from Z[k] and conj Z[n - k] through the frame's exchange row
template <typename T, int LOGN, bool MULTI>
__device__ __forceinline__ void sst2_split(const cpx<T> (&v)[16], cpx<T>* exch, int t, T h_a, T h_b, cpx<T> (&A)[9],
                                           cpx<T> (&B)[9]) {
  constexpr int N = 1 << LOGN, L = N / 16;
#pragma unroll
  for (int q = 0; q < 16; ++q) exch[exch_phys(t + L * q)] = v[q];
  frame_sync<MULTI>();
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const int idx = t + L * q;
    const cpx<T> zp = exch[exch_phys((N - idx) & (N - 1))];
    A[q] = {(v[q].x + zp.x) * h_a, (v[q].y - zp.y) * h_a};
    B[q] = {(v[q].y + zp.y) * h_b, (zp.x - v[q].x) * h_b};
  }
  frame_sync<MULTI>();
}

// the operator of one bin in fp64 -> (fs |Re w|, or inf where the bin is not kept; unused)
template <typename O>
__device__ __forceinline__ cpx<double> sst2_operator(const Sst2Dev<O>& p, double eta, cpx<double> V, cpx<double> V1,
                                                     cpx<double> V2, cpx<double> Vt, cpx<double> Vt1) {
  using T = double;
  const T two_pi = (T)6.283185307179586;
  const T den = V.x * V.x + V.y * V.y;
  const T re1 = eta - (V1.y * V.x - V1.x * V.y) / (den * two_pi);          // Re w1 (upstream's first-order expression)
  const cpx<T> D = cmul(Vt, V1) - cmul(Vt1, V);
  const cpx<T> num = cmul(V2, V) - cmul(V1, V1);
  const T inv_den = (T)1 / den;                                              // the two quotients, formed once
  const cpx<T> r = {(Vt.x * V.x + Vt.y * V.y) * inv_den, (Vt.y * V.x - Vt.x * V.y) * inv_den};      // Vt / V
  const cpx<T> nr = cmul(num, r);
  const T dd = D.x * D.x + D.y * D.y;
  const T re2 = re1 - ((nr.y * D.x - nr.x * D.y) / dd) / two_pi;           // Re(q Vt/V) = Im(num r / D) / (2 pi)
  const bool second = hypot(D.x, D.y) > p.gamma_sq && isfinite(re2);
  const T w = p.fs * fabs(second ? re2 : re1);
  const bool keep = hypot(V.x, V.y) > p.gamma;
  return {keep ? w : (T)INFINITY, (T)0};
}

// the upstream bin rule (phase_bin_upstream's) on the frequency the call reports, in the call's dtype -> (w2, bin or -1)
template <typename O>
__device__ __forceinline__ cpx<O> sst2_bin(const Sst2Dev<O>& p, int last, double w_or_inf) {
  const O w = (O)w_or_inf;
  if (w_or_inf == (double)INFINITY) return {w, (O)-1};
  const O v = fmax(w / p.dw, (O)0);                                         // (w - Sfs[0]) / dw, Sfs[0] = 0
  int kk = (v >= (O)last) ? last : (int)rint(v);
  if (!(v == v)) kk = 0;
  if (p.flip) kk = last - kk;
  return {w, (O)kk};
}

template <typename O, int LOGN>
__global__ __launch_bounds__(kSst2Threads) void sst2_operator_kernel(const Sst2Dev<O> p) {
  using T = double;
  using C = Sst2Cfg<LOGN>;
  constexpr int N = C::N, L = C::L, FPR = C::FPR, ROW = C::ROW, F = C::F, TFS = C::TFS, SP = C::SP;
  constexpr bool MULTI = C::MULTI;
  __shared__ __attribute__((aligned(16))) cpx<T> exch_all[FPR * ROW];
  __shared__ __attribute__((aligned(16))) cpx<T> st_s[F * SP];
  __shared__ __attribute__((aligned(16))) cpx<T> st_m[F * SP];

  const int tid = threadIdx.x;
  int g = tid / L;                                         // frame slot of the round
  const int t = tid % L;                                   // lane inside the frame
  if constexpr (L >= 64) g = __builtin_amdgcn_readfirstlane(g);        // one frame (or part of one) per wave: scalar
  cpx<T>* exch = exch_all + g * ROW;

  const long long nfr = p.n_frames;
  const long long b = blockIdx.y;
  const T* __restrict__ xs = p.x + b * p.n_signal;
  cpx<O>* __restrict__ Sx = p.Sx + b * (long long)F * nfr;
  cpx<O>* __restrict__ map = p.map + b * (long long)F * nfr;
  const long long f_tile = (long long)blockIdx.x * p.tile_frames;
  const long long f_end = f_tile + p.tile_frames < nfr ? f_tile + p.tile_frames : nfr;
  const T inv_n = (T)(1.0 / (double)N);

  for (long long fr0 = f_tile; fr0 < f_end; fr0 += TFS) {               // a round = a store tile: FPR frames side by side
    {
      const long long f = fr0 + g;
      const bool valid = f < f_end;                                      // (a frame past the end transforms zeros)
      const long long pos0 = f * p.hop - p.pad_left;
      const bool interior = valid && pos0 >= 0 && pos0 + N <= p.n_signal;
      T xv[16];
      sst2_samples<O, LOGN>(p, xs, pos0, t + sst2_opaque_zero(), valid, interior, reinterpret_cast<T*>(exch), xv);
      frame_sync<MULTI>();      // (an edge frame's samples went through the row: all read before the first exchange writes it)
      // The three transforms: (g, g1) first, its V straight into the store tile and V1 parked in the lane's own map
      // slots (the lane reads back what it wrote: no ordering point); tg alone (real input, no split); (tg1, g2) last.
      // So the last transform runs beside ONE held spectrum, not four (what keeps the kernel inside 256 registers).
      // The tables are loop invariant: an opaque zero offset per transform keeps their loads (and the twiddles') where
      // they are used instead of in ~100 registers across the loop; added to the lane index it does the same for the
      // LDS and table addresses built on it (another ~90 registers when hoisted).  The scheduling barriers keep a later
      // transform's loads from being moved above an earlier one.
      const int slot = g;
      cpx<T> v[16];
      cpx<T> Vt[9], Vt1[9], V2[9];
      {
        cpx<T> V[9], V1[9];
        const int z = sst2_opaque_zero(), tz = t + z;
        const cpx<T>* __restrict__ wa = p.wa + z;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const cpx<T> w = wa[(tz + L * q + p.rot) & (N - 1)];
          v[q] = {xv[q] * w.x, xv[q] * w.y};
        }
        fft_pass_compact<T, LOGN, 0, MULTI>(v, exch, p.tw + z, tz);
        sst2_split<T, LOGN, MULTI>(v, exch, tz, (T)0.5, p.h1, V, V1);
#pragma unroll
        for (int q = 0; q < 9; ++q) {
          const int k = tz + L * q;
          if (k <= N / 2) {
            st_s[k * SP + slot] = V[q];
            st_m[k * SP + slot] = V1[q];
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      {
        const int z = sst2_opaque_zero(), tz = t + z;
        const T* __restrict__ wb = p.wb + z;                             // real input: its spectrum is the transform itself
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = {xv[q] * wb[(tz + L * q + p.rot) & (N - 1)], (T)0};
        fft_pass_compact<T, LOGN, 0, MULTI>(v, exch, p.tw + z, tz);
#pragma unroll
        for (int q = 0; q < 9; ++q) Vt[q] = cscale(v[q], p.it);
      }
      __builtin_amdgcn_sched_barrier(0);
      {
        const int z = sst2_opaque_zero(), tz = t + z;
        const cpx<T>* __restrict__ wc = p.wc + z;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const cpx<T> w = wc[(tz + L * q + p.rot) & (N - 1)];
          v[q] = {xv[q] * w.x, xv[q] * w.y};
        }
        fft_pass_compact<T, LOGN, 0, MULTI>(v, exch, p.tw + z, tz);
        sst2_split<T, LOGN, MULTI>(v, exch, tz, p.ht1, p.h2, Vt1, V2);
      }
      __builtin_amdgcn_sched_barrier(0);
      // ---- the operator per bin k <= n/2, into the store tile [bin][frame]
      const int te = t + sst2_opaque_zero();
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        const int k = te + L * q;
        if (k <= N / 2) {
          const cpx<T> V = st_s[k * SP + slot], V1 = st_m[k * SP + slot];
          st_m[k * SP + slot] = sst2_operator<O>(p, (T)k * inv_n, V, V1, V2[q], Vt[q], Vt1[q]);
        }
      }
    }
    __syncthreads();
    const int nft = (int)(f_end - fr0 < TFS ? f_end - fr0 : TFS);
    for (int e = tid; e < F * TFS; e += kSst2Threads) {                  // neighbouring lanes: neighbouring frames of a bin
      const int k = e / TFS, fl = e % TFS;
      if (fl < nft) {
        const long long o = (long long)k * nfr + fr0 + fl;
        const cpx<T> S = st_s[k * SP + fl];
        Sx[o] = {(O)S.x, (O)S.y};
        map[o] = sst2_bin<O>(p, F - 1, st_m[k * SP + fl].x);
      }
    }
    __syncthreads();
  }
}

__global__ void sst2_widen_kernel(const float* __restrict__ in, double* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (double)in[i];
}

template <typename T>
__global__ void sst2_scatter_kernel(const cpx<T>* __restrict__ Sx, const cpx<T>* __restrict__ map, cpx<T>* __restrict__ Tx,
                                    T* __restrict__ w_out, int n_freqs, long long n_frames, int squeezing, T dw, T leb_val) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_frames) return;
  const long long base = (long long)blockIdx.y * n_freqs * n_frames + j;
  for (int i = 0; i < n_freqs; ++i) {
    const long long o = base + (long long)i * n_frames;
    const cpx<T> m = map[o];
    if (w_out) w_out[o] = m.x;
    if (m.y >= (T)0) {
      const long long d = base + (long long)(int)m.y * n_frames;
      cpx<T> acc = Tx[d];
      if (squeezing == 1) {
        acc.x += leb_val;
      } else {
        const cpx<T> S = Sx[o];
        acc.x += S.x * dw;
        acc.y += S.y * dw;
      }
      Tx[d] = acc;
    }
  }
}

template <typename T, int LOGN>
static hipError_t sst2_launch_one(Sst2Dev<T> p, long long batch, hipStream_t stream) {
  p.tile_frames = Sst2Cfg<LOGN>::TFS * kSst2RoundsPerTile;
  const long long tiles = (p.n_frames + p.tile_frames - 1) / p.tile_frames;
  if (tiles > 0x7fffffffLL || batch > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL((sst2_operator_kernel<T, LOGN>), dim3((unsigned)tiles, (unsigned)batch), dim3(kSst2Threads), 0, stream, p);
  return hipGetLastError();
}

template <typename T>
static hipError_t sst2_launch(const Sst2Dev<T>& p, int logn, long long batch, hipStream_t stream) {
  switch (logn) {
    case 4: return sst2_launch_one<T, 4>(p, batch, stream);
    case 5: return sst2_launch_one<T, 5>(p, batch, stream);
    case 6: return sst2_launch_one<T, 6>(p, batch, stream);
    case 7: return sst2_launch_one<T, 7>(p, batch, stream);
    case 8: return sst2_launch_one<T, 8>(p, batch, stream);
    case 9: return sst2_launch_one<T, 9>(p, batch, stream);
    case 10: return sst2_launch_one<T, 10>(p, batch, stream);
    case 11: return sst2_launch_one<T, 11>(p, batch, stream);
    case 12: return sst2_launch_one<T, 12>(p, batch, stream);
  }
  return hipErrorInvalidValue;
}

}  // namespace ssq

using namespace ssq;

namespace {

// a power of two a with a * max|tab| within a factor two of `level` (exact to apply and to undo)
double level_scale(const std::vector<double>& tab, double level) {
  double m = 0;
  for (double v : tab) m = std::fmax(m, std::fabs(v));
  if (!(m > 0) || !(level > 0) || !std::isfinite(level / m)) return 1.0;
  int e = 0;
  std::frexp(level / m, &e);
  return std::ldexp(1.0, e - 1);
}

struct Sst2Shape {
  int logn = 0;
  int64_t n_freqs = 0, n_frames = 0;
  double fs = 1.0, gamma = 0.0, dw = 0.0;
  std::vector<double> sfs;
};

// The argument checks of the three entry points, and the shape they work on (sets the error and returns non-zero)
int sst2_shape(int dtype, int64_t batch, int64_t n_signal, int64_t n_fft, int64_t hop, double fs, int padtype, int squeezing,
               double gamma, Sst2Shape* s) {
  if (dtype != SSQ_F32 && dtype != SSQ_F64) SSQ_FAIL("dtype must be SSQ_F32 or SSQ_F64");
  if (batch < 1) SSQ_FAIL("batch must be >= 1");
  if (n_fft < 16 || n_fft > 4096 || (n_fft & (n_fft - 1)) != 0)
    SSQ_FAIL("ssq_stft2: n_fft must be a power of two from 16 to 4096");
  if (n_signal < 1 || hop < 1) SSQ_FAIL("ssq_stft2: n_signal and hop must be >= 1");
  if (padtype < SSQ_PAD_REFLECT || padtype > 4) SSQ_FAIL("ssq_stft2: unknown padtype");
  if (squeezing != SSQ_SQUEEZE_SUM && squeezing != SSQ_SQUEEZE_LEBESGUE) SSQ_FAIL("ssq_stft2: squeezing must be 'sum' or 'lebesgue'");
  if (!(fs > 0) || !std::isfinite(fs)) SSQ_FAIL("ssq_stft2: fs must be positive");
  if (padtype == 4 && n_signal < 1) SSQ_FAIL("ssq_stft2: empty signal");
  s->logn = 0;
  while ((1LL << s->logn) < n_fft) ++s->logn;
  s->n_freqs = n_fft / 2 + 1;
  s->n_frames = (n_signal - 1) / hop + 1;
  if (s->n_frames > (1LL << 30)) SSQ_FAIL("ssq_stft2: too many frames");
  s->fs = fs;
  s->gamma = gamma < 0 ? 10.0 * (dtype == SSQ_F64 ? 2.2204460492503131e-16 : 1.1920928955078125e-07) : gamma;
  s->sfs = host::np_linspace(0.0, 0.5 * fs, s->n_freqs);
  s->dw = s->sfs[1] - s->sfs[0];
  return 0;
}

// g1 = g', g2 = g'' (spectral derivatives, Nyquist term zeroed), tg = u g, tg1 = u g1 with u = j - n/2, in fp64
void sst2_window_tables(const double* window, int64_t n, std::vector<double>& g1, std::vector<double>& g2,
                        std::vector<double>& tg, std::vector<double>& tg1) {
  g1 = host::diff_window(window, n, true);
  g2 = host::diff_window(g1.data(), n, true);
  tg.resize((size_t)n);
  tg1.resize((size_t)n);
  for (int64_t j = 0; j < n; ++j) {
    const double u = (double)(j - n / 2);
    tg[j] = u * window[j];
    tg1[j] = u * g1[j];
  }
}

// the call's tables on the device (held by `d`) and the parameter block without its signal / output pointers
template <typename T>
int sst2_tables(HostCallBufs& d, const Sst2Shape& s, const double* window, int64_t n, int64_t n_signal, int64_t hop,
                int padtype, int variant, Sst2Dev<T>* p) {
  const std::vector<double> g(window, window + n);
  std::vector<double> g1, g2, tg, tg1;
  sst2_window_tables(window, n, g1, g2, tg, tg1);
  double mg = 0;
  for (double v : g) mg = std::fmax(mg, std::fabs(v));
  const double a1 = level_scale(g1, mg), a2 = level_scale(g2, mg), at = level_scale(tg, mg), at1 = level_scale(tg1, mg);
  std::vector<cpx<double>> wa((size_t)n), wc((size_t)n), tw;      // fp64 for either dtype of the call (Sst2Dev)
  std::vector<double> wb((size_t)n);
  for (int64_t j = 0; j < n; ++j) {
    wa[j] = {g[j], g1[j] * a1};
    wb[j] = tg[j] * at;
    wc[j] = {tg1[j] * at1, g2[j] * a2};
  }
  for (int P = 1; P < num_passes(s.logn); ++P) {             // read coalesced by fft_pass_compact
    const int R = pass_radix(s.logn, P), NS = pass_ns(s.logn, P);
    for (int m = 0; m < R; ++m)
      for (int k = 0; k < NS; ++k) {
        const long double ang = 2.0L * 3.14159265358979323846264338327950288L * (long double)((long long)k * m) /
                                (long double)((long long)NS * R);
        tw.push_back({(double)cosl(ang), (double)(-sinl(ang))});
      }
  }
  void *d_tw, *d_wa, *d_wb, *d_wc;
  SSQ_HIP(d.upload(&d_tw, tw.data(), sizeof(cpx<double>) * tw.size()));
  SSQ_HIP(d.upload(&d_wa, wa.data(), sizeof(cpx<double>) * n));
  SSQ_HIP(d.upload(&d_wb, wb.data(), sizeof(double) * n));
  SSQ_HIP(d.upload(&d_wc, wc.data(), sizeof(cpx<double>) * n));
  *p = Sst2Dev<T>{};
  p->tw = (const cpx<double>*)d_tw;
  p->wa = (const cpx<double>*)d_wa;
  p->wb = (const double*)d_wb;
  p->wc = (const cpx<double>*)d_wc;
  p->n_signal = n_signal;
  p->n_frames = s.n_frames;
  p->hop = (int)hop;
  p->pad_left = (int)(n / 2);                                // the larger half of the n - 1 pad samples on the left
  p->padtype = padtype;
  p->rot = (variant & SSQ_VARIANT_MODULATED) ? (int)(n / 2) : 0;
  p->flip = (variant & SSQ_VARIANT_FLIPUD) ? 1 : 0;
  p->gamma = s.gamma;
  p->gamma_sq = s.gamma * s.gamma;
  p->dw = (T)s.dw;
  p->fs = s.fs;
  p->h1 = 0.5 / a1;
  p->it = 1.0 / at;
  p->ht1 = 0.5 / at1;
  p->h2 = 0.5 / a2;
  return 0;
}

// both kernels of `nb` signals on device buffers (Tx is zeroed here)
template <typename T>
hipError_t sst2_run(Sst2Dev<T> p, const Sst2Shape& s, int squeezing, const T* d_x, int64_t nb, cpx<T>* d_Tx, cpx<T>* d_Sx,
                    T* d_w, cpx<T>* d_map, double* d_xd /* float32 calls: [nb][n_signal] */) {
  const size_t map_sig = (size_t)s.n_freqs * (size_t)s.n_frames;
  hipError_t e = hipMemsetAsync(d_Tx, 0, sizeof(cpx<T>) * map_sig * (size_t)nb, nullptr);
  if (e != hipSuccess) return e;
  const double* xd;
  if constexpr (sizeof(T) == 4) {
    const long long n = (long long)nb * p.n_signal;
    hipLaunchKernelGGL(sst2_widen_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, (const float*)d_x, d_xd, n);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    xd = d_xd;
  } else {
    xd = (const double*)d_x;
  }
  for (int64_t b0 = 0; b0 < nb; b0 += 65535) {
    const int64_t n1 = nb - b0 < 65535 ? nb - b0 : 65535;
    p.x = xd + b0 * p.n_signal;
    p.Sx = d_Sx + map_sig * b0;
    p.map = d_map + map_sig * b0;
    e = sst2_launch<T>(p, s.logn, n1, nullptr);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sst2_scatter_kernel<T>, dim3((unsigned)((s.n_frames + 255) / 256), (unsigned)n1), dim3(256), 0, nullptr,
                       (const cpx<T>*)p.Sx, (const cpx<T>*)p.map, d_Tx + map_sig * b0, d_w ? d_w + map_sig * b0 : (T*)nullptr,
                       (int)s.n_freqs, (long long)s.n_frames, squeezing, p.dw, (T)((T)s.dw / (T)s.n_freqs));
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <typename T>
int sst2_host_typed(const Sst2Shape& s, const void* x, int64_t batch, int64_t n_signal, const double* window, int64_t n,
                    int64_t hop, int padtype, int squeezing, int variant, void* Tx, void* Sx, void* w2) {
  HostCallBufs d;
  Sst2Dev<T> p;
  if (int rc = sst2_tables<T>(d, s, window, n, n_signal, hop, padtype, variant, &p)) return rc;
  const size_t map_sig = (size_t)s.n_freqs * (size_t)s.n_frames;
  // signals per slice: most of the free memory (a signal's result does not depend on the slice it is in)
  const double per = (double)(sizeof(T) == 4 ? 12 : 8) * (double)n_signal + (double)map_sig * (3.0 * sizeof(cpx<T>) + (w2 ? sizeof(T) : 0));
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)1 << 30;
  int64_t slice = (int64_t)(0.8 * (double)free_b / per);
  if (slice > batch) slice = batch;
  if (slice < 1) slice = 1;                                  // one signal is always tried: hipMalloc reports the rest
  void *d_x, *d_Tx, *d_Sx, *d_map, *d_w = nullptr, *d_xd = nullptr;
  SSQ_HIP(d.alloc(&d_x, sizeof(T) * (size_t)n_signal * slice));
  if (sizeof(T) == 4) SSQ_HIP(d.alloc(&d_xd, sizeof(double) * (size_t)n_signal * slice));
  SSQ_HIP(d.alloc(&d_Tx, sizeof(cpx<T>) * map_sig * slice));
  SSQ_HIP(d.alloc(&d_Sx, sizeof(cpx<T>) * map_sig * slice));
  SSQ_HIP(d.alloc(&d_map, sizeof(cpx<T>) * map_sig * slice));
  if (w2) SSQ_HIP(d.alloc(&d_w, sizeof(T) * map_sig * slice));
  for (int64_t b0 = 0; b0 < batch; b0 += slice) {
    const int64_t nb = batch - b0 < slice ? batch - b0 : slice;
    SSQ_HIP(hipMemcpy(d_x, (const T*)x + (size_t)n_signal * b0, sizeof(T) * (size_t)n_signal * nb, hipMemcpyHostToDevice));
    SSQ_HIP(sst2_run<T>(p, s, squeezing, (const T*)d_x, nb, (cpx<T>*)d_Tx, (cpx<T>*)d_Sx, (T*)d_w, (cpx<T>*)d_map, (double*)d_xd));
    SSQ_HIP(hipMemcpy((cpx<T>*)Tx + map_sig * b0, d_Tx, sizeof(cpx<T>) * map_sig * nb, hipMemcpyDeviceToHost));
    SSQ_HIP(hipMemcpy((cpx<T>*)Sx + map_sig * b0, d_Sx, sizeof(cpx<T>) * map_sig * nb, hipMemcpyDeviceToHost));
    if (w2) SSQ_HIP(hipMemcpy((T*)w2 + map_sig * b0, d_w, sizeof(T) * map_sig * nb, hipMemcpyDeviceToHost));
  }
  return 0;
}

struct Sst2Events {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  ~Sst2Events() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
};

template <typename T>
int sst2_exec_typed(const Sst2Shape& s, const void* d_x, int64_t batch, int64_t n_signal, const double* window, int64_t n,
                    int64_t hop, int padtype, int squeezing, int variant, void* d_Tx, void* d_Sx, void* d_w2, void* d_work,
                    float* kernel_ms) {
  HostCallBufs d;
  Sst2Events t;
  Sst2Dev<T> p;
  if (int rc = sst2_tables<T>(d, s, window, n, n_signal, hop, padtype, variant, &p)) return rc;
  if (kernel_ms) {
    SSQ_HIP(hipEventCreate(&t.ev0));
    SSQ_HIP(hipEventCreate(&t.ev1));
    SSQ_HIP(hipEventRecord(t.ev0, nullptr));
  }
  // the workspace: the map, then (float32 calls) the widened signals
  double* d_xd = (double*)((char*)d_work + sizeof(cpx<T>) * (size_t)batch * (size_t)s.n_freqs * (size_t)s.n_frames);
  SSQ_HIP(sst2_run<T>(p, s, squeezing, (const T*)d_x, batch, (cpx<T>*)d_Tx, (cpx<T>*)d_Sx, (T*)d_w2, (cpx<T>*)d_work, d_xd));
  if (kernel_ms) {
    SSQ_HIP(hipEventRecord(t.ev1, nullptr));
    SSQ_HIP(hipEventSynchronize(t.ev1));
    SSQ_HIP(hipEventElapsedTime(kernel_ms, t.ev0, t.ev1));
  } else {
    SSQ_HIP(hipDeviceSynchronize());
  }
  return 0;
}

}  // namespace

extern "C" {

int ssq_ssq_stft2_host(int dtype, const void* x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                       int64_t hop, double fs, int padtype, int squeezing, double gamma, int variant, void* Tx,
                       double* ssq_freqs, void* Sx, void* w2) {
  if (!x || !window || !Tx || !Sx) SSQ_FAIL("NULL argument");
  Sst2Shape s;
  if (int rc = sst2_shape(dtype, batch, n_signal, n_fft, hop, fs, padtype, squeezing, gamma, &s)) return rc;
  if (ssq_freqs)
    for (int64_t i = 0; i < s.n_freqs; ++i) ssq_freqs[i] = (variant & SSQ_VARIANT_FLIPUD) ? s.sfs[s.n_freqs - 1 - i] : s.sfs[i];
  if (int rc = require_device()) return rc;
  return dtype == SSQ_F32
             ? sst2_host_typed<float>(s, x, batch, n_signal, window, n_fft, hop, padtype, squeezing, variant, Tx, Sx, w2)
             : sst2_host_typed<double>(s, x, batch, n_signal, window, n_fft, hop, padtype, squeezing, variant, Tx, Sx, w2);
}

int ssq_ssq_stft2_window_tables(const double* window, int64_t n_fft, double* g1, double* g2, double* tg, double* tg1) {
  if (!window || !g1 || !g2 || !tg || !tg1) SSQ_FAIL("NULL argument");
  if (n_fft < 16 || n_fft > 4096 || (n_fft & (n_fft - 1)) != 0)
    SSQ_FAIL("ssq_stft2: n_fft must be a power of two from 16 to 4096");
  std::vector<double> a, b, c, d;
  sst2_window_tables(window, n_fft, a, b, c, d);
  for (int64_t j = 0; j < n_fft; ++j) {
    g1[j] = a[j];
    g2[j] = b[j];
    tg[j] = c[j];
    tg1[j] = d[j];
  }
  return 0;
}

int64_t ssq_ssq_stft2_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t n_fft, int64_t hop) {
  Sst2Shape s;
  if (sst2_shape(dtype, batch, n_signal, n_fft, hop, 1.0, SSQ_PAD_REFLECT, SSQ_SQUEEZE_SUM, -1.0, &s)) return -1;
  return (int64_t)(dtype == SSQ_F32 ? 8 : 16) * batch * s.n_freqs * s.n_frames + (dtype == SSQ_F32 ? 8 * batch * n_signal : 0);
}

int ssq_ssq_stft2_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                       int64_t hop, double fs, int padtype, int squeezing, double gamma, int variant, void* d_Tx, void* d_Sx,
                       void* d_w2, void* d_workspace, int64_t workspace_bytes, float* kernel_ms) {
  if (!d_x || !window || !d_Tx || !d_Sx || !d_workspace) SSQ_FAIL("NULL argument");
  Sst2Shape s;
  if (int rc = sst2_shape(dtype, batch, n_signal, n_fft, hop, fs, padtype, squeezing, gamma, &s)) return rc;
  if (workspace_bytes < ssq_ssq_stft2_workspace_bytes(dtype, batch, n_signal, n_fft, hop))
    SSQ_FAIL("ssq_stft2: workspace smaller than ssq_ssq_stft2_workspace_bytes");
  if (int rc = require_device()) return rc;
  return dtype == SSQ_F32 ? sst2_exec_typed<float>(s, d_x, batch, n_signal, window, n_fft, hop, padtype, squeezing, variant, d_Tx,
                                                   d_Sx, d_w2, d_workspace, kernel_ms)
                          : sst2_exec_typed<double>(s, d_x, batch, n_signal, window, n_fft, hop, padtype, squeezing, variant,
                                                    d_Tx, d_Sx, d_w2, d_workspace, kernel_ms);
}

}  // extern "C"
