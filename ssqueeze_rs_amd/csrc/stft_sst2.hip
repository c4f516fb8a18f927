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
//                          Transforms and operator run in fp64 for float32 calls too (widen_f64 widens the
//                          signals first; Sx and w2 are rounded on store and the bin taken from the rounded w2 in
//                          the call's dtype).
//   sst2_scatter_kernel  : one thread per time column, rows ascending (reassign_cols_kernel's order), no atomics:
//                          the result does not depend on batch size or tiling.
// The frame ownership, the loader, the split and the tables are stft_frames64.h's and sst_tables.h's, shared with
// stft_tsst.hip and stft_reassign.hip.  stft_msst.hip (mssq_stft) runs both kernels of this file through stft_sst2.h, with
// its walk between them; its order 1 is gamma_sq = +inf (|D| > gamma_sq nowhere: every bin reports fs |Re w1|).
#include <cmath>
#include <vector>

#include "../../include/ssq_hip.h"
#include "dev_buffers.h"
#include "sst_tables.h"
#include "stft_frames64.h"
#include "stft_sst2.h"

namespace ssq {

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
__global__ __launch_bounds__(kFrameThreads) void sst2_operator_kernel(const Sst2Dev<O> p) {
  using T = double;
  using C = FrameCfg<LOGN>;
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
      frame_samples<LOGN>(p, xs, pos0, t + opaque_zero(), valid, interior, reinterpret_cast<T*>(exch), xv);
      frame_sync<MULTI>();      // (an edge frame's samples went through the row: all read before the first exchange writes it)
      // The three transforms: (g, g1) first, its V straight into the store tile and V1 parked in the lane's own map
      // slots (the lane reads back what it wrote: no ordering point); tg alone (real input, no split); (tg1, g2) last.
      // So the last transform runs beside ONE held spectrum, not four (what keeps the kernel inside 256 registers).
      // An opaque zero offset per transform (stft_frames64.h) keeps the loop-invariant table loads where they are used;
      // the scheduling barriers keep a later transform's loads from being moved above an earlier one.
      const int slot = g;
      cpx<T> v[16];
      cpx<T> Vt[9], Vt1[9], V2[9];
      {
        cpx<T> V[9], V1[9];
        const int z = opaque_zero(), tz = t + z;
        const cpx<T>* __restrict__ wa = p.wa + z;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const cpx<T> w = wa[(tz + L * q + p.rot) & (N - 1)];
          v[q] = {xv[q] * w.x, xv[q] * w.y};
        }
        fft_pass_compact<T, LOGN, 0, MULTI>(v, exch, p.tw + z, tz);
        frame_split<T, LOGN, MULTI>(v, exch, tz, (T)0.5, p.h1, V, V1);
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
        const int z = opaque_zero(), tz = t + z;
        const T* __restrict__ wb = p.wb + z;                             // real input: its spectrum is the transform itself
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = {xv[q] * wb[(tz + L * q + p.rot) & (N - 1)], (T)0};
        fft_pass_compact<T, LOGN, 0, MULTI>(v, exch, p.tw + z, tz);
#pragma unroll
        for (int q = 0; q < 9; ++q) Vt[q] = cscale(v[q], p.it);
      }
      __builtin_amdgcn_sched_barrier(0);
      {
        const int z = opaque_zero(), tz = t + z;
        const cpx<T>* __restrict__ wc = p.wc + z;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const cpx<T> w = wc[(tz + L * q + p.rot) & (N - 1)];
          v[q] = {xv[q] * w.x, xv[q] * w.y};
        }
        fft_pass_compact<T, LOGN, 0, MULTI>(v, exch, p.tw + z, tz);
        frame_split<T, LOGN, MULTI>(v, exch, tz, p.ht1, p.h2, Vt1, V2);
      }
      __builtin_amdgcn_sched_barrier(0);
      // ---- the operator per bin k <= n/2, into the store tile [bin][frame]
      const int te = t + opaque_zero();
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
    for (int e = tid; e < F * TFS; e += kFrameThreads) {                  // neighbouring lanes: neighbouring frames of a bin
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

template <typename T>
static hipError_t sst2_launch(Sst2Dev<T> p, int logn, long long batch, hipStream_t stream) {
  return dispatch_logn(logn, [&](auto ln) {
    constexpr int LOGN = decltype(ln)::value;
    dim3 grid;
    if (hipError_t e = frame_grid<LOGN>(p.n_frames, batch, &p.tile_frames, &grid); e != hipSuccess) return e;
    hipLaunchKernelGGL((sst2_operator_kernel<T, LOGN>), grid, dim3(kFrameThreads), 0, stream, p);
    return hipGetLastError();
  });
}

// The argument checks of the entry points, and the shape they work on (sets the error and returns non-zero)
int sst2_shape(const char* name, const char* own_fail, const FrameCall& c, Sst2Shape* s) {
  const bool sq_ok = c.squeezing == SSQ_SQUEEZE_SUM || c.squeezing == SSQ_SQUEEZE_LEBESGUE;
  if (!own_fail && !sq_ok) own_fail = "squeezing must be 'sum' or 'lebesgue'";
  if (int rc = frame_shape(name, false, own_fail, c, s)) return rc;
  s->sfs = host::np_linspace(0.0, 0.5 * c.fs, s->n_freqs);
  s->dw = s->sfs[1] - s->sfs[0];
  return 0;
}

// the call's tables on the device (held by `d`) and the parameter block without its signal / output pointers
template <typename T>
int sst2_tables(DeviceBufs& d, const Sst2Shape& s, const FrameCall& c, Sst2Dev<T>* p) {
  const int64_t n = c.n_fft;
  const host::SstTables t = host::sst_level_tables(c.window, n, host::kSstSecond);   // fp64 for either dtype of the call
  const std::vector<double> tw = host::pass_twiddles(s.logn);
  void *d_tw, *d_wa, *d_wb, *d_wc;
  SSQ_HIP(d.upload(&d_tw, tw.data(), sizeof(double) * tw.size()));
  SSQ_HIP(d.upload(&d_wa, t.wa.data(), sizeof(cpx<double>) * n));
  SSQ_HIP(d.upload(&d_wb, t.wb.data(), sizeof(double) * n));
  SSQ_HIP(d.upload(&d_wc, t.wc.data(), sizeof(cpx<double>) * n));
  *p = Sst2Dev<T>{};
  p->tw = (const cpx<double>*)d_tw;
  p->wa = (const cpx<double>*)d_wa;
  p->wb = (const double*)d_wb;
  p->wc = (const cpx<double>*)d_wc;
  p->n_signal = c.n_signal;
  p->n_frames = s.n_frames;
  p->hop = (int)c.hop;
  p->pad_left = (int)(n / 2);                                // the larger half of the n - 1 pad samples on the left
  p->padtype = c.padtype;
  p->rot = (c.variant & SSQ_VARIANT_MODULATED) ? (int)(n / 2) : 0;
  p->flip = (c.variant & SSQ_VARIANT_FLIPUD) ? 1 : 0;
  p->gamma = s.gamma;
  p->gamma_sq = s.gamma * s.gamma;
  p->dw = (T)s.dw;
  p->fs = s.fs;
  p->h1 = t.h1;
  p->it = t.it;
  p->ht1 = t.ht1;
  p->h2 = t.h2;
  return 0;
}

// the operator kernel of `nb` signals on device buffers
template <typename T>
hipError_t sst2_operator_run(Sst2Dev<T> p, const Sst2Shape& s, const T* d_x, int64_t nb, cpx<T>* d_Sx, cpx<T>* d_map,
                             double* d_xd /* float32 calls: [nb][n_signal] */) {
  const size_t map_sig = (size_t)s.n_freqs * (size_t)s.n_frames;
  const double* xd;
  if (hipError_t e = frame_signals64(d_x, d_xd, (long long)nb * p.n_signal, nullptr, &xd); e != hipSuccess) return e;
  return for_signal_runs(nb, [&](int64_t b0, int64_t n1) {
    p.x = xd + b0 * p.n_signal;
    p.Sx = d_Sx + map_sig * b0;
    p.map = d_map + map_sig * b0;
    return sst2_launch<T>(p, s.logn, n1, nullptr);
  });
}

// Tx zeroed, then the scatter of `nb` signals on device buffers
template <typename T>
hipError_t sst2_scatter_run(const Sst2Shape& s, int squeezing, T dw, int64_t nb, const cpx<T>* d_Sx, const cpx<T>* d_map,
                            cpx<T>* d_Tx, T* d_w) {
  const size_t map_sig = (size_t)s.n_freqs * (size_t)s.n_frames;
  if (hipError_t e = hipMemsetAsync(d_Tx, 0, sizeof(cpx<T>) * map_sig * (size_t)nb, nullptr); e != hipSuccess) return e;
  return for_signal_runs(nb, [&](int64_t b0, int64_t n1) {
    hipLaunchKernelGGL(sst2_scatter_kernel<T>, dim3((unsigned)((s.n_frames + 255) / 256), (unsigned)n1), dim3(256), 0, nullptr,
                       d_Sx + map_sig * b0, d_map + map_sig * b0, d_Tx + map_sig * b0, d_w ? d_w + map_sig * b0 : (T*)nullptr,
                       (int)s.n_freqs, (long long)s.n_frames, squeezing, dw, (T)((T)s.dw / (T)s.n_freqs));
    return hipGetLastError();
  });
}

#define SSQ_SST2_INSTANTIATE(T)                                                                                          \
  template int sst2_tables<T>(DeviceBufs&, const Sst2Shape&, const FrameCall&, Sst2Dev<T>*);                            \
  template hipError_t sst2_operator_run<T>(Sst2Dev<T>, const Sst2Shape&, const T*, int64_t, cpx<T>*, cpx<T>*, double*);   \
  template hipError_t sst2_scatter_run<T>(const Sst2Shape&, int, T, int64_t, const cpx<T>*, const cpx<T>*, cpx<T>*, T*);
SSQ_SST2_INSTANTIATE(float)
SSQ_SST2_INSTANTIATE(double)
#undef SSQ_SST2_INSTANTIATE

}  // namespace ssq

using namespace ssq;

namespace {

// ssq_stft2 on device buffers (pipe_host, pipe_exec): the operator, then the scatter (Tx is zeroed there)
template <typename T>
struct Sst2Pipe {
  static constexpr int kMid = 0;
  const FrameCall& c;
  const Sst2Shape& s;
  DeviceBufs d;
  Sst2Dev<T> p;
  cpx<T>*Tx, *Sx, *map;
  T* w;
  double* xd;
  int tables() { return sst2_tables<T>(d, s, c, &p); }
  int bind(int64_t cap, void* const* outs /* Tx, Sx, w2 */, void* work) {
    const Sst2Work k = sst2_work(c.dtype, cap, c.n_signal, s);
    Tx = (cpx<T>*)outs[0];
    Sx = (cpx<T>*)outs[1];
    w = (T*)outs[2];
    map = (cpx<T>*)((char*)work + k.map);
    xd = (double*)((char*)work + k.xd);
    return 0;
  }
  int run(int64_t nb, const void* d_x, const hipEvent_t*) {
    SSQ_HIP(sst2_operator_run<T>(p, s, (const T*)d_x, nb, Sx, map, xd));
    SSQ_HIP(sst2_scatter_run<T>(s, c.squeezing, p.dw, nb, Sx, map, Tx, w));
    return 0;
  }
};

}  // namespace

extern "C" {

int ssq_ssq_stft2_host(int dtype, const void* x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                       int64_t hop, double fs, int padtype, int squeezing, double gamma, int variant, void* Tx,
                       double* ssq_freqs, void* Sx, void* w2) {
  if (!x || !window || !Tx || !Sx) SSQ_FAIL("NULL argument");
  const FrameCall c{dtype, batch, n_signal, window, n_fft, hop, fs, padtype, gamma, variant, squeezing};
  Sst2Shape s;
  if (int rc = sst2_shape("ssq_stft2", nullptr, c, &s)) return rc;
  fill_ssq_freqs(ssq_freqs, s.sfs, variant);
  if (int rc = require_device()) return rc;
  const size_t el = dtype == SSQ_F32 ? 4 : 8, map_el = (size_t)s.n_freqs * (size_t)s.n_frames * el;
  const HostOut outs[] = {{Tx, 2 * map_el}, {Sx, 2 * map_el}, {w2, map_el}};
  const size_t work = (size_t)sst2_work(dtype, 1, n_signal, s).bytes;
  return dtype == SSQ_F32 ? pipe_host<Sst2Pipe<float>>(c, s, x, el * (size_t)n_signal, outs, work)
                          : pipe_host<Sst2Pipe<double>>(c, s, x, el * (size_t)n_signal, outs, work);
}

int ssq_ssq_stft2_window_tables(const double* window, int64_t n_fft, double* g1, double* g2, double* tg, double* tg1) {
  if (!window || !g1 || !g2 || !tg || !tg1) SSQ_FAIL("NULL argument");
  if (n_fft < 16 || n_fft > 4096 || (n_fft & (n_fft - 1)) != 0)
    SSQ_FAIL("ssq_stft2: n_fft must be a power of two from 16 to 4096");
  const host::SstWindows w = host::sst_window_tables(window, n_fft);
  for (int64_t j = 0; j < n_fft; ++j) {
    g1[j] = w.g1[j];
    g2[j] = w.g2[j];
    tg[j] = w.tg[j];
    tg1[j] = w.tg1[j];
  }
  return 0;
}

int64_t ssq_ssq_stft2_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t n_fft, int64_t hop) {
  Sst2Shape s;
  if (sst2_shape("ssq_stft2", nullptr, frame_sizes_call(dtype, batch, n_signal, n_fft, hop), &s)) return -1;
  return sst2_work(dtype, batch, n_signal, s).bytes;
}

int ssq_ssq_stft2_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                       int64_t hop, double fs, int padtype, int squeezing, double gamma, int variant, void* d_Tx, void* d_Sx,
                       void* d_w2, void* d_workspace, int64_t workspace_bytes, float* kernel_ms) {
  if (!d_x || !window || !d_Tx || !d_Sx || !d_workspace) SSQ_FAIL("NULL argument");
  const FrameCall c{dtype, batch, n_signal, window, n_fft, hop, fs, padtype, gamma, variant, squeezing};
  Sst2Shape s;
  if (int rc = sst2_shape("ssq_stft2", nullptr, c, &s)) return rc;
  if (workspace_bytes < sst2_work(dtype, batch, n_signal, s).bytes)
    SSQ_FAIL("ssq_stft2: workspace smaller than ssq_ssq_stft2_workspace_bytes");
  if (int rc = require_device()) return rc;
  void* const outs[] = {d_Tx, d_Sx, d_w2};
  return dtype == SSQ_F32 ? pipe_exec<Sst2Pipe<float>>(c, s, d_x, outs, d_workspace, kernel_ms)
                          : pipe_exec<Sst2Pipe<double>>(c, s, d_x, outs, d_workspace, kernel_ms);
}

}  // extern "C"
