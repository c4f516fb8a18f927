// stft_conceft.hip -- ConceFT on the STFT, the multitaper synchrosqueezed STFT `upstream.conceft_stft` (DESIGN 4.19;
// Daubechies, Wang and Wu 2016).  Upstream has no such transform: the definition is the project's own, restated in numpy
// by tests/helpers/conceft_stft_ref.py.  Per-sample units, fs enters where ssq_stft2 lets it enter.  With n = n_fft,
// c = n/2, the J real tapers h_j sized to n, g1_j their spectral derivatives (Nyquist term zeroed) and M unit vectors r_m
// in C^J, gauged by the caller so that c_m = sum_j r_mj h_j[c] > 0:
//   V_j, V1_j = the STFTs of x with h_j, g1_j (padding, hop and `modulated` rotation of ssq_stft2), in fp64 for either
//               dtype, rounded once to the call's dtype
//   S = sum_j r_mj V_j,  dS = sum_j r_mj V1_j                 j ascending, in the call's dtype
//   w = fs |k/n - Im(dS/S)/(2 pi)|  (sst2_operator's re1), kept where |S| > gamma;  bin = sst2_bin's rule on w
//   Tx[bin, t] += S (dw h_0[c] / sum_m c_m)                   the factor rounded once to the dtype
//
//   conceft_stft_planes_kernel : stage 1, on the frame pipeline of stft_frames64.h as sst2_operator_kernel runs it: a
//                          workgroup of 256 lanes owns a tile of consecutive frames of one signal; the frame's 16
//                          samples per lane are loaded ONCE, then one packed transform x (h_j + i a1 g1_j) per taper,
//                          the packed pair split through the frame's exchange row, and V_j, V1_j out through the LDS
//                          transpose so that global stores run along frames.  The planes of a slice go to the caller's
//                          workspace as [signal][2 J][F][slice frames].
//   conceft_stft_squeeze_kernel : stage 2, cwt_conceft_kernel's schedule on the linear grid: one thread owns a column of
//                          Tx (lanes along frames: every load and store is coalesced) and is its only writer; no
//                          atomics.  The draws go in register chunks of kConceftStftDraws; per row the chunk's
//                          combinations and bins are formed first, then a (current bin, complex sum) pair per draw: a
//                          run of rows landing in one bin is summed in registers and flushed by one plain
//                          read-modify-write.  The order of the additions into a cell is fixed by the column alone:
//                          chunks ascending, rows ascending, draws ascending.  It depends neither on the batch nor on the
//                          slices of the workspace.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ssq_hip.h"
#include "dev_buffers.h"
#include "sst_tables.h"
#include "stft_frames64.h"

namespace ssq {

// draws per register chunk (profiles/conceft_stft_resources.txt)
constexpr int kConceftStftDraws = 8;
constexpr int kConceftStftMaxTapers = 8;   // upstream.CONCEFT_MAX_ORDERS
constexpr int kConceftStftMaxDraws = 256;  // upstream.CONCEFT_MAX_DRAWS

template <typename O>
struct CfPlanesDev {
  const double* x;         // [signals][n_signal], widened (widen_f64) for a float32 call
  const cpx<double>* tw;   // the passes' twiddle tables (sst_tables.h: pass_twiddles)
  const cpx<double>* wa;   // [J][n] (h_j, g1_j a1_j) by frame sample; a1_j: the power of two that levels g1_j
  const double* h1;        // [J] 0.5 / a1_j
  cpx<O>* planes;          // [signals][2 J][F][pitch]: V_0 .. V_{J-1}, V1_0 .. V1_{J-1} of the frames f_begin .. f_stop - 1
  cpx<O>* Sx;              // [signals][J][F][n_frames] or nullptr: the planes V_j where the caller asks for them
  cpx<O>* dSx;             // likewise V1_j
  long long n_signal, n_frames, pitch, f_begin, f_stop;
  int J, hop, pad_left, padtype, rot, tile_frames;
};

template <typename O, int LOGN>
__global__ __launch_bounds__(kFrameThreads) void conceft_stft_planes_kernel(const CfPlanesDev<O> p) {
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
  const long long plane = (long long)F * p.pitch;
  const T* __restrict__ xs = p.x + b * p.n_signal;
  cpx<O>* __restrict__ out = p.planes + b * 2 * p.J * plane;
  cpx<O>* __restrict__ Sx = p.Sx ? p.Sx + b * p.J * (long long)F * nfr : nullptr;
  cpx<O>* __restrict__ dSx = p.dSx ? p.dSx + b * p.J * (long long)F * nfr : nullptr;
  const long long f_tile = p.f_begin + (long long)blockIdx.x * p.tile_frames;
  const long long f_end = f_tile + p.tile_frames < p.f_stop ? f_tile + p.tile_frames : p.f_stop;

  for (long long fr0 = f_tile; fr0 < f_end; fr0 += TFS) {               // a round = a store tile: FPR frames side by side
    const long long f = fr0 + g;
    const bool valid = f < f_end;                                        // (a frame past the end transforms zeros)
    const long long pos0 = f * p.hop - p.pad_left;
    const bool interior = valid && pos0 >= 0 && pos0 + N <= p.n_signal;
    T xv[16];
    frame_samples<LOGN>(p, xs, pos0, t + opaque_zero(), valid, interior, reinterpret_cast<T*>(exch), xv);
    frame_sync<MULTI>();      // (an edge frame's samples went through the row: all read before the first exchange writes it)
    const int nft = (int)(f_end - fr0 < TFS ? f_end - fr0 : TFS);
    const long long col0 = fr0 - p.f_begin;
    // One packed transform per taper on the samples held in xv.  An opaque zero offset per transform (stft_frames64.h)
    // keeps the table loads where they are used; the scheduling barrier keeps a later taper's loads below the store.
#pragma unroll 1
    for (int j = 0; j < p.J; ++j) {
      {
        cpx<T> v[16];
        cpx<T> V[9], V1[9];
        const int z = opaque_zero(), tz = t + z;
        const cpx<T>* __restrict__ wa = p.wa + (long long)j * N + z;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const cpx<T> w = wa[(tz + L * q + p.rot) & (N - 1)];
          v[q] = {xv[q] * w.x, xv[q] * w.y};
        }
        fft_pass_compact<T, LOGN, 0, MULTI>(v, exch, p.tw + z, tz);
        frame_split<T, LOGN, MULTI>(v, exch, tz, (T)0.5, p.h1[j], V, V1);
#pragma unroll
        for (int q = 0; q < 9; ++q) {
          const int k = tz + L * q;
          if (k <= N / 2) {
            st_s[k * SP + g] = V[q];
            st_m[k * SP + g] = V1[q];
          }
        }
      }
      __syncthreads();
      cpx<O>* __restrict__ oV = out + (long long)j * plane + col0;
      cpx<O>* __restrict__ oD = out + (long long)(p.J + j) * plane + col0;
      for (int e = tid; e < F * TFS; e += kFrameThreads) {                // neighbouring lanes: neighbouring frames of a bin
        const int k = e / TFS, fl = e % TFS;
        if (fl < nft) {
          const cpx<T> S = st_s[k * SP + fl], D = st_m[k * SP + fl];
          const cpx<O> So = {(O)S.x, (O)S.y}, Do = {(O)D.x, (O)D.y};
          const long long o = (long long)k * p.pitch + fl;
          oV[o] = So;
          oD[o] = Do;
          if (Sx) Sx[((long long)j * F + k) * nfr + fr0 + fl] = So;
          if (dSx) dSx[((long long)j * F + k) * nfr + fr0 + fl] = Do;
        }
      }
      __syncthreads();
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

template <typename T>
struct CfSqueezeDev {
  const cpx<T>* planes;    // [signals][2 J][F][pitch]
  cpx<T>* Tx;              // [signals][F][n_frames], at the slice's first column; zero on entry
  T* w;                    // [signals][M][F][n_frames], at the slice's first column, or nullptr
  long long signals, pitch, n_frames, cols;
  int J, M, F, flip;
  T gamma, dw, fs, inv_n, fac;   // fac: dw h_0[c] / sum_m c_m, rounded once
};

// the draw's frequency (sst2_operator's re1 on the combination, in the call's dtype; +inf where the bin is not kept) and
// its bin (sst2_bin's rule; -1 where not kept)
template <typename T>
__device__ __forceinline__ int conceft_stft_bin(const CfSqueezeDev<T>& p, T eta, cpx<T> V, cpx<T> V1, T& w) {
  const T two_pi = (T)6.283185307179586;
  const T den = V.x * V.x + V.y * V.y;
  const T re1 = eta - (V1.y * V.x - V1.x * V.y) / (den * two_pi);
  w = (T)INFINITY;
  if (!(hypot(V.x, V.y) > p.gamma)) return -1;
  w = p.fs * fabs(re1);
  const int last = p.F - 1;
  const T v = fmax(w / p.dw, (T)0);
  int kk = (v >= (T)last) ? last : (int)rint(v);
  if (!(v == v)) kk = 0;
  if (p.flip) kk = last - kk;
  return kk;
}

// One chunk of draws on one column: the walk up the rows (cwt_conceft.hip's conceft_chunk on the linear grid).  FULL: the
// chunk holds kConceftStftDraws draws and the draw loops carry no guard.
template <typename T, bool FULL>
__device__ __forceinline__ void conceft_stft_chunk(const CfSqueezeDev<T>& p, const cpx<T>* __restrict__ vec,
                                                   const cpx<T>* __restrict__ Pb, cpx<T>* __restrict__ Tb,
                                                   T* __restrict__ wb, int mc) {
  constexpr int MC = kConceftStftDraws;
  const long long nfr = p.n_frames;
  const int F = p.F;
  const long long plane = (long long)F * p.pitch;
  const long long wplane = (long long)F * nfr;
  int k_cur[MC];
  cpx<T> acc[MC];
#pragma unroll
  for (int m = 0; m < MC; ++m) {
    k_cur[m] = -1;
    acc[m] = {(T)0, (T)0};
  }
  auto flush = [&](int k, cpx<T> a) {
    if (k < 0) return;
    cpx<T>* d = Tb + (long long)k * nfr;
    cpx<T> t = *d;
    t.x += a.x;
    t.y += a.y;
    *d = t;
  };
  for (int i = 0; i < F; ++i) {
    cpx<T> Sm[MC], dSm[MC];
#pragma unroll
    for (int m = 0; m < MC; ++m) {
      Sm[m] = {(T)0, (T)0};
      dSm[m] = {(T)0, (T)0};
    }
    for (int g = 0; g < p.J; ++g) {
      const cpx<T> a = Pb[(long long)g * plane + (long long)i * p.pitch];
      const cpx<T> d = Pb[(long long)(p.J + g) * plane + (long long)i * p.pitch];
#pragma unroll
      for (int m = 0; m < MC; ++m) {
        if (FULL || m < mc) {                              // (wave-uniform: the last chunk may be short)
          const cpx<T> v = vec[m * p.J + g];               // four fused multiply-adds a product, g ascending
          Sm[m].x = fma(-v.y, a.y, fma(v.x, a.x, Sm[m].x));
          Sm[m].y = fma(v.y, a.x, fma(v.x, a.y, Sm[m].y));
          dSm[m].x = fma(-v.y, d.y, fma(v.x, d.x, dSm[m].x));
          dSm[m].y = fma(v.y, d.x, fma(v.x, d.y, dSm[m].y));
        }
      }
    }
    const T eta = (T)i * p.inv_n;
    int kk[MC];
    T w[MC];
#pragma unroll
    for (int m = 0; m < MC; ++m) {
      kk[m] = -1;
      w[m] = (T)INFINITY;
      if (FULL || m < mc) kk[m] = conceft_stft_bin<T>(p, eta, Sm[m], dSm[m], w[m]);
    }
#pragma unroll
    for (int m = 0; m < MC; ++m) {
      if (FULL || m < mc) {
        if (wb) wb[(long long)m * wplane + (long long)i * nfr] = w[m];
        if (kk[m] != k_cur[m]) {
          flush(k_cur[m], acc[m]);
          k_cur[m] = kk[m];
          acc[m] = {(T)0, (T)0};
        }
        if (kk[m] >= 0) {
          acc[m].x += Sm[m].x * p.fac;
          acc[m].y += Sm[m].y * p.fac;
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MC; ++m)
    if (FULL || m < mc) flush(k_cur[m], acc[m]);
}

// grid (ceil(cols / 64), min(signals, 65535)), block 64: thread = column, the y blocks stride over the signals.
// vectors [M][J], the gauged unit vectors, are an argument of their own: const and restrict there, and indexed by
// wave-uniform values, so the compiler reads them through the scalar cache.
template <typename T>
__global__ __launch_bounds__(64) void conceft_stft_squeeze_kernel(const CfSqueezeDev<T> p,
                                                                  const cpx<T>* __restrict__ vectors) {
  constexpr int MC = kConceftStftDraws;
  const long long j = (long long)blockIdx.x * 64 + threadIdx.x;
  if (j >= p.cols) return;
  const long long plane = (long long)p.F * p.pitch;
  const long long tplane = (long long)p.F * p.n_frames;
  for (long long b = blockIdx.y; b < p.signals; b += gridDim.y) {
    const cpx<T>* __restrict__ Pb = p.planes + b * 2 * p.J * plane + j;
    cpx<T>* __restrict__ Tb = p.Tx + b * tplane + j;
    for (int m0 = 0; m0 < p.M; m0 += MC) {
      const int mc = (p.M - m0 < MC) ? p.M - m0 : MC;
      const cpx<T>* __restrict__ vec = vectors + (long long)m0 * p.J;
      T* __restrict__ wb = p.w ? p.w + (b * p.M + m0) * tplane + j : nullptr;
      if (mc == MC) conceft_stft_chunk<T, true>(p, vec, Pb, Tb, wb, mc);
      else conceft_stft_chunk<T, false>(p, vec, Pb, Tb, wb, mc);
    }
  }
}

}  // namespace ssq

using namespace ssq;

namespace {

struct CfStftCall {
  int dtype;
  int64_t batch, N;
  const double* tapers;       // [J][n_fft]
  int64_t J, n_fft, hop;
  double fs;
  int padtype;
  const double* vectors;      // [M][J] complex (interleaved)
  int64_t M;
  double scale, gamma;
  int variant;
  hipStream_t st;             // of the launches (the host door: the null stream)
  float* ms;                  // the exec door's kernel_ms (CfStftPipe), or nullptr
};

struct CfStftShape : FrameShape {
  int64_t tfs;                // frames of a store tile
  int64_t frame_bytes;        // the 2 J coefficients of every bin of one frame
  int64_t widen_bytes;        // the fp64 copy of one signal (float32 calls)
  int64_t min_bytes, pref_bytes;
  int64_t work_bytes = 0;     // of the workspace the call runs in (the doors set it): sets the inner slices
  double dw;
  std::vector<double> sfs;
};

// The preferred workspace: whole signals up to 1 GiB.  Measured against 128 MiB (DESIGN 4.19,
// profiles/conceft_stft_bench.txt): the squeeze kernel has one wave per 64 columns, so a wider slice, not a slice that
// still sits in the last-level cache, is what it needs; 128 MiB was 3 - 6 x slower.
constexpr int64_t kCfStftPrefBytes = (int64_t)1 << 30;

// the signals and frames of a slice that `work_bytes` >= min_bytes hold: whole signals where one fits, else runs of whole
// store tiles of one signal
void cf_stft_slice(const CfStftShape& s, int64_t batch, int64_t work_bytes, int64_t* nb, int64_t* sf) {
  const int64_t per_signal = s.widen_bytes + s.frame_bytes * s.n_frames;
  if (work_bytes >= per_signal) {
    *nb = std::min<int64_t>(batch, work_bytes / per_signal);
    *sf = s.n_frames;
  } else {
    *nb = 1;
    *sf = (work_bytes - s.widen_bytes) / (s.frame_bytes * s.tfs) * s.tfs;
  }
}

int cf_stft_shape(int dtype, int64_t batch, int64_t N, int64_t n_fft, int64_t hop, int64_t J, double fs, int padtype,
                  double gamma, CfStftShape* s) {
  const char* own = (J < 1 || J > kConceftStftMaxTapers) ? "n_tapers must be 1 .. 8" : nullptr;
  if (int rc = frame_shape("conceft_stft", true, own, dtype, batch, N, n_fft, hop, fs, padtype, gamma, s)) return rc;
  const int64_t csz = dtype == SSQ_F32 ? 8 : 16;
  if ((double)batch * (double)kConceftStftMaxDraws * (double)s->n_freqs * (double)s->n_frames * (double)csz > 9.0e18)
    SSQ_FAIL("conceft_stft: transform too large");
  s->tfs = 4096 / n_fft;                                       // FrameCfg<LOGN>::TFS
  s->frame_bytes = 2 * J * s->n_freqs * csz;
  s->widen_bytes = dtype == SSQ_F32 ? 8 * N : 0;
  s->min_bytes = s->widen_bytes + s->frame_bytes * s->tfs;
  const int64_t per_signal = s->widen_bytes + s->frame_bytes * s->n_frames;
  if (per_signal <= kCfStftPrefBytes) {
    s->pref_bytes = per_signal * std::min<int64_t>(batch, kCfStftPrefBytes / per_signal);
  } else {
    const int64_t tile = s->frame_bytes * s->tfs;
    s->pref_bytes = s->widen_bytes + tile * std::max<int64_t>(1, (kCfStftPrefBytes - s->widen_bytes) / tile);
  }
  s->pref_bytes = std::max(s->pref_bytes, s->min_bytes);
  s->sfs = host::np_linspace(0.0, 0.5 * fs, s->n_freqs);
  s->dw = s->sfs[1] - s->sfs[0];
  return 0;
}

int cf_stft_check(const CfStftCall& c, CfStftShape* s) {
  if (int rc = cf_stft_shape(c.dtype, c.batch, c.N, c.n_fft, c.hop, c.J, c.fs, c.padtype, c.gamma, s)) return rc;
  if (!c.tapers || !c.vectors) SSQ_FAIL("conceft_stft: NULL argument");
  if (c.M < 1 || c.M > kConceftStftMaxDraws)
    SSQ_FAIL("conceft_stft: n_draws must be 1 .. " + std::to_string(kConceftStftMaxDraws));
  if (!std::isfinite(c.scale) || !(c.scale > 0)) SSQ_FAIL("conceft_stft: scale must be positive and finite");
  for (int64_t i = 0; i < c.J * c.n_fft; ++i)
    if (!std::isfinite(c.tapers[i])) SSQ_FAIL("conceft_stft: tapers must be finite");
  for (int64_t i = 0; i < 2 * c.M * c.J; ++i)
    if (!std::isfinite(c.vectors[i])) SSQ_FAIL("conceft_stft: vectors must be finite");
  return 0;
}

template <typename T>
hipError_t cf_planes_launch(CfPlanesDev<T> p, int logn, long long frames, long long signals, hipStream_t stream) {
  return dispatch_logn(logn, [&](auto ln) {
    constexpr int LOGN = decltype(ln)::value;
    dim3 grid;
    if (hipError_t e = frame_grid<LOGN>(frames, signals, &p.tile_frames, &grid); e != hipSuccess) return e;
    hipLaunchKernelGGL((conceft_stft_planes_kernel<T, LOGN>), grid, dim3(kFrameThreads), 0, stream, p);
    return hipGetLastError();
  });
}

// conceft_stft on device buffers (pipe_host, pipe_exec).  A call's workspace of s.work_bytes >= s.min_bytes is fixed by
// the call, not by the signals of a host slice: run() walks its signals in inner slices of that workspace (cf_stft_slice),
// the plane kernel and the squeeze kernel alternating.  kernel_ms is therefore the pipe's own (c.ms, two floats: the
// squeeze kernel alone, then the plane kernel alone, each summed over the inner slices), not run_timed's.
template <typename T>
struct CfStftPipe {
  static constexpr int kMid = 0;
  const CfStftCall& c;
  const CfStftShape& s;
  DeviceBufs d;
  TimingEvents t;
  CfPlanesDev<T> p1;
  CfSqueezeDev<T> p2;
  const cpx<T>* vec;
  cpx<T>*Tx, *Sx, *dSx, *planes;
  T* w;
  double* xd;                 // float32 calls: [nb_slice][N]
  int64_t nb_slice, sf;       // signals and frames of an inner slice
  int tables() {
    const int64_t n = c.n_fft, J = c.J, M = c.M;
    std::vector<double> wa((size_t)(2 * J * n)), h1((size_t)J);
    for (int64_t j = 0; j < J; ++j) {
      const host::SstTables tb = host::sst_level_tables(c.tapers + j * n, n, host::kSstFirst);   // fp64 for either dtype
      std::copy(tb.wa.begin(), tb.wa.end(), wa.begin() + 2 * j * n);
      h1[(size_t)j] = tb.h1;
    }
    std::vector<cpx<T>> v((size_t)(M * J));
    for (int64_t i = 0; i < M * J; ++i) v[(size_t)i] = {(T)c.vectors[2 * i], (T)c.vectors[2 * i + 1]};
    p1 = CfPlanesDev<T>{};
    SSQ_HIP(d.upload(&p1.tw, host::pass_twiddles(s.logn)));
    SSQ_HIP(d.upload(&p1.wa, wa));
    SSQ_HIP(d.upload(&p1.h1, h1));
    SSQ_HIP(d.upload(&vec, v));
    p1.n_signal = c.N;
    p1.n_frames = s.n_frames;
    p1.J = (int)J;
    p1.hop = (int)c.hop;
    p1.pad_left = (int)(n / 2);                                // the larger half of the n - 1 pad samples on the left
    p1.padtype = c.padtype;
    p1.rot = (c.variant & SSQ_VARIANT_MODULATED) ? (int)(n / 2) : 0;
    p2 = CfSqueezeDev<T>{};
    p2.n_frames = s.n_frames;
    p2.J = (int)J;
    p2.M = (int)M;
    p2.F = (int)s.n_freqs;
    p2.flip = (c.variant & SSQ_VARIANT_FLIPUD) ? 1 : 0;
    p2.gamma = (T)s.gamma;
    p2.dw = (T)s.dw;
    p2.fs = (T)s.fs;
    p2.inv_n = (T)(1.0 / (double)n);
    p2.fac = (T)(s.dw * c.scale);
    return 0;
  }
  int bind(int64_t cap, void* const* outs /* Tx, Sx, dSx, w */, void* work) {
    Tx = (cpx<T>*)outs[0];
    Sx = (cpx<T>*)outs[1];
    dSx = (cpx<T>*)outs[2];
    w = (T*)outs[3];
    cf_stft_slice(s, cap, s.work_bytes, &nb_slice, &sf);
    xd = (double*)work;
    planes = (cpx<T>*)((char*)work + s.widen_bytes * nb_slice);
    p1.pitch = p2.pitch = sf;
    p2.planes = planes;
    if (c.ms) {
      c.ms[0] = c.ms[1] = 0.0f;
      SSQ_HIP(t.start(3, c.st));
    }
    return 0;
  }
  int run(int64_t nb_run, const void* d_x, const hipEvent_t*) {
    const int64_t N = c.N, J = c.J, M = c.M, F = s.n_freqs, nfr = s.n_frames;
    const size_t map_sig = (size_t)F * (size_t)nfr;
    const hipStream_t st = c.st;
    SSQ_HIP(hipMemsetAsync(Tx, 0, (size_t)nb_run * map_sig * sizeof(cpx<T>), st));
    for (int64_t b0 = 0; b0 < nb_run; b0 += nb_slice) {
      const int64_t nb = std::min(nb_slice, nb_run - b0);
      const double* x64;
      SSQ_HIP(frame_signals64((const T*)d_x + b0 * N, xd, (long long)nb * N, st, &x64));
      for (int64_t f0 = 0; f0 < nfr; f0 += sf) {
        const int64_t cols = std::min(sf, nfr - f0);
        if (c.ms) SSQ_HIP(hipEventRecord(t.ev[0], st));
        p1.f_begin = f0;
        p1.f_stop = f0 + cols;
        SSQ_HIP(for_signal_runs(nb, [&](int64_t b1, int64_t n1) {
          p1.x = x64 + b1 * N;
          p1.planes = planes + b1 * 2 * J * F * sf;
          p1.Sx = Sx ? Sx + (size_t)(b0 + b1) * J * map_sig : nullptr;
          p1.dSx = dSx ? dSx + (size_t)(b0 + b1) * J * map_sig : nullptr;
          return cf_planes_launch<T>(p1, s.logn, cols, n1, st);
        }));
        if (c.ms) SSQ_HIP(hipEventRecord(t.ev[1], st));
        p2.Tx = Tx + (size_t)b0 * map_sig + f0;
        p2.w = w ? w + (size_t)b0 * M * map_sig + f0 : nullptr;
        p2.signals = nb;
        p2.cols = cols;
        const dim3 grid((unsigned)((cols + 63) / 64), (unsigned)std::min<int64_t>(nb, 65535));
        hipLaunchKernelGGL((conceft_stft_squeeze_kernel<T>), grid, dim3(64), 0, st, p2, vec);
        SSQ_HIP(hipGetLastError());
        if (c.ms) {
          float ms1 = 0.0f, ms2 = 0.0f;
          SSQ_HIP(hipEventRecord(t.ev[2], st));
          SSQ_HIP(hipEventSynchronize(t.ev[2]));
          SSQ_HIP(hipEventElapsedTime(&ms1, t.ev[0], t.ev[1]));
          SSQ_HIP(hipEventElapsedTime(&ms2, t.ev[1], t.ev[2]));
          c.ms[0] += ms2;
          c.ms[1] += ms1;
        }
      }
    }
    return 0;
  }
};

}  // namespace

extern "C" {

int64_t ssq_conceft_stft_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t n_fft, int64_t hop,
                                         int64_t n_tapers, int64_t* min_bytes) {
  CfStftShape s;
  if (cf_stft_shape(dtype, batch, n_signal, n_fft, hop, n_tapers, 1.0, SSQ_PAD_REFLECT, -1.0, &s)) return -1;
  if (min_bytes) *min_bytes = s.min_bytes;
  return s.pref_bytes;
}

int ssq_conceft_stft_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, const double* tapers,
                          int64_t n_tapers, int64_t n_fft, int64_t hop, double fs, int padtype, const double* vectors,
                          int64_t n_draws, double scale, double gamma, int variant, void* d_Tx, void* d_Sx, void* d_dSx,
                          void* d_w, void* d_workspace, int64_t workspace_bytes, void* stream, float* kernel_ms) {
  if (!d_x || !d_Tx || !d_workspace) SSQ_FAIL("conceft_stft: NULL argument");
  const CfStftCall c{dtype, batch, n_signal, tapers, n_tapers, n_fft, hop, fs, padtype, vectors, n_draws, scale, gamma, variant,
                     static_cast<hipStream_t>(stream), kernel_ms};
  CfStftShape s;
  if (int rc = cf_stft_check(c, &s)) return rc;
  if (workspace_bytes < s.min_bytes)
    SSQ_FAIL("conceft_stft: workspace too small (" + std::to_string(workspace_bytes) + " < " + std::to_string(s.min_bytes) +
             " bytes: ssq_conceft_stft_workspace_bytes)");
  if (int rc = require_device()) return rc;
  s.work_bytes = workspace_bytes;
  void* const outs[] = {d_Tx, d_Sx, d_dSx, d_w};
  return dtype == SSQ_F32 ? pipe_exec<CfStftPipe<float>>(c, s, d_x, outs, d_workspace, nullptr, &c.st)
                          : pipe_exec<CfStftPipe<double>>(c, s, d_x, outs, d_workspace, nullptr, &c.st);
}

int ssq_conceft_stft_host(int dtype, const void* x, int64_t batch, int64_t n_signal, const double* tapers, int64_t n_tapers,
                          int64_t n_fft, int64_t hop, double fs, int padtype, const double* vectors, int64_t n_draws,
                          double scale, double gamma, int variant, int64_t work_limit_bytes, void* Tx, double* ssq_freqs,
                          void* Sx, void* dSx, void* w) {
  if (!x || !Tx) SSQ_FAIL("conceft_stft: NULL argument");
  const CfStftCall c{dtype, batch, n_signal, tapers, n_tapers, n_fft, hop, fs, padtype, vectors, n_draws, scale, gamma, variant,
                     nullptr, nullptr};
  CfStftShape s;
  if (int rc = cf_stft_check(c, &s)) return rc;
  if (work_limit_bytes < 0 || (work_limit_bytes > 0 && work_limit_bytes < s.min_bytes))
    SSQ_FAIL("conceft_stft: work_limit_bytes must be 0 or at least " + std::to_string(s.min_bytes) + " bytes");
  s.work_bytes = work_limit_bytes ? std::min(work_limit_bytes, s.pref_bytes) : s.pref_bytes;
  fill_ssq_freqs(ssq_freqs, s.sfs, variant);
  if (int rc = require_device()) return rc;
  const size_t el = dtype == SSQ_F32 ? 4 : 8, map_el = (size_t)s.n_freqs * (size_t)s.n_frames * el;
  const HostOut outs[] = {{Tx, 2 * map_el}, {Sx, 2 * map_el * (size_t)n_tapers}, {dSx, 2 * map_el * (size_t)n_tapers},
                          {w, map_el * (size_t)n_draws}};
  // the signals that fit beside the call's workspace; a workspace of whole signals holds no more of them than a slice has
  const int64_t slice = slice_signals(batch, host_signal_bytes(el * (size_t)n_signal, outs), (double)s.work_bytes, batch);
  s.work_bytes = std::min(s.work_bytes, std::max(s.min_bytes, slice * (s.widen_bytes + s.frame_bytes * s.n_frames)));
  const HostSlice sl{slice, (size_t)s.work_bytes};
  return dtype == SSQ_F32 ? pipe_host<CfStftPipe<float>>(c, s, x, el * (size_t)n_signal, outs, sl)
                          : pipe_host<CfStftPipe<double>>(c, s, x, el * (size_t)n_signal, outs, sl);
}

}  // extern "C"
