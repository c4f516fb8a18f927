// stft_tsst.hip -- time-reassigned synchrosqueezed STFT, `upstream.tssq_stft`, orders 1 and 2 (He, Tu, Bao,
// Hu and Zhang 2019).  Upstream has no such transform: the definition is the project's own, restated in numpy by
// tests/helpers/tsst_ref.py.  It is the dual of stft_sst2.hip: every coefficient moves along TIME to its estimated group
// delay.  Per-sample units, fs enters at the end.  With n = n_fft, u[j] = j - n/2, the five windows g, g1, g2, tg, tg1
// of stft_sst2.hip and V, V1, V2, Vt, Vt1 the STFTs of x with them (frame m centred on sample m hop):
//   d1 = Re(Vt/V)       D = Vt V1 - Vt1 V       num = V2 V - V1^2       d2 = Re(Vt/V + V1 D / (V num))
//   offset = d2 where order = 2, |num| > gamma^2, d2 is finite and |d2| <= n/2, else d1; clamped to [-n/2, n/2]
//   tau = offset / fs (fp64, rounded once to the call's dtype), +inf where |V| <= gamma
//   r = rint(tau / (hop/fs)) in the call's dtype (0 where not finite)      m' = clip(m + r, 0, n_frames - 1)
//   Tx[k, m'] += Sx[k, m] exp(-2 pi i ((k (m - m') hop) mod n) / n)         in ascending source frame m
//
//   tsst_operator_kernel : stft_sst2.hip's frame ownership and transforms (the shared pieces are stft_frames64.h's,
//                          the transform block is written out here in its order): 256 lanes own a tile of
//                          consecutive frames, n/16 lanes a frame, three packed fp64 transforms for order 2, ONE
//                          (x (g + i tg)) for order 1; the time operator per
//                          bin; Sx, tau and the relative target r (int16, kTsstNone where the bin is not kept) out
//                          through the LDS transpose, so that global stores run along frames.
//   tsst_scatter_kernel  : a workgroup owns a tile of target frames of one row and stages the int16 targets of the
//                          sources within H = ceil(n / (2 hop)) frames of it in LDS.  A wave owns 64 consecutive target
//                          cells, one per lane, walks the sources 64 at a time in ascending order, and hands the hits
//                          of each step to the lanes that own their cells: all at once where no two hits of the step
//                          share a cell (the usual case), else one by one in ascending lane order (ballot, readlane).
//                          The owner adds them with a compensated (Neumaier) fp64 sum.  Every cell is therefore the sum of
//                          its contributions in ascending source frame whatever the tiling or the batch, no atomics,
//                          and every cell of Tx is written exactly once (no clear of Tx).
// The two halves (tsst_operator_run, tsst_scatter_run) are lent to stft_tmsst.hip through stft_tsst.h, which
// runs the scatter's other instantiations: a reach of several windows, trimmed to what a workgroup's map really moves.
#include <cmath>
#include <vector>

#include "../../include/ssq_hip.h"
#include "dev_buffers.h"
#include "sst_tables.h"
#include "stft_frames64.h"
#include "stft_tsst.h"

namespace ssq {

// (the constants and the parameter blocks TsstOut, TsstDev, TsstScat: stft_tsst.h, shared with stft_tmsst.hip)
// first order: the group-delay offset Re(Vt / V) in samples, or +inf where the bin is not kept
template <typename O>
__device__ __forceinline__ double tsst_operator1(const TsstDev<O>& p, double half, cpx<double> V, cpx<double> Vt) {
  const double den = V.x * V.x + V.y * V.y;
  const double d1 = (Vt.x * V.x + Vt.y * V.y) / den;
  return hypot(V.x, V.y) > p.gamma ? clamp_keep_nan(d1, half) : (double)INFINITY;
}

// second order: Re(Vt/V + V1 D / (V num)) where the chirp fit is usable, else the first-order offset
template <typename O>
__device__ __forceinline__ double tsst_operator2(const TsstDev<O>& p, double half, cpx<double> V, cpx<double> V1,
                                                 cpx<double> V2, cpx<double> Vt, cpx<double> Vt1) {
  using T = double;
  const T den = V.x * V.x + V.y * V.y;
  const T d1 = (Vt.x * V.x + Vt.y * V.y) / den;
  const cpx<T> D = cmul(Vt, V1) - cmul(Vt1, V);
  const cpx<T> num = cmul(V2, V) - cmul(V1, V1);
  const cpx<T> a = cmul(V1, D), b = cmul(V, num);
  const T d2 = d1 + (a.x * b.x + a.y * b.y) / (b.x * b.x + b.y * b.y);     // Re(a / b)
  const bool second = hypot(num.x, num.y) > p.gamma_sq && isfinite(d2) && fabs(d2) <= half;
  return hypot(V.x, V.y) > p.gamma ? clamp_keep_nan(second ? d2 : d1, half) : (T)INFINITY;
}

template <typename O, int LOGN, int ORDER>
__global__ __launch_bounds__(kFrameThreads) void tsst_operator_kernel(const TsstDev<O> p) {
  using T = double;
  using C = FrameCfg<LOGN>;
  constexpr int N = C::N, L = C::L, FPR = C::FPR, ROW = C::ROW, F = C::F, TFS = C::TFS, SP = C::SP;
  constexpr bool MULTI = C::MULTI;
  __shared__ __attribute__((aligned(16))) cpx<T> exch_all[FPR * ROW];
  __shared__ __attribute__((aligned(16))) cpx<T> st_s[F * SP];
  __shared__ __attribute__((aligned(16))) cpx<T> st_m[F * SP];      // order 2: V1, then (offset or inf, -)

  const int tid = threadIdx.x;
  int g = tid / L;                                         // frame slot of the round
  const int t = tid % L;                                   // lane inside the frame
  if constexpr (L >= 64) g = __builtin_amdgcn_readfirstlane(g);        // one frame (or part of one) per wave: scalar
  cpx<T>* exch = exch_all + g * ROW;

  const long long nfr = p.n_frames;
  const long long b = (long long)blockIdx.y + p.b0;
  const int f_tile = (int)blockIdx.x * p.tile_frames;                   // frames fit an int: n_frames <= 2^30
  const int f_end = (long long)f_tile + p.tile_frames < nfr ? f_tile + p.tile_frames : (int)nfr;

  for (int fr0 = f_tile; fr0 < f_end; fr0 += TFS) {                     // a round = a store tile: FPR frames side by side
    {
      const int f = fr0 + g;
      const bool valid = f < f_end;                                      // (a frame past the end transforms zeros)
      const long long pos0 = (long long)f * p.hop - N / 2;              // the larger half of the n - 1 pad samples on the left
      const T* __restrict__ xs = p.x + (b + opaque_zero()) * p.n_signal;   // (formed per round, not held)
      const bool interior = valid && pos0 >= 0 && pos0 + N <= p.n_signal;
      T xv[16];
      frame_samples<LOGN>(p, xs, pos0, t + opaque_zero(), valid, interior, reinterpret_cast<T*>(exch), xv);
      frame_sync<MULTI>();      // (an edge frame's samples went through the row: all read before the first exchange writes it)
      const int slot = g;
      cpx<T> v[16];
      if constexpr (ORDER == 1) {
        // one packed transform x (g + i tg): V and Vt are all the first-order offset needs
        cpx<T> V[9], Vt[9];
        const int z = opaque_zero(), tz = t + z;
        const cpx<T>* __restrict__ wa = p.wa + z;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const cpx<T> w = wa[(tz + L * q + p.rot) & (N - 1)];
          v[q] = {xv[q] * w.x, xv[q] * w.y};
        }
        fft_pass_compact<T, LOGN, 0, MULTI>(v, exch, p.tw + z, tz);
        frame_split<T, LOGN, MULTI>(v, exch, tz, (T)0.5, p.it, V, Vt);
#pragma unroll
        for (int q = 0; q < 9; ++q) {
          const int k = tz + L * q;
          if (k <= N / 2) {
            st_s[k * SP + slot] = V[q];
            st_m[k * SP + slot] = {tsst_operator1<O>(p, (T)(N / 2), V[q], Vt[q]), (T)0};
          }
        }
      } else {
        // The three transforms of stft_sst2.hip, in its order and with its opaque offsets (stft_frames64.h) and
        // scheduling barriers (what keeps the kernel inside 256 registers): (g, g1) first, V into the store
        // tile and V1 parked in the lane's own map slots; tg alone; (tg1, g2) last.
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
          const T* __restrict__ wb = p.wb + z;                           // real input: its spectrum is the transform itself
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
        const int te = t + opaque_zero();
#pragma unroll
        for (int q = 0; q < 9; ++q) {
          const int k = te + L * q;
          if (k <= N / 2) {
            const cpx<T> V = st_s[k * SP + slot], V1 = st_m[k * SP + slot];
            st_m[k * SP + slot] = {tsst_operator2<O>(p, (T)(N / 2), V, V1, V2[q], Vt[q], Vt1[q]), (T)0};
          }
        }
      }
    }
    __syncthreads();
    // the outputs' addresses are fetched and formed here, so that no pointer is held across the transforms
    const TsstOut<O> po = p.out[opaque_zero()];
    const long long ob = b * (long long)F * nfr;
    cpx<O>* __restrict__ Sx = po.Sx + ob;
    O* __restrict__ tau_out = po.tau ? po.tau + ob : nullptr;
    short* __restrict__ rel_out = po.rel + ob;
    const int nft = f_end - fr0 < TFS ? f_end - fr0 : TFS;
    for (int e = tid; e < F * TFS; e += kFrameThreads) {                  // neighbouring lanes: neighbouring frames of a bin
      const int k = e / TFS, fl = e % TFS;
      if (fl < nft) {
        const long long m = (long long)fr0 + fl, o = (long long)k * nfr + m;
        const cpx<T> S = st_s[k * SP + fl];
        Sx[o] = {(O)S.x, (O)S.y};
        const T off = st_m[k * SP + fl].x;
        O tau = (O)INFINITY;
        int rel = kTsstNone;
        if (off != (T)INFINITY) {
          tau = (O)(off / po.fs);
          const O v = tau / po.step;
          // |r| <= ceil(n / (2 hop)), the offset being clamped; the bound below only keeps a quotient of denormals
          // (an fs next to the dtype's smallest number) inside an int16
          const O rv = isfinite(v) ? rint(v) : (O)0;
          const long long r = (long long)(rv < (O)-4096 ? (O)-4096 : (rv > (O)4096 ? (O)4096 : rv));
          long long mt = m + r;
          mt = mt < 0 ? 0 : (mt > nfr - 1 ? nfr - 1 : mt);
          rel = (int)(mt - m);
        }
        if (tau_out) tau_out[o] = tau;
        rel_out[o] = (short)rel;
      }
    }
    __syncthreads();
  }
}

__device__ __forceinline__ void tsst_neumaier(double& s, double& c, double x) {
  const double t = s + x;
  c += fabs(s) >= fabs(x) ? (s - t) + x : (x - t) + s;
  s = t;
}

// lane j's value of v, j the same in every lane
__device__ __forceinline__ double tsst_readlane(double v, int j) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}

// STAGE: the int16 targets a workgroup stages, tile + 2 reach at the most (kTsstStage: tssq_stft's one-window reach;
// kTsstWideStage: a walked map's, stft_tmsst.hip).  TRIM: the workgroup walks only the sources within the largest
// |target| it staged -- a source farther from a cell than that cannot hit it, and the hits of a cell still arrive in
// ascending source frame, so every cell is the same sum; what a map that moves little saves is the walk over a reach of
// several windows.  tssq_stft runs <kTsstStage, false>, the kernel as it was.
template <typename O, int STAGE, bool TRIM>
__global__ __launch_bounds__(kTsstThreads) void tsst_scatter_kernel(const TsstScat<O> p) {
  __shared__ short rel_s[STAGE];
  __shared__ int slot_s[kTsstThreads];
  const long long nfr = p.n_frames;
  const int k = blockIdx.y;
  const long long base = ((long long)blockIdx.z * p.n_freqs + k) * nfr;
  const long long t0 = (long long)blockIdx.x * p.tile;                    // the targets [t0, t1) are this workgroup's
  const long long t1 = t0 + p.tile < nfr ? t0 + p.tile : nfr;
  const long long s0 = t0 - p.reach > 0 ? t0 - p.reach : 0;              // the sources [s0, s1) can reach them
  const long long s1 = t1 + p.reach < nfr ? t1 + p.reach : nfr;
  const int tid = threadIdx.x;
  int far = 0;                                                             // TRIM: the largest |target| staged
  for (int i = tid; i < (int)(s1 - s0); i += kTsstThreads) {
    const short r = p.rel[base + s0 + i];
    rel_s[i] = r;
    if constexpr (TRIM) {
      const int a = r < 0 ? -(int)r : (int)r;
      if (r != kTsstNone && a > far) far = a;
    }
  }
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  int reach = p.reach;
  if constexpr (TRIM) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const int o = __shfl_xor(far, d);
      far = o > far ? o : far;
    }
    if (lane == 0) slot_s[wave] = far;
    __syncthreads();
    for (int w = 0; w < kTsstThreads / 64; ++w) far = slot_s[w] > far ? slot_s[w] : far;
    reach = __builtin_amdgcn_readfirstlane(far < reach ? far : reach);
  }
  __syncthreads();                                                         // (TRIM: slot_s is the waves' own from here on)
  volatile int* slot = slot_s + 64 * wave;                                // the wave's own 64 slots: no workgroup barrier
  for (long long g0 = t0 + 64 * wave; g0 < t1; g0 += kTsstThreads) {     // the wave's 64 cells, one per lane
    double sr = 0, si = 0, cr = 0, ci = 0;
    for (long long c0 = g0 - reach; c0 <= g0 + 63 + reach; c0 += 64) {   // 64 sources a step, ascending
      const long long m = c0 + lane;
      int r = kTsstNone;
      if (m >= s0 && m < s1) r = rel_s[m - s0];
      const long long tl = m + r - g0;
      const bool hit = r != kTsstNone && tl >= 0 && tl < 64;
      double zr = 0, zi = 0;
      if (hit) {
        const cpx<O> S = p.Sx[base + m];
        // (k (m - m') hop) mod n = (-k r hop) mod n: the factors reduced first, so that the product stays in an int
        const int rh = (int)(((long long)r * p.hop) & (p.n - 1));
        const cpx<double> w = p.rot[(p.n - ((k * rh) & (p.n - 1))) & (p.n - 1)];
        zr = (double)S.x * w.x - (double)S.y * w.y;
        zi = (double)S.x * w.y + (double)S.y * w.x;
      }
      unsigned long long mask = __ballot(hit);
      if (mask) {
        // Which cells does this step feed?  Every hit writes its lane into its cell's slot; a hit that does not read its
        // own lane back shares the cell with another hit of the step.
        slot[lane] = -1;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (hit) slot[(int)tl] = lane;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        const int from = slot[lane];
        const bool clash = hit && slot[(int)tl] != lane;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");             // (all read before the next step writes)
        if (__ballot(clash) == 0) {
          // at most one value a cell: the order inside the step does not enter, all cells take theirs at once
          const int src = from < 0 ? lane : from;
          const double ar = __shfl(zr, src), ai = __shfl(zi, src);
          if (from >= 0) {
            tsst_neumaier(sr, cr, ar);
            tsst_neumaier(si, ci, ai);
          }
        } else {
          while (mask) {                                                   // the step's hits in ascending source frame
            const int j = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const int tj = __builtin_amdgcn_readlane((int)tl, j);
            const double ar = tsst_readlane(zr, j), ai = tsst_readlane(zi, j);
            if (lane == tj) {
              tsst_neumaier(sr, cr, ar);
              tsst_neumaier(si, ci, ai);
            }
          }
        }
      }
    }
    if (g0 + lane < t1) p.Tx[base + g0 + lane] = {(O)(sr + cr), (O)(si + ci)};
  }
}

template <typename T>
static hipError_t tsst_launch(TsstDev<T> p, int logn, int order, long long batch, hipStream_t stream) {
  return dispatch_logn(logn, [&](auto ln) {
    constexpr int LOGN = decltype(ln)::value;
    dim3 grid;
    if (hipError_t e = frame_grid<LOGN>(p.n_frames, batch, &p.tile_frames, &grid); e != hipSuccess) return e;
    if (order == 1)
      hipLaunchKernelGGL((tsst_operator_kernel<T, LOGN, 1>), grid, dim3(kFrameThreads), 0, stream, p);
    else
      hipLaunchKernelGGL((tsst_operator_kernel<T, LOGN, 2>), grid, dim3(kFrameThreads), 0, stream, p);
    return hipGetLastError();
  });
}

// The argument checks of the entry points, and the shape they work on (sets the error and returns non-zero)
int tsst_shape(const char* name, const char* own_fail, const FrameCall& c, TsstShape* s) {
  if (int rc = frame_shape(name, true, own_fail, c, s)) return rc;
  s->order = c.order;
  s->tile = tsst_tile(s->reach);                             // halo re-read (tile + 2 H) / tile <= 2
  return 0;
}

// the call's tables on the device (held by `d`) and the two parameter blocks without their signal / output pointers
template <typename T>
int tsst_tables(DeviceBufs& d, const TsstShape& s, const FrameCall& c, TsstDev<T>* p, TsstScat<T>* sc) {
  const int64_t n = c.n_fft;
  const host::SstTables t = host::sst_level_tables(c.window, n, s.order == 1 ? host::kSstTimeFirst : host::kSstSecond);
  const std::vector<double> tw = host::pass_twiddles(s.logn);
  std::vector<cpx<double>> rot((size_t)n);
  for (int64_t j = 0; j < n; ++j) {
    const long double ang = 2.0L * 3.14159265358979323846264338327950288L * (long double)j / (long double)n;
    rot[j] = {(double)cosl(ang), (double)(-sinl(ang))};
  }
  void *d_tw, *d_wa, *d_wb, *d_wc, *d_rot;
  SSQ_HIP(d.upload(&d_tw, tw.data(), sizeof(double) * tw.size()));
  SSQ_HIP(d.upload(&d_wa, t.wa.data(), sizeof(cpx<double>) * n));
  SSQ_HIP(d.upload(&d_wb, t.wb.data(), sizeof(double) * n));
  SSQ_HIP(d.upload(&d_wc, t.wc.data(), sizeof(cpx<double>) * n));
  SSQ_HIP(d.upload(&d_rot, rot.data(), sizeof(cpx<double>) * n));
  *p = TsstDev<T>{};
  p->tw = (const cpx<double>*)d_tw;
  p->wa = (const cpx<double>*)d_wa;
  p->wb = (const double*)d_wb;
  p->wc = (const cpx<double>*)d_wc;
  p->n_signal = c.n_signal;
  p->n_frames = s.n_frames;
  p->hop = (int)c.hop;
  p->padtype = c.padtype;
  p->rot = (c.variant & SSQ_VARIANT_MODULATED) ? (int)(n / 2) : 0;
  p->gamma = s.gamma;
  p->gamma_sq = s.gamma * s.gamma;
  p->h1 = t.h1;
  p->it = t.it;
  p->ht1 = t.ht1;
  p->h2 = t.h2;
  *sc = TsstScat<T>{};
  sc->rot = (const cpx<double>*)d_rot;
  sc->n_frames = s.n_frames;
  sc->n_freqs = (int)s.n_freqs;
  sc->n = (int)n;
  sc->hop = (int)c.hop;
  sc->reach = s.reach;
  sc->tile = s.tile;
  return 0;
}

// the operator kernel's output block (TsstOut) on the device, held by `d`
template <typename T>
int tsst_out_block(DeviceBufs& d, const TsstShape& s, int64_t hop, void* d_Sx, void* d_tau, void* d_rel, TsstDev<T>* p) {
  TsstOut<T> o{};
  o.Sx = (cpx<T>*)d_Sx;
  o.tau = (T*)d_tau;
  o.rel = (short*)d_rel;
  o.fs = s.fs;
  o.step = (T)((double)hop / s.fs);
  void* d_o;
  SSQ_HIP(d.upload(&d_o, &o, sizeof(o)));
  p->out = (const TsstOut<T>*)d_o;
  return 0;
}

template <typename T>
hipError_t tsst_operator_run(TsstDev<T> p, const TsstShape& s, const T* d_x, int64_t nb,
                             double* d_xd /* float32 calls: [nb][n_signal] */) {
  if (hipError_t e = frame_signals64(d_x, d_xd, (long long)nb * p.n_signal, nullptr, &p.x); e != hipSuccess) return e;
  return for_signal_runs(nb, [&](int64_t b0, int64_t n1) {
    p.b0 = (int)b0;
    return tsst_launch<T>(p, s.logn, s.order, n1, nullptr);
  });
}

template <typename T>
hipError_t tsst_scatter_run(TsstScat<T> sc, const TsstShape& s, int64_t nb, const cpx<T>* d_Sx, const short* d_rel,
                            cpx<T>* d_Tx, bool trim) {
  const size_t map_sig = (size_t)s.n_freqs * (size_t)s.n_frames;
  const long long tiles = (s.n_frames + sc.tile - 1) / sc.tile;
  const long long stage = (long long)sc.tile + 2LL * sc.reach;
  if (sc.reach < 1 || sc.tile < 256 || sc.tile % 256 || sc.tile > kTsstMaxTile || stage > kTsstWideStage ||
      (!trim && stage > kTsstStage))
    return hipErrorInvalidValue;
  return for_signal_runs(nb, [&](int64_t b0, int64_t n1) {
    sc.Sx = d_Sx + map_sig * b0;
    sc.rel = d_rel + map_sig * b0;
    sc.Tx = d_Tx + map_sig * b0;
    const dim3 grid((unsigned)tiles, (unsigned)s.n_freqs, (unsigned)n1);
    if (!trim)
      hipLaunchKernelGGL((tsst_scatter_kernel<T, kTsstStage, false>), grid, dim3(kTsstThreads), 0, nullptr, sc);
    else if (stage <= kTsstStage)
      hipLaunchKernelGGL((tsst_scatter_kernel<T, kTsstStage, true>), grid, dim3(kTsstThreads), 0, nullptr, sc);
    else
      hipLaunchKernelGGL((tsst_scatter_kernel<T, kTsstWideStage, true>), grid, dim3(kTsstThreads), 0, nullptr, sc);
    return hipGetLastError();
  });
}

#define SSQ_TSST_INSTANTIATE(T)                                                                                          \
  template int tsst_tables<T>(DeviceBufs&, const TsstShape&, const FrameCall&, TsstDev<T>*, TsstScat<T>*);              \
  template int tsst_out_block<T>(DeviceBufs&, const TsstShape&, int64_t, void*, void*, void*, TsstDev<T>*);             \
  template hipError_t tsst_operator_run<T>(TsstDev<T>, const TsstShape&, const T*, int64_t, double*);                    \
  template hipError_t tsst_scatter_run<T>(TsstScat<T>, const TsstShape&, int64_t, const cpx<T>*, const short*, cpx<T>*,  \
                                          bool);
SSQ_TSST_INSTANTIATE(float)
SSQ_TSST_INSTANTIATE(double)
#undef SSQ_TSST_INSTANTIATE

}  // namespace ssq

using namespace ssq;

namespace {

const char* tsst_own_fail(int order) { return order == 1 || order == 2 ? nullptr : "order must be 1 or 2"; }

// tssq_stft on device buffers (pipe_host, pipe_exec): the operator, then the time scatter.  kernel_ms: two parts, the
// event recorded between the two.
template <typename T>
struct TsstPipe {
  static constexpr int kMid = 1;
  const FrameCall& c;
  const TsstShape& s;
  DeviceBufs d;
  TsstDev<T> p;
  TsstScat<T> sc;
  cpx<T>*Tx, *Sx;
  short* rel;
  double* xd;
  int tables() { return tsst_tables<T>(d, s, c, &p, &sc); }
  int bind(int64_t cap, void* const* outs /* Tx, Sx, tau */, void* work) {
    const TsstWork k = tsst_work(c.dtype, cap, c.n_signal, s, false);
    Tx = (cpx<T>*)outs[0];
    Sx = (cpx<T>*)outs[1];
    xd = (double*)((char*)work + k.xd);
    rel = (short*)((char*)work + k.rel);
    return tsst_out_block<T>(d, s, c.hop, Sx, outs[2], rel, &p);
  }
  int run(int64_t nb, const void* d_x, const hipEvent_t* mid) {
    SSQ_HIP(tsst_operator_run<T>(p, s, (const T*)d_x, nb, xd));
    if (mid[0]) SSQ_HIP(hipEventRecord(mid[0], nullptr));
    SSQ_HIP(tsst_scatter_run<T>(sc, s, nb, Sx, rel, Tx, false));
    return 0;
  }
};

}  // namespace

extern "C" {

int ssq_tssq_stft_host(int dtype, const void* x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                       int64_t hop, double fs, int padtype, int order, double gamma, int variant, void* Tx, void* Sx,
                       void* tau) {
  if (!x || !window || !Tx || !Sx) SSQ_FAIL("NULL argument");
  const FrameCall c{dtype, batch, n_signal, window, n_fft, hop, fs, padtype, gamma, variant, SSQ_SQUEEZE_SUM, order};
  TsstShape s;
  if (int rc = tsst_shape("tssq_stft", tsst_own_fail(order), c, &s)) return rc;
  if (int rc = require_device()) return rc;
  const size_t el = dtype == SSQ_F32 ? 4 : 8, map_el = (size_t)s.n_freqs * (size_t)s.n_frames * el;
  const HostOut outs[] = {{Tx, 2 * map_el}, {Sx, 2 * map_el}, {tau, map_el}};
  const size_t work = (size_t)tsst_work(dtype, 1, n_signal, s, false).bytes;
  return dtype == SSQ_F32 ? pipe_host<TsstPipe<float>>(c, s, x, el * (size_t)n_signal, outs, work)
                          : pipe_host<TsstPipe<double>>(c, s, x, el * (size_t)n_signal, outs, work);
}

int64_t ssq_tssq_stft_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t n_fft, int64_t hop) {
  TsstShape s;
  if (tsst_shape("tssq_stft", nullptr, frame_sizes_call(dtype, batch, n_signal, n_fft, hop), &s)) return -1;
  return tsst_work(dtype, batch, n_signal, s, false).bytes;
}

int ssq_tssq_stft_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                       int64_t hop, double fs, int padtype, int order, double gamma, int variant, void* d_Tx, void* d_Sx,
                       void* d_tau, void* d_workspace, int64_t workspace_bytes, float* kernel_ms) {
  if (!d_x || !window || !d_Tx || !d_Sx || !d_workspace) SSQ_FAIL("NULL argument");
  const FrameCall c{dtype, batch, n_signal, window, n_fft, hop, fs, padtype, gamma, variant, SSQ_SQUEEZE_SUM, order};
  TsstShape s;
  if (int rc = tsst_shape("tssq_stft", tsst_own_fail(order), c, &s)) return rc;
  if (workspace_bytes < tsst_work(dtype, batch, n_signal, s, false).bytes)
    SSQ_FAIL("tssq_stft: workspace smaller than ssq_tssq_stft_workspace_bytes");
  if (int rc = require_device()) return rc;
  void* const outs[] = {d_Tx, d_Sx, d_tau};
  return dtype == SSQ_F32 ? pipe_exec<TsstPipe<float>>(c, s, d_x, outs, d_workspace, kernel_ms)
                          : pipe_exec<TsstPipe<double>>(c, s, d_x, outs, d_workspace, kernel_ms);
}

}  // extern "C"
