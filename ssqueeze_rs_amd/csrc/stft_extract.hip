// stft_extract.hip -- synchroextracting and transient-extracting STFT, `upstream.set_stft` and `upstream.tet_stft`, orders
// 1 and 2 (Yu, Yu and Zhang 2017; Bao et al. 2019; Yu 2019).  Upstream has neither: the definition is the
// project's own, restated in numpy by tests/helpers/extract_ref.py.  Where the rest of the family MOVES a coefficient to
// where its estimate points, these KEEP it only where the estimate says it already sits on the ridge, and zero the rest.
// With the windows, the STFTs V, V1, V2, Vt, Vt1, the frequency w of stft_sst2.hip and the offset of stft_tsst.hip:
//   axis 0 (SET): w = fs |Re w2| where order = 2, |D| > gamma^2 and Re w2 is finite, else fs |Re w1|; rounded once to the
//                 call's dtype, +inf where |V| <= gamma;  b = the clamped round-half-even bin of w on
//                 np.linspace(0, fs/2, F) in the call's dtype (stft_sst2.hip's rule);  keep where b == k
//   axis 1 (TET): tau = offset / fs of stft_tsst.hip in the call's dtype, +inf where |V| <= gamma;
//                 r = rint(tau / (hop/fs)) in the call's dtype, BEFORE any clip to the frame range;  keep where r == 0
//   Te[k, m] = Sx[k, m] where |V| > gamma and the cell is kept, else +0 + 0i
// The decision is local to a cell, so the whole transform is the epilogue of the frame kernel: ONE launch, no packed map,
// no int16 plane, no clearing of Te (every cell is written exactly once) and no second kernel that reads Sx again.
//
//   extract_kernel : stft_sst2.hip's frame ownership and transforms (the shared pieces are stft_frames64.h's, the
//                    transform block is written out here in its order): 256 lanes own a tile of consecutive frames, n/16
//                    lanes a frame; three packed fp64 transforms for order 2, after which all five spectra are at hand
//                    and one instantiation serves both axes through a uniform branch; ONE packed transform for order 1,
//                    x (g + i g1) for SET and x (g + i tg) for TET, the same code on another second table.  Te, and Sx
//                    and the real map where asked for, leave through the LDS transpose, so that global stores run along
//                    frames.
#include <cmath>
#include <vector>

#include "../../include/ssq_hip.h"
#include "dev_buffers.h"
#include "sst_tables.h"
#include "stft_frames64.h"

namespace ssq {

// O: the dtype of the call (float or double: x in, Te / Sx / map out).  The transforms and the operators always run in
// fp64, on the widened signal, as in stft_sst2.hip.
// What the kernel needs only after the transforms: where it picks the operator (axis, fs, gamma) and where it stores a
// tile.  It lives in device memory and is read there, behind an opaque offset: as kernel arguments these would sit in
// scalar registers across the transforms, which are at the limit (106 SGPRs).
template <typename O>
struct ExtractOut {
  cpx<O>* Te;              // [batch][F][n_frames]
  cpx<O>* Sx;              // [batch][F][n_frames], or nullptr
  O* map;                  // [batch][F][n_frames], or nullptr: w (axis 0) or tau (axis 1)
  double fs, gamma;        // gamma: a cell is live where |V| > gamma; the second-order estimates where |D| or |num| > gamma^2
  O unit;                  // axis 0: Sfs[1] - Sfs[0]; axis 1: hop / fs -- in the call's dtype: the rule runs on the map the call reports
  int axis;                // 0: frequency (SET), 1: time (TET); read after the transforms, where the operator is picked
};

template <typename O>
struct ExtractDev {
  const double* x;         // [batch][n_signal], widened (widen_f64) for a float32 call
  const cpx<double>* tw;   // the passes' twiddle tables, passes 1, 2, .. back to back
  const cpx<double>* wa;   // order 2: (g, g1 a1); order 1: (g, g1 a1) for axis 0, (g, tg at) for axis 1
  const double* wb;        // order 2: tg at
  const cpx<double>* wc;   // order 2: (tg1 at1, g2 a2)
  const ExtractOut<O>* out;
  long long n_signal, n_frames;
  int hop, padtype, rot, b0;   // b0: the signal of blockIdx.y = 0
  double h1, it, ht1, h2;  // 0.5 / a1 (order 1, axis 1: 0.5 / at), 1 / at, 0.5 / at1, 0.5 / a2
};

struct ExtractShape : FrameShape {
  int order = 2, axis = 0;
  double dw = 0.0;
};

// axis 0, first order: fs |Re w1| (stft_sst2.hip's expression), or +inf where the bin is not live
template <typename O>
__device__ __forceinline__ double extract_freq1(double gamma, double fs, double eta, cpx<double> V, cpx<double> V1) {
  const double two_pi = 6.283185307179586;
  const double den = V.x * V.x + V.y * V.y;
  const double re1 = eta - (V1.y * V.x - V1.x * V.y) / (den * two_pi);
  return hypot(V.x, V.y) > gamma ? fs * fabs(re1) : (double)INFINITY;
}

// axis 0, second order: stft_sst2.hip's operator
template <typename O>
__device__ __forceinline__ double extract_freq2(double gamma, double fs, double eta, cpx<double> V, cpx<double> V1,
                                                cpx<double> V2, cpx<double> Vt, cpx<double> Vt1) {
  using T = double;
  const T two_pi = (T)6.283185307179586;
  const T den = V.x * V.x + V.y * V.y;
  const T re1 = eta - (V1.y * V.x - V1.x * V.y) / (den * two_pi);
  const cpx<T> D = cmul(Vt, V1) - cmul(Vt1, V);
  const cpx<T> num = cmul(V2, V) - cmul(V1, V1);
  const T inv_den = (T)1 / den;
  const cpx<T> r = {(Vt.x * V.x + Vt.y * V.y) * inv_den, (Vt.y * V.x - Vt.x * V.y) * inv_den};      // Vt / V
  const cpx<T> nr = cmul(num, r);
  const T dd = D.x * D.x + D.y * D.y;
  const T re2 = re1 - ((nr.y * D.x - nr.x * D.y) / dd) / two_pi;
  const bool second = hypot(D.x, D.y) > gamma * gamma && isfinite(re2);
  return hypot(V.x, V.y) > gamma ? fs * fabs(second ? re2 : re1) : (T)INFINITY;
}

// axis 1, first order: stft_tsst.hip's offset Re(Vt / V) in samples
template <typename O>
__device__ __forceinline__ double extract_delay1(double gamma, double half, cpx<double> V, cpx<double> Vt) {
  const double den = V.x * V.x + V.y * V.y;
  const double d1 = (Vt.x * V.x + Vt.y * V.y) / den;
  return hypot(V.x, V.y) > gamma ? clamp_keep_nan(d1, half) : (double)INFINITY;
}

// axis 1, second order: stft_tsst.hip's operator
template <typename O>
__device__ __forceinline__ double extract_delay2(double gamma, double half, cpx<double> V, cpx<double> V1,
                                                 cpx<double> V2, cpx<double> Vt, cpx<double> Vt1) {
  using T = double;
  const T den = V.x * V.x + V.y * V.y;
  const T d1 = (Vt.x * V.x + Vt.y * V.y) / den;
  const cpx<T> D = cmul(Vt, V1) - cmul(Vt1, V);
  const cpx<T> num = cmul(V2, V) - cmul(V1, V1);
  const cpx<T> a = cmul(V1, D), b = cmul(V, num);
  const T d2 = d1 + (a.x * b.x + a.y * b.y) / (b.x * b.x + b.y * b.y);     // Re(a / b)
  const bool second = hypot(num.x, num.y) > gamma * gamma && isfinite(d2) && fabs(d2) <= half;
  return hypot(V.x, V.y) > gamma ? clamp_keep_nan(second ? d2 : d1, half) : (T)INFINITY;
}

template <typename O, int LOGN, int ORDER>
__global__ __launch_bounds__(kFrameThreads) void extract_kernel(const ExtractDev<O> p) {
  using T = double;
  using C = FrameCfg<LOGN>;
  constexpr int N = C::N, L = C::L, FPR = C::FPR, ROW = C::ROW, F = C::F, TFS = C::TFS, SP = C::SP;
  constexpr bool MULTI = C::MULTI;
  __shared__ __attribute__((aligned(16))) cpx<T> exch_all[FPR * ROW];
  __shared__ __attribute__((aligned(16))) cpx<T> st_s[F * SP];
  __shared__ __attribute__((aligned(16))) cpx<T> st_m[F * SP];      // order 2: V1, then (w or offset or inf, -)

  const int tid = threadIdx.x;
  int g = tid / L;                                         // frame slot of the round
  const int t = tid % L;                                   // lane inside the frame
  if constexpr (L >= 64) g = __builtin_amdgcn_readfirstlane(g);        // one frame (or part of one) per wave: scalar
  cpx<T>* exch = exch_all + g * ROW;

  const long long nfr = p.n_frames;
  const int b = (int)blockIdx.y + p.b0;                                 // (an int, widened where it is used: one scalar held)
  constexpr int TILE = TFS * kFrameRoundsPerTile;                       // frame_grid's tile: the frames of a workgroup
  const int f_tile = (int)blockIdx.x * TILE;                            // frames fit an int: n_frames <= 2^30
  const int f_end = (long long)f_tile + TILE < nfr ? f_tile + TILE : (int)nfr;
  const T inv_n = (T)(1.0 / (double)N);

  for (int fr0 = f_tile; fr0 < f_end; fr0 += TFS) {                     // a round = a store tile: FPR frames side by side
    {
      const int f = fr0 + g;
      const bool valid = f < f_end;                                      // (a frame past the end transforms zeros)
      const long long pos0 = (long long)f * p.hop - N / 2;              // the larger half of the n - 1 pad samples on the left
      const T* __restrict__ xs = p.x + (long long)(b + opaque_zero()) * p.n_signal;   // (formed per round, not held)
      const bool interior = valid && pos0 >= 0 && pos0 + N <= p.n_signal;
      T xv[16];
      frame_samples<LOGN>(p, xs, pos0, t + opaque_zero(), valid, interior, reinterpret_cast<T*>(exch), xv);
      frame_sync<MULTI>();      // (an edge frame's samples went through the row: all read before the first exchange writes it)
      const int slot = g;
      cpx<T> v[16];
      if constexpr (ORDER == 1) {
        // one packed transform x (g + i w): w = g1 (axis 0) or tg (axis 1), p.h1 half its inverse level
        cpx<T> V[9], W[9];
        const int z = opaque_zero(), tz = t + z;
        const cpx<T>* __restrict__ wa = p.wa + z;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const cpx<T> w = wa[(tz + L * q + p.rot) & (N - 1)];
          v[q] = {xv[q] * w.x, xv[q] * w.y};
        }
        fft_pass_compact<T, LOGN, 0, MULTI>(v, exch, p.tw + z, tz);
        frame_split<T, LOGN, MULTI>(v, exch, tz, (T)0.5, p.h1, V, W);
        const ExtractOut<O>* __restrict__ pa = p.out + opaque_zero();   // (read where they are used, not held in scalars)
        const T gam = pa->gamma;
        if (pa->axis == 0) {
          const T fs = pa->fs;
#pragma unroll
          for (int q = 0; q < 9; ++q) {
            const int k = tz + L * q;
            if (k <= N / 2) {
              st_s[k * SP + slot] = V[q];
              st_m[k * SP + slot] = {extract_freq1<O>(gam, fs, (T)k * inv_n, V[q], W[q]), (T)0};
            }
          }
        } else {
#pragma unroll
          for (int q = 0; q < 9; ++q) {
            const int k = tz + L * q;
            if (k <= N / 2) {
              st_s[k * SP + slot] = V[q];
              st_m[k * SP + slot] = {extract_delay1<O>(gam, (T)(N / 2), V[q], W[q]), (T)0};
            }
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
        // all five spectra at hand: the axis picks the operator (the same branch in every lane of the grid)
        const int te = t + opaque_zero();
        const ExtractOut<O>* __restrict__ pa = p.out + opaque_zero();   // (read where they are used, not held in scalars)
        const T gam = pa->gamma;
        if (pa->axis == 0) {
          const T fs = pa->fs;
#pragma unroll
          for (int q = 0; q < 9; ++q) {
            const int k = te + L * q;
            if (k <= N / 2) {
              const cpx<T> V = st_s[k * SP + slot], V1 = st_m[k * SP + slot];
              st_m[k * SP + slot] = {extract_freq2<O>(gam, fs, (T)k * inv_n, V, V1, V2[q], Vt[q], Vt1[q]), (T)0};
            }
          }
        } else {
#pragma unroll
          for (int q = 0; q < 9; ++q) {
            const int k = te + L * q;
            if (k <= N / 2) {
              const cpx<T> V = st_s[k * SP + slot], V1 = st_m[k * SP + slot];
              st_m[k * SP + slot] = {extract_delay2<O>(gam, (T)(N / 2), V, V1, V2[q], Vt[q], Vt1[q]), (T)0};
            }
          }
        }
      }
    }
    __syncthreads();
    // the outputs' addresses are fetched and formed here, so that no pointer is held across the transforms
    const ExtractOut<O> po = p.out[opaque_zero()];
    const long long ob = (long long)b * F * nfr;
    cpx<O>* __restrict__ Te = po.Te + ob;
    cpx<O>* __restrict__ Sx = po.Sx ? po.Sx + ob : nullptr;
    O* __restrict__ map_out = po.map ? po.map + ob : nullptr;
    const bool freq = po.axis == 0;
    const int nft = f_end - fr0 < TFS ? f_end - fr0 : TFS;
    for (int e = tid; e < F * TFS; e += kFrameThreads) {                  // neighbouring lanes: neighbouring frames of a bin
      const int k = e / TFS, fl = e % TFS;
      if (fl < nft) {
        const long long o = (long long)k * nfr + fr0 + fl;
        const cpx<T> S = st_s[k * SP + fl];
        const cpx<O> So = {(O)S.x, (O)S.y};
        const T val = st_m[k * SP + fl].x;
        O mv = (O)INFINITY;
        bool keep = false;
        if (val != (T)INFINITY) {
          if (freq) {
            // stft_sst2.hip's bin rule on the frequency the call reports, in the call's dtype
            mv = (O)val;
            const O u = fmax(mv / po.unit, (O)0);                        // (w - Sfs[0]) / dw, Sfs[0] = 0
            int kk = (u >= (O)(F - 1)) ? F - 1 : (int)rint(u);
            if (!(u == u)) kk = 0;
            keep = kk == k;
          } else {
            // stft_tsst.hip's relative target on the tau the call reports, before its clip to the frame range
            mv = (O)(val / po.fs);
            keep = rint(mv / po.unit) == (O)0;
          }
        }
        Te[o] = keep ? So : cpx<O>{(O)0, (O)0};
        if (Sx) Sx[o] = So;
        if (map_out) map_out[o] = mv;
      }
    }
    __syncthreads();
  }
}

template <typename T>
static hipError_t extract_launch(ExtractDev<T> p, int logn, int order, long long batch, hipStream_t stream) {
  return dispatch_logn(logn, [&](auto ln) {
    constexpr int LOGN = decltype(ln)::value;
    dim3 grid;
    int tile_frames;                                       // (the kernel knows it: TFS kFrameRoundsPerTile)
    if (hipError_t e = frame_grid<LOGN>(p.n_frames, batch, &tile_frames, &grid); e != hipSuccess) return e;
    if (order == 1)
      hipLaunchKernelGGL((extract_kernel<T, LOGN, 1>), grid, dim3(kFrameThreads), 0, stream, p);
    else
      hipLaunchKernelGGL((extract_kernel<T, LOGN, 2>), grid, dim3(kFrameThreads), 0, stream, p);
    return hipGetLastError();
  });
}

}  // namespace ssq

using namespace ssq;

namespace {

const char* extract_own_fail(int axis, int order) {
  if (axis != 0 && axis != 1) return "axis must be 0 (frequency) or 1 (time)";
  return order == 1 || order == 2 ? nullptr : "order must be 1 or 2";
}

// The argument checks of the entry points, and the shape they work on (sets the error and returns non-zero)
int extract_shape(const char* own_fail, const FrameCall& c, int axis, ExtractShape* s) {
  if (int rc = frame_shape("extract_stft", true, own_fail, c, s)) return rc;
  s->order = c.order;
  s->axis = axis;
  const std::vector<double> sfs = host::np_linspace(0.0, 0.5 * c.fs, s->n_freqs);
  s->dw = sfs[1] - sfs[0];
  return 0;
}

// The workspace of `cap` signals: the widened signals of a float32 call, nothing for a float64 one.  The only place that
// knows the layout: the workspace_bytes, exec and host doors all go through it.
int64_t extract_work_bytes(int dtype, int64_t cap, int64_t n_signal) { return widened_bytes(dtype, cap, n_signal); }

// set_stft / tet_stft on device buffers (pipe_host, pipe_exec): the widening of a float32 call and ONE kernel
template <typename T>
struct ExtractPipe {
  static constexpr int kMid = 0;
  const FrameCall& c;
  const ExtractShape& s;
  DeviceBufs d;
  ExtractDev<T> p;
  double* xd;
  int tables() {
    const int64_t n = c.n_fft;
    const bool time1 = s.order == 1 && s.axis == 1;
    const host::SstTables t =
        host::sst_level_tables(c.window, n, s.order == 2 ? host::kSstSecond : (time1 ? host::kSstTimeFirst : host::kSstFirst));
    const std::vector<double> tw = host::pass_twiddles(s.logn);
    void *d_tw, *d_wa, *d_wb = nullptr, *d_wc = nullptr;
    SSQ_HIP(d.upload(&d_tw, tw.data(), sizeof(double) * tw.size()));
    SSQ_HIP(d.upload(&d_wa, t.wa.data(), sizeof(cpx<double>) * n));
    if (s.order == 2) {
      SSQ_HIP(d.upload(&d_wb, t.wb.data(), sizeof(double) * n));
      SSQ_HIP(d.upload(&d_wc, t.wc.data(), sizeof(cpx<double>) * n));
    }
    p = ExtractDev<T>{};
    p.tw = (const cpx<double>*)d_tw;
    p.wa = (const cpx<double>*)d_wa;
    p.wb = (const double*)d_wb;
    p.wc = (const cpx<double>*)d_wc;
    p.n_signal = c.n_signal;
    p.n_frames = s.n_frames;
    p.hop = (int)c.hop;
    p.padtype = c.padtype;
    p.rot = (c.variant & SSQ_VARIANT_MODULATED) ? (int)(n / 2) : 0;
    p.h1 = time1 ? t.it : t.h1;
    p.it = t.it;
    p.ht1 = t.ht1;
    p.h2 = t.h2;
    return 0;
  }
  int bind(int64_t, void* const* outs /* Te, Sx, map */, void* work) {
    xd = (double*)work;                                    // (a float64 call has no workspace: not read)
    ExtractOut<T> o{};
    o.Te = (cpx<T>*)outs[0];
    o.Sx = (cpx<T>*)outs[1];
    o.map = (T*)outs[2];
    o.fs = s.fs;
    o.gamma = s.gamma;
    o.axis = s.axis;
    o.unit = s.axis == 0 ? (T)s.dw : (T)((double)c.hop / s.fs);
    void* d_o;
    SSQ_HIP(d.upload(&d_o, &o, sizeof(o)));
    p.out = (const ExtractOut<T>*)d_o;
    return 0;
  }
  int run(int64_t nb, const void* d_x, const hipEvent_t*) {
    SSQ_HIP(frame_signals64((const T*)d_x, xd, (long long)nb * p.n_signal, nullptr, &p.x));
    SSQ_HIP(for_signal_runs(nb, [&](int64_t b0, int64_t n1) {
      p.b0 = (int)b0;
      return extract_launch<T>(p, s.logn, s.order, n1, nullptr);
    }));
    return 0;
  }
};

}  // namespace

extern "C" {

int ssq_extract_stft_host(int dtype, const void* x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                          int64_t hop, double fs, int padtype, int axis, int order, double gamma, int variant, void* Te,
                          void* Sx, void* map) {
  if (!x || !window || !Te) SSQ_FAIL("NULL argument");
  const FrameCall c{dtype, batch, n_signal, window, n_fft, hop, fs, padtype, gamma, variant, SSQ_SQUEEZE_SUM, order};
  ExtractShape s;
  if (int rc = extract_shape(extract_own_fail(axis, order), c, axis, &s)) return rc;
  if (int rc = require_device()) return rc;
  const size_t el = dtype == SSQ_F32 ? 4 : 8, map_el = (size_t)s.n_freqs * (size_t)s.n_frames * el;
  const HostOut outs[] = {{Te, 2 * map_el}, {Sx, 2 * map_el}, {map, map_el}};
  const size_t work = (size_t)extract_work_bytes(dtype, 1, n_signal);
  return dtype == SSQ_F32 ? pipe_host<ExtractPipe<float>>(c, s, x, el * (size_t)n_signal, outs, work)
                          : pipe_host<ExtractPipe<double>>(c, s, x, el * (size_t)n_signal, outs, work);
}

int64_t ssq_extract_stft_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t n_fft, int64_t hop) {
  ExtractShape s;
  if (extract_shape(nullptr, frame_sizes_call(dtype, batch, n_signal, n_fft, hop), 0, &s)) return -1;
  return extract_work_bytes(dtype, batch, n_signal);
}

int ssq_extract_stft_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                          int64_t hop, double fs, int padtype, int axis, int order, double gamma, int variant, void* d_Te,
                          void* d_Sx, void* d_map, void* d_workspace, int64_t workspace_bytes, float* kernel_ms) {
  if (!d_x || !window || !d_Te) SSQ_FAIL("NULL argument");
  const FrameCall c{dtype, batch, n_signal, window, n_fft, hop, fs, padtype, gamma, variant, SSQ_SQUEEZE_SUM, order};
  ExtractShape s;
  if (int rc = extract_shape(extract_own_fail(axis, order), c, axis, &s)) return rc;
  const int64_t need = extract_work_bytes(dtype, batch, n_signal);
  if (workspace_bytes < need) SSQ_FAIL("extract_stft: workspace smaller than ssq_extract_stft_workspace_bytes");
  if (need > 0 && !d_workspace) SSQ_FAIL("NULL argument");      // (a float64 call needs none: NULL and 0 bytes go together)
  if (int rc = require_device()) return rc;
  void* const outs[] = {d_Te, d_Sx, d_map};
  return dtype == SSQ_F32 ? pipe_exec<ExtractPipe<float>>(c, s, d_x, outs, d_workspace, kernel_ms)
                          : pipe_exec<ExtractPipe<double>>(c, s, d_x, outs, d_workspace, kernel_ms);
}

}  // extern "C"
