// stft_reassign.hip -- the reassigned spectrogram, `upstream.reassign_stft` (Kodera, Gendrin and de
// Villedary 1978; Auger and Flandrin 1995).  Upstream has no such transform: the definition is the project's own,
// restated in numpy by tests/helpers/reassign_ref.py.  Every bin's energy |Sx|^2 moves in BOTH directions at once, to its
// instantaneous frequency (ssq_stft2's first-order operator) and its group delay (tssq_stft's).  Per-sample units, fs
// enters at the end.  With n = n_fft, u[j] = j - n/2, the windows g, g1 = g' and tg = u g of stft_sst2.hip and V, V1, Vt
// the STFTs of x with them (frame m centred on sample m hop):
//   w   = fs |k/n - Im(V1/V) / (2 pi)|           fp64, rounded once to the call's dtype; +inf where |V| <= gamma
//   tau = clamp(Re(Vt/V), -n/2, n/2) / fs        fp64, rounded once to the call's dtype; +inf where |V| <= gamma
//   k'  = ssq_stft2's bin rule on the reported w (clamped round-half-even on np.linspace(0, fs/2, F))
//   m'  = clip(m + rint(tau / (hop/fs)), 0, n_frames - 1) in the call's dtype        |m' - m| <= H = ceil(n / (2 hop))
//   Rx[k', m'] += |Sx[k, m]|^2                   of the REPORTED Sx, formed in fp64
//
//   reassign_operator_kernel : stft_tsst.hip's frame ownership, loader, packed fp64 transforms, split and LDS transpose
//                              (the shared pieces are stft_frames64.h's): TWO
//                              transforms a frame, x (g + i g1) and x tg; both operators per bin; Sx, optionally w and tau,
//                              and one packed 4-byte target per bin (int16 r = m' - m, kReassignNone where the bin is not
//                              kept, above uint16 k') out along frames.  It also reduces max |Sx|^2 per signal: a
//                              block reduction, then ONE 64-bit integer atomic max per workgroup on the bit pattern of
//                              the non-negative double (order-independent).
//   reassign_scatter_kernel  : a workgroup owns ALL F target rows x a tile of T target frames, one 64-bit integer
//                              accumulator per cell in LDS.  It walks the packed targets of every row over the frames
//                              [t0 - H, t0 + T + H) along frames; a lane whose source lands in the tile loads that Sx,
//                              forms |Sx|^2 in fp64, converts it to fixed point (quantum q = P 2^-38, P the smallest
//                              power of two >= the signal's max |Sx|^2) and adds it with a 64-bit integer LDS atomic.
//                              Integer adds commute: a cell's bits do not depend on order, tiling or batch.  A cell takes
//                              at most (2 H + 1) F < 2^24 contributions of at most 2^38 quanta: no overflow of 63 bits.
//                              The read-out converts every cell once and writes every cell of Rx exactly once.
#include <cmath>
#include <vector>

#include "../../include/ssq_hip.h"
#include "dev_buffers.h"
#include "sst_tables.h"
#include "stft_frames64.h"

namespace ssq {

constexpr int kReassignNone = -32768;          // the relative time target of a bin that is not kept
constexpr int kReassignQuantumLog2 = -38;      // q = P 2^-38 (upstream.REASSIGN_QUANTUM_LOG2)
constexpr int kReassignScatterThreads = 1024;
constexpr int kReassignCells = 16384;          // 64-bit accumulators of one scatter workgroup: 128 KiB of the CU's 160
constexpr int kReassignMaxTile = 1024;         // target frames of one scatter workgroup at the small n_fft

// O: the dtype of the call (float or double: x in, Sx / w / tau / Rx out).  The transforms and the operators always run
// in fp64, on the widened signal, as in stft_sst2.hip and stft_tsst.hip.
// What the operator kernel needs only when it stores a tile.  It lives in device memory and is read there, behind an
// opaque offset: as kernel arguments these would sit in scalar registers across the transforms.
template <typename O>
struct ReassignOut {
  cpx<O>* Sx;                  // [batch][F][n_frames]
  O* w;                        // [batch][F][n_frames], or nullptr
  O* tau;                      // [batch][F][n_frames], or nullptr
  unsigned* tgt;               // [batch][F][n_frames]  (int16 m' - m or kReassignNone) << 16 | uint16 k'
  unsigned long long* emax;    // [batch]  bit pattern of max |Sx|^2, zeroed before the launch
  double fs;
  O step;                      // hop / fs in the call's dtype: the time rule runs on the tau the call reports
  O dw;                        // Sfs[1] - Sfs[0] in the call's dtype: the bin rule runs on the w the call reports
};

template <typename O>
struct ReassignDev {
  const double* x;             // [batch][n_signal], widened (widen_f64) for a float32 call
  const cpx<double>* tw;       // the passes' twiddle tables, passes 1, 2, .. back to back
  const cpx<double>* wa;       // (g, g1 a1)      a*: powers of two that level the channels
  const double* wb;            // tg at
  const ReassignOut<O>* out;
  long long n_signal, n_frames;
  int hop, padtype, rot, tile_frames, b0;   // b0: the signal of blockIdx.y = 0
  double gamma;
  double h1, it;               // 0.5 / a1, 1 / at
};

// both first-order operators of one bin, per sample: (|k/n - Im(V1/V)/(2 pi)|, clamp(Re(Vt/V))), or (inf, inf) where the
// bin is not kept
template <typename O>
__device__ __forceinline__ cpx<double> reassign_operator(const ReassignDev<O>& p, double eta, double half, cpx<double> V,
                                                         cpx<double> V1, cpx<double> Vt) {
  using T = double;
  const T two_pi = (T)6.283185307179586;
  const T den = V.x * V.x + V.y * V.y;
  const T re1 = eta - (V1.y * V.x - V1.x * V.y) / (den * two_pi);          // ssq_stft2's Re w1
  const T d1 = (Vt.x * V.x + Vt.y * V.y) / den;                            // tssq_stft's order-1 offset
  const bool keep = hypot(V.x, V.y) > p.gamma;
  return {keep ? fabs(re1) : (T)INFINITY, keep ? clamp_keep_nan(d1, half) : (T)INFINITY};
}

template <typename O, int LOGN>
__global__ __launch_bounds__(kFrameThreads) void reassign_operator_kernel(const ReassignDev<O> p) {
  using T = double;
  using C = FrameCfg<LOGN>;
  constexpr int N = C::N, L = C::L, FPR = C::FPR, ROW = C::ROW, F = C::F, TFS = C::TFS, SP = C::SP;
  constexpr bool MULTI = C::MULTI;
  __shared__ __attribute__((aligned(16))) cpx<T> exch_all[FPR * ROW];
  __shared__ __attribute__((aligned(16))) cpx<T> st_s[F * SP];
  __shared__ __attribute__((aligned(16))) cpx<T> st_m[F * SP];      // V1, then (|Re w1| or inf, offset or inf)
  __shared__ T mx_s[kFrameThreads];                              // every lane's own running max |Sx|^2

  const int tid = threadIdx.x;
  int g = tid / L;                                         // frame slot of the round
  const int t = tid % L;                                   // lane inside the frame
  if constexpr (L >= 64) g = __builtin_amdgcn_readfirstlane(g);        // one frame (or part of one) per wave: scalar
  cpx<T>* exch = exch_all + g * ROW;

  const long long nfr = p.n_frames;
  const long long b = (long long)blockIdx.y + p.b0;
  const int f_tile = (int)blockIdx.x * p.tile_frames;                   // frames fit an int: n_frames <= 2^30
  const int f_end = (long long)f_tile + p.tile_frames < nfr ? f_tile + p.tile_frames : (int)nfr;
  const T inv_n = (T)(1.0 / (double)N);
  mx_s[tid] = (T)0;                                                     // (the lane alone reads and writes its slot)

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
      // Two transforms, with stft_frames64.h's opaque offsets and stft_sst2.hip's scheduling barriers (the loop-invariant table loads stay
      // where they are used): (g, g1) first, V into the store tile and V1 parked in the lane's own map slots (the lane
      // reads back what it wrote: no ordering point); tg alone (real input: its spectrum is the transform itself).
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
        const T* __restrict__ wb = p.wb + z;
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = {xv[q] * wb[(tz + L * q + p.rot) & (N - 1)], (T)0};
        fft_pass_compact<T, LOGN, 0, MULTI>(v, exch, p.tw + z, tz);
      }
      __builtin_amdgcn_sched_barrier(0);
      const int te = t + opaque_zero();
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        const int k = te + L * q;
        if (k <= N / 2) {
          const cpx<T> V = st_s[k * SP + slot], V1 = st_m[k * SP + slot];
          st_m[k * SP + slot] = reassign_operator<O>(p, (T)k * inv_n, (T)(N / 2), V, V1, cscale(v[q], p.it));
        }
      }
    }
    __syncthreads();
    // the outputs' addresses are fetched and formed here, so that no pointer is held across the transforms
    const ReassignOut<O> po = p.out[opaque_zero()];
    const long long ob = b * (long long)F * nfr;
    cpx<O>* __restrict__ Sx = po.Sx + ob;
    O* __restrict__ w_out = po.w ? po.w + ob : nullptr;
    O* __restrict__ tau_out = po.tau ? po.tau + ob : nullptr;
    unsigned* __restrict__ tgt_out = po.tgt + ob;
    const int nft = f_end - fr0 < TFS ? f_end - fr0 : TFS;
    T mx = mx_s[tid];
    for (int e = tid; e < F * TFS; e += kFrameThreads) {              // neighbouring lanes: neighbouring frames of a bin
      const int k = e / TFS, fl = e % TFS;
      if (fl < nft) {
        const long long m = (long long)fr0 + fl, o = (long long)k * nfr + m;
        const cpx<T> S = st_s[k * SP + fl];
        const cpx<O> So = {(O)S.x, (O)S.y};
        Sx[o] = So;
        mx = fmax(mx, energy_f64<O>(So));
        const cpx<T> M = st_m[k * SP + fl];
        O w = (O)INFINITY, tau = (O)INFINITY;
        unsigned pk = (unsigned)(kReassignNone & 0xffff) << 16;
        if (M.x != (T)INFINITY) {
          w = (O)(po.fs * M.x);
          tau = (O)(M.y / po.fs);
          // ssq_stft2's bin rule on the reported w: (w - Sfs[0]) / dw with Sfs[0] = 0, clamped round-half-even
          const O vb = fmax(w / po.dw, (O)0);
          int kk = (vb >= (O)(F - 1)) ? F - 1 : (int)rint(vb);
          if (!(vb == vb)) kk = 0;
          // tssq_stft's time rule on the reported tau.  |r| <= ceil(n / (2 hop)), the offset being clamped; the bound
          // below only keeps a quotient of denormals (an fs next to the dtype's smallest number) inside an int16
          const O vt = tau / po.step;
          const O rv = isfinite(vt) ? rint(vt) : (O)0;
          const long long r = (long long)(rv < (O)-4096 ? (O)-4096 : (rv > (O)4096 ? (O)4096 : rv));
          long long mt = m + r;
          mt = mt < 0 ? 0 : (mt > nfr - 1 ? nfr - 1 : mt);
          pk = ((unsigned)((int)(mt - m) & 0xffff) << 16) | (unsigned)kk;       // |m' - m| <= 4096: an int16, never kReassignNone
        }
        if (w_out) w_out[o] = w;
        if (tau_out) tau_out[o] = tau;
        tgt_out[o] = pk;
      }
    }
    mx_s[tid] = mx;
    __syncthreads();
  }
  // max |Sx|^2 of the workgroup's bins, then one integer atomic max on the bit pattern (non-negative doubles order as
  // their bit patterns do; max is order-independent)
  for (int s = kFrameThreads / 2; s > 0; s >>= 1) {
    if (tid < s) mx_s[tid] = fmax(mx_s[tid], mx_s[tid + s]);
    __syncthreads();
  }
  if (tid == 0) {
    const ReassignOut<O> po = p.out[opaque_zero()];
    atomicMax(po.emax + b, (unsigned long long)__double_as_longlong(mx_s[0]));
  }
}

template <typename O>
struct ReassignScat {
  const cpx<O>* Sx;                  // [batch][F][n_frames]
  const unsigned* tgt;               // [batch][F][n_frames]
  const unsigned long long* emax;    // [batch]
  O* Rx;                             // [batch][F][n_frames]
  long long n_frames;
  int n_freqs, reach, tile;          // reach = H; n_freqs * tile <= kReassignCells
};

template <typename O>
__global__ __launch_bounds__(kReassignScatterThreads) void reassign_scatter_kernel(const ReassignScat<O> p) {
  extern __shared__ __align__(16) unsigned long long reassign_cells[];   // [F][T]
  const long long nfr = p.n_frames;
  const int F = p.n_freqs, T = p.tile, tid = threadIdx.x;
  const long long base = (long long)blockIdx.y * F * nfr;
  const long long t0 = (long long)blockIdx.x * T;                        // the targets [t0, t1) x all rows are this workgroup's
  const long long t1 = t0 + T < nfr ? t0 + T : nfr;
  const long long s0 = t0 - p.reach > 0 ? t0 - p.reach : 0;              // the source frames [s0, s1) can reach them
  const long long s1 = t1 + p.reach < nfr ? t1 + p.reach : nfr;
  const int W = (int)(s1 - s0), TW = (int)(t1 - t0);
  for (int i = tid; i < F * T; i += kReassignScatterThreads) reassign_cells[i] = 0ull;
  // the signal's scale: P = the smallest power of two >= max |Sx|^2, quantum q = P 2^-38 (exponent clamped so that both
  // q and 1 / q are normal numbers; a signal of zeros, or one whose energy is not finite, gets q = 0)
  const double mx = __longlong_as_double((long long)p.emax[blockIdx.y]);
  double q = 0.0, inv_q = 0.0;
  if (mx > 0.0 && mx <= 1.7976931348623157e308) {
    int ex;
    const double fr = frexp(mx, &ex);                                    // mx = fr 2^ex, fr in [0.5, 1)
    int lp = fr == 0.5 ? ex - 1 : ex;
    lp = lp < -960 ? -960 : (lp > 960 ? 960 : lp);
    q = ldexp(1.0, lp + kReassignQuantumLog2);
    inv_q = ldexp(1.0, -lp - kReassignQuantumLog2);
  }
  __syncthreads();
  {
    int k = tid / W, i = tid % W;                                        // the walk (k, i) += 1024 without a division
    const int dk = kReassignScatterThreads / W, di = kReassignScatterThreads % W;
    while (k < F) {
      const long long o = base + (long long)k * nfr + s0 + i;
      const unsigned pk = p.tgt[o];
      const int r = (int)pk >> 16;                                       // the int16 above, sign-extended
      const long long mt = s0 + i + r;
      const int kk = (int)(pk & 0xffffu);
      if (r != kReassignNone && mt >= t0 && mt < t1 && kk < F) {
        const double e = fmin(energy_f64<O>(p.Sx[o]) * inv_q, 274877906944.0);      // <= 2^38 quanta
        atomicAdd(&reassign_cells[kk * T + (int)(mt - t0)], (unsigned long long)to_fixed_f64(e));
      }
      k += dk;
      i += di;
      if (i >= W) {
        i -= W;
        ++k;
      }
    }
  }
  __syncthreads();
  {
    int k = tid / TW, j = tid % TW;
    const int dk = kReassignScatterThreads / TW, dj = kReassignScatterThreads % TW;
    while (k < F) {
      p.Rx[base + (long long)k * nfr + t0 + j] = (O)((double)(long long)reassign_cells[k * T + j] * q);
      k += dk;
      j += dj;
      if (j >= TW) {
        j -= TW;
        ++k;
      }
    }
  }
}

template <typename T>
static hipError_t reassign_launch(ReassignDev<T> p, int logn, long long batch, hipStream_t stream) {
  return dispatch_logn(logn, [&](auto ln) {
    constexpr int LOGN = decltype(ln)::value;
    dim3 grid;
    if (hipError_t e = frame_grid<LOGN>(p.n_frames, batch, &p.tile_frames, &grid); e != hipSuccess) return e;
    hipLaunchKernelGGL((reassign_operator_kernel<T, LOGN>), grid, dim3(kFrameThreads), 0, stream, p);
    return hipGetLastError();
  });
}

}  // namespace ssq

using namespace ssq;

namespace {

struct ReassignShape : FrameShape {
  int tile = 1;
  double dw = 0.0;
};

// The argument checks of the three entry points, and the shape they work on (sets the error and returns non-zero)
int reassign_shape(const FrameCall& c, ReassignShape* s) {
  if (int rc = frame_shape("reassign_stft", true, nullptr, c, s)) return rc;
  // target frames of a scatter workgroup: what kReassignCells accumulators hold of all F rows (1024 ... 7)
  int64_t tile = kReassignCells / s->n_freqs;
  if (tile > kReassignMaxTile) tile = kReassignMaxTile;
  if (tile > s->n_frames) tile = s->n_frames;
  s->tile = (int)tile;
  const std::vector<double> sfs = host::np_linspace(0.0, 0.5 * c.fs, s->n_freqs);
  s->dw = sfs[1] - sfs[0];
  return 0;
}

// The workspace of `cap` signals, as byte offsets: (float32 calls) the widened signals, the signals' maxima, the packed
// targets.  The only place that knows the layout: the workspace_bytes, exec and host doors all go through it.
struct ReassignWork {
  int64_t xd, emax, tgt, bytes;
};
ReassignWork reassign_work(int dtype, int64_t cap, int64_t n_signal, const FrameShape& s) {
  const int64_t xd_b = widened_bytes(dtype, cap, n_signal);
  return {0, xd_b, xd_b + 8 * cap, xd_b + 8 * cap + 4 * cap * s.n_freqs * s.n_frames};
}

// the call's tables on the device (held by `d`) and the two parameter blocks without their signal / output pointers
template <typename T>
int reassign_tables(DeviceBufs& d, const ReassignShape& s, const FrameCall& c, ReassignDev<T>* p, ReassignScat<T>* sc) {
  const int64_t n = c.n_fft;
  const host::SstTables t = host::sst_level_tables(c.window, n, host::kSstFirst);
  const std::vector<double> tw = host::pass_twiddles(s.logn);
  void *d_tw, *d_wa, *d_wb;
  SSQ_HIP(d.upload(&d_tw, tw.data(), sizeof(double) * tw.size()));
  SSQ_HIP(d.upload(&d_wa, t.wa.data(), sizeof(cpx<double>) * n));
  SSQ_HIP(d.upload(&d_wb, t.wb.data(), sizeof(double) * n));
  *p = ReassignDev<T>{};
  p->tw = (const cpx<double>*)d_tw;
  p->wa = (const cpx<double>*)d_wa;
  p->wb = (const double*)d_wb;
  p->n_signal = c.n_signal;
  p->n_frames = s.n_frames;
  p->hop = (int)c.hop;
  p->padtype = c.padtype;
  p->rot = (c.variant & SSQ_VARIANT_MODULATED) ? (int)(n / 2) : 0;
  p->gamma = s.gamma;
  p->h1 = t.h1;
  p->it = t.it;
  *sc = ReassignScat<T>{};
  sc->n_frames = s.n_frames;
  sc->n_freqs = (int)s.n_freqs;
  sc->reach = s.reach;
  sc->tile = s.tile;
  return 0;
}

// the operator kernel's output block (ReassignOut) on the device, held by `d`
template <typename T>
int reassign_out_block(DeviceBufs& d, const ReassignShape& s, int64_t hop, void* d_Sx, void* d_w, void* d_tau, void* d_tgt,
                       void* d_emax, ReassignDev<T>* p) {
  ReassignOut<T> o{};
  o.Sx = (cpx<T>*)d_Sx;
  o.w = (T*)d_w;
  o.tau = (T*)d_tau;
  o.tgt = (unsigned*)d_tgt;
  o.emax = (unsigned long long*)d_emax;
  o.fs = s.fs;
  o.step = (T)((double)hop / s.fs);
  o.dw = (T)s.dw;
  void* d_o;
  SSQ_HIP(d.upload(&d_o, &o, sizeof(o)));
  p->out = (const ReassignOut<T>*)d_o;
  return 0;
}

// both kernels of `nb` signals on device buffers; ev (may be nullptr): an event recorded between the two
template <typename T>
hipError_t reassign_run(ReassignDev<T> p, ReassignScat<T> sc, const ReassignShape& s, const T* d_x, int64_t nb, T* d_Rx,
                        cpx<T>* d_Sx, unsigned* d_tgt, unsigned long long* d_emax,
                        double* d_xd /* float32 calls: [nb][n_signal] */, hipEvent_t ev) {
  const size_t map_sig = (size_t)s.n_freqs * (size_t)s.n_frames;
  hipError_t e = hipMemsetAsync(d_emax, 0, sizeof(unsigned long long) * (size_t)nb, nullptr);
  if (e != hipSuccess) return e;
  if ((e = frame_signals64(d_x, d_xd, (long long)nb * p.n_signal, nullptr, &p.x)) != hipSuccess) return e;
  e = for_signal_runs(nb, [&](int64_t b0, int64_t n1) {
    p.b0 = (int)b0;
    return reassign_launch<T>(p, s.logn, n1, nullptr);
  });
  if (e != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev, nullptr)) != hipSuccess) return e;
  const long long tiles = (s.n_frames + s.tile - 1) / s.tile;
  const size_t lds = sizeof(unsigned long long) * (size_t)s.n_freqs * (size_t)s.tile;    // <= 8 kReassignCells
  if ((e = hipFuncSetAttribute((const void*)reassign_scatter_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds)) != hipSuccess)
    return e;
  return for_signal_runs(nb, [&](int64_t b0, int64_t n1) {
    sc.Sx = d_Sx + map_sig * b0;
    sc.tgt = d_tgt + map_sig * b0;
    sc.emax = d_emax + b0;
    sc.Rx = d_Rx + map_sig * b0;
    hipLaunchKernelGGL(reassign_scatter_kernel<T>, dim3((unsigned)tiles, (unsigned)n1), dim3(kReassignScatterThreads), lds,
                       nullptr, sc);
    return hipGetLastError();
  });
}

// reassign_stft on device buffers (pipe_host, pipe_exec).  kernel_ms: two parts, the event recorded between the operator
// and the scatter.
template <typename T>
struct ReassignPipe {
  static constexpr int kMid = 1;
  const FrameCall& c;
  const ReassignShape& s;
  DeviceBufs d;
  ReassignDev<T> p;
  ReassignScat<T> sc;
  T* Rx;
  cpx<T>* Sx;
  unsigned* tgt;
  unsigned long long* emax;
  double* xd;
  int tables() { return reassign_tables<T>(d, s, c, &p, &sc); }
  int bind(int64_t cap, void* const* outs /* Rx, Sx, w, tau */, void* work) {
    const ReassignWork k = reassign_work(c.dtype, cap, c.n_signal, s);
    Rx = (T*)outs[0];
    Sx = (cpx<T>*)outs[1];
    xd = (double*)((char*)work + k.xd);
    emax = (unsigned long long*)((char*)work + k.emax);
    tgt = (unsigned*)((char*)work + k.tgt);
    return reassign_out_block<T>(d, s, c.hop, Sx, outs[2], outs[3], tgt, emax, &p);
  }
  int run(int64_t nb, const void* d_x, const hipEvent_t* mid) {
    SSQ_HIP(reassign_run<T>(p, sc, s, (const T*)d_x, nb, Rx, Sx, tgt, emax, xd, mid[0]));
    return 0;
  }
};

}  // namespace

extern "C" {

int ssq_reassign_stft_host(int dtype, const void* x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                           int64_t hop, double fs, int padtype, double gamma, int variant, void* Rx, void* Sx, void* w,
                           void* tau) {
  if (!x || !window || !Rx || !Sx) SSQ_FAIL("NULL argument");
  const FrameCall c{dtype, batch, n_signal, window, n_fft, hop, fs, padtype, gamma, variant};
  ReassignShape s;
  if (int rc = reassign_shape(c, &s)) return rc;
  if (int rc = require_device()) return rc;
  const size_t el = dtype == SSQ_F32 ? 4 : 8, map_el = (size_t)s.n_freqs * (size_t)s.n_frames * el;
  const HostOut outs[] = {{Rx, map_el}, {Sx, 2 * map_el}, {w, map_el}, {tau, map_el}};
  const size_t work = (size_t)reassign_work(dtype, 1, n_signal, s).bytes;
  return dtype == SSQ_F32 ? pipe_host<ReassignPipe<float>>(c, s, x, el * (size_t)n_signal, outs, work)
                          : pipe_host<ReassignPipe<double>>(c, s, x, el * (size_t)n_signal, outs, work);
}

int64_t ssq_reassign_stft_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t n_fft, int64_t hop) {
  ReassignShape s;
  if (reassign_shape(frame_sizes_call(dtype, batch, n_signal, n_fft, hop), &s)) return -1;
  return reassign_work(dtype, batch, n_signal, s).bytes;
}

int ssq_reassign_stft_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                           int64_t hop, double fs, int padtype, double gamma, int variant, void* d_Rx, void* d_Sx,
                           void* d_w, void* d_tau, void* d_workspace, int64_t workspace_bytes, float* kernel_ms) {
  if (!d_x || !window || !d_Rx || !d_Sx || !d_workspace) SSQ_FAIL("NULL argument");
  const FrameCall c{dtype, batch, n_signal, window, n_fft, hop, fs, padtype, gamma, variant};
  ReassignShape s;
  if (int rc = reassign_shape(c, &s)) return rc;
  if (workspace_bytes < reassign_work(dtype, batch, n_signal, s).bytes)
    SSQ_FAIL("reassign_stft: workspace smaller than ssq_reassign_stft_workspace_bytes");
  if (int rc = require_device()) return rc;
  void* const outs[] = {d_Rx, d_Sx, d_w, d_tau};
  return dtype == SSQ_F32 ? pipe_exec<ReassignPipe<float>>(c, s, d_x, outs, d_workspace, kernel_ms)
                          : pipe_exec<ReassignPipe<double>>(c, s, d_x, outs, d_workspace, kernel_ms);
}

}  // extern "C"
