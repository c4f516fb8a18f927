// stft_lmsst.hip -- local maximum synchrosqueezed STFT, `upstream.lmssq_stft` (Yu, Wang, Zhao and Liu 2019).
// Upstream has no such transform: the definition is the project's own, restated in numpy by tests/helpers/lmsst_ref.py.
// Where the rest of the family moves a coefficient to the frequency a quotient of STFTs estimates, this moves it to the
// row where |Sx| is largest inside a window of +- delta rows: no g', tg or g'', ONE transform, with the window alone.
// Per column, with F = n_fft/2 + 1 rows:
//   A[k] = re^2 + im^2 of the coefficient as the call reports it (rounded to the call's dtype), evaluated in fp64, the
//          two products and the sum rounded one by one (no fused multiply-add: numpy's re*re + im*im bit for bit)
//   m[k] = the row of the maximum of A over max(0, k - delta) .. min(F - 1, k + delta), scanned ascending and taken only
//          where strictly greater: the lowest row wins a tie; rows that are not kept take part in the window
//   Tx[r(m[k])] += Sx[k] dw ('sum') or dw / F ('lebesgue') for the kept k (|V| > gamma on the fp64 coefficient), rows
//          ascending, in the call's dtype;   r(b) = F - 1 - b under flipud, else b
// Everything is decided inside one column, which the frame kernel holds in LDS: ONE launch, no map plane in device
// memory, no clearing of Tx and no scatter kernel.
//
//   lmsst_kernel : stft_extract.hip's frame ownership and LDS layout (the shared pieces are stft_frames64.h's): 256 lanes
//                  own a tile of consecutive frames, n/16 lanes a frame.  One real-input fp64 transform x g; V goes into
//                  the store tile and A into the plane extract_kernel uses for its map.  After a barrier every cell
//                  scans its 2 delta + 1 rows of A in LDS (a direct scan: DESIGN 4.25 has why) and leaves m, or -1
//                  where the cell is not kept, beside A.  After another barrier Tx is formed in GATHER form: the cell
//                  of target b sums the rows k in b - delta .. b + delta with m[k] == b, ascending -- the order of the
//                  rows-ascending scatter -- so every cell of Tx is written exactly once.  Tx, Sx and the bins leave
//                  through the LDS transpose: global stores run along frames.
#include <cmath>
#include <vector>

#include "../../include/ssq_hip.h"
#include "dev_buffers.h"
#include "host_math.h"
#include "sst_tables.h"
#include "stft_frames64.h"

namespace ssq {

constexpr int kLmsstMaxDelta = 256;       // a bound on work (the scan reads 2 delta + 1 rows a cell), not a measured number

// What the kernel needs only after the transform.  It lives in device memory and is read there, behind an opaque
// offset, as stft_extract.hip's ExtractOut is.
template <typename O>
struct LmsstOut {
  cpx<O>* Tx;              // [batch][F][n_frames]
  cpx<O>* Sx;              // [batch][F][n_frames]
  int* bins;               // [batch][F][n_frames], or nullptr: the row of Tx a coefficient went to, -1 where not kept
  double gamma;            // a cell is kept where |V| > gamma
  O dw, leb;               // Sfs[1] - Sfs[0], and dw / F, in the call's dtype
  int delta, flip, squeezing;
};

template <typename O>
struct LmsstDev {
  const double* x;         // [batch][n_signal], widened (widen_f64) for a float32 call
  const cpx<double>* tw;   // the passes' twiddle tables, passes 1, 2, .. back to back
  const double* wg;        // the sized window g by frame sample
  const LmsstOut<O>* out;
  long long n_signal, n_frames;
  int hop, padtype, rot, b0;   // b0: the signal of blockIdx.y = 0
};

struct LmsstShape : FrameShape {
  int delta = 1;
  double dw = 0.0;
  std::vector<double> sfs;
};

// re^2 + im^2 with the products and the sum rounded one by one
__device__ __forceinline__ double lmsst_energy(double re, double im) {
#pragma clang fp contract(off)
  const double a = re * re;
  const double b = im * im;
  return a + b;
}

// The row of the maximum of A over lo .. hi (lo <= hi), A(r) the value of row r: ascending, strictly greater only
template <typename Load>
__device__ __forceinline__ int lmsst_argmax(int lo, int hi, Load&& A) {
  double best = A(lo);
  int mb = lo;
  for (int r = lo + 1; r <= hi; ++r) {
    const double a = A(r);
    if (a > best) {
      best = a;
      mb = r;
    }
  }
  return mb;
}

template <typename O, int LOGN>
__global__ __launch_bounds__(kFrameThreads) void lmsst_kernel(const LmsstDev<O> p) {
  using T = double;
  using C = FrameCfg<LOGN>;
  constexpr int N = C::N, L = C::L, FPR = C::FPR, ROW = C::ROW, F = C::F, TFS = C::TFS, SP = C::SP;
  constexpr bool MULTI = C::MULTI;
  __shared__ __attribute__((aligned(16))) cpx<T> exch_all[FPR * ROW];
  __shared__ __attribute__((aligned(16))) cpx<T> st_s[F * SP];
  __shared__ __attribute__((aligned(16))) cpx<T> st_m[F * SP];      // (A, m or -1)

  const int tid = threadIdx.x;
  int g = tid / L;                                         // frame slot of the round
  const int t = tid % L;                                   // lane inside the frame
  if constexpr (L >= 64) g = __builtin_amdgcn_readfirstlane(g);        // one frame (or part of one) per wave: scalar
  cpx<T>* exch = exch_all + g * ROW;

  const long long nfr = p.n_frames;
  const int b = (int)blockIdx.y + p.b0;
  constexpr int TILE = TFS * kFrameRoundsPerTile;                       // frame_grid's tile: the frames of a workgroup
  const int f_tile = (int)blockIdx.x * TILE;                            // frames fit an int: n_frames <= 2^30
  const int f_end = (long long)f_tile + TILE < nfr ? f_tile + TILE : (int)nfr;

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
      const int z = opaque_zero(), tz = t + z;
      const T* __restrict__ wg = p.wg + z;                               // real input: its spectrum is the transform itself
#pragma unroll
      for (int q = 0; q < 16; ++q) v[q] = {xv[q] * wg[(tz + L * q + p.rot) & (N - 1)], (T)0};
      fft_pass_compact<T, LOGN, 0, MULTI>(v, exch, p.tw + z, tz);
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        const int k = tz + L * q;
        if (k <= N / 2) {
          st_s[k * SP + slot] = v[q];
          st_m[k * SP + slot] = {lmsst_energy((T)(O)v[q].x, (T)(O)v[q].y), (T)-1};
        }
      }
    }
    __syncthreads();
    const LmsstOut<O> po = p.out[opaque_zero()];
    const int nft = f_end - fr0 < TFS ? f_end - fr0 : TFS;
    // m: every cell scans its window of A (neighbouring lanes: neighbouring frames of a row, or with one frame a round
    // neighbouring rows: no bank conflict either way)
    for (int e = tid; e < F * TFS; e += kFrameThreads) {
      const int k = e / TFS, fl = e % TFS;
      if (fl < nft) {
        const cpx<T> S = st_s[k * SP + fl];
        if (hypot(S.x, S.y) > po.gamma) {
          const int lo = k - po.delta < 0 ? 0 : k - po.delta, hi = k + po.delta > F - 1 ? F - 1 : k + po.delta;
          st_m[k * SP + fl].y = (T)lmsst_argmax(lo, hi, [&](int r) { return st_m[r * SP + fl].x; });
        }
      }
    }
    __syncthreads();
    // the outputs' addresses are formed here, so that no pointer is held across the transform
    const long long ob = (long long)b * F * nfr;
    cpx<O>* __restrict__ Tx = po.Tx + ob;
    cpx<O>* __restrict__ Sx = po.Sx + ob;
    int* __restrict__ bins = po.bins ? po.bins + ob : nullptr;
    for (int e = tid; e < F * TFS; e += kFrameThreads) {                  // neighbouring lanes: neighbouring frames of a bin
      const int k = e / TFS, fl = e % TFS;
      if (fl < nft) {
        const int lo = k - po.delta < 0 ? 0 : k - po.delta, hi = k + po.delta > F - 1 ? F - 1 : k + po.delta;
        cpx<O> acc = {(O)0, (O)0};
        for (int r = lo; r <= hi; ++r) {                                  // the rows that name this cell, ascending
          if (st_m[r * SP + fl].y == (T)k) {
            if (po.squeezing == SSQ_SQUEEZE_LEBESGUE) {
              acc.x += po.leb;
            } else {
              const cpx<T> S = st_s[r * SP + fl];
              acc.x += (O)S.x * po.dw;
              acc.y += (O)S.y * po.dw;
            }
          }
        }
        const long long col = fr0 + fl;
        Tx[(long long)(po.flip ? F - 1 - k : k) * nfr + col] = acc;
        const long long o = (long long)k * nfr + col;
        const cpx<T> S = st_s[k * SP + fl];
        Sx[o] = {(O)S.x, (O)S.y};
        if (bins) {
          const int m = (int)st_m[k * SP + fl].y;
          bins[o] = m < 0 ? -1 : (po.flip ? F - 1 - m : m);
        }
      }
    }
    __syncthreads();
  }
}

template <typename T>
static hipError_t lmsst_launch(LmsstDev<T> p, int logn, long long batch, hipStream_t stream) {
  return dispatch_logn(logn, [&](auto ln) {
    constexpr int LOGN = decltype(ln)::value;
    dim3 grid;
    int tile_frames;                                       // (the kernel knows it: TFS kFrameRoundsPerTile)
    if (hipError_t e = frame_grid<LOGN>(p.n_frames, batch, &tile_frames, &grid); e != hipSuccess) return e;
    hipLaunchKernelGGL((lmsst_kernel<T, LOGN>), grid, dim3(kFrameThreads), 0, stream, p);
    return hipGetLastError();
  });
}

}  // namespace ssq

using namespace ssq;

namespace {

// The argument checks of the entry points, and the shape they work on (sets the error and returns non-zero).
// delta < 0: not checked (the workspace does not depend on it).
int lmsst_shape(const FrameCall& c, int delta, LmsstShape* s) {
  const char* own_fail = nullptr;
  if (c.squeezing != SSQ_SQUEEZE_SUM && c.squeezing != SSQ_SQUEEZE_LEBESGUE) own_fail = "squeezing must be 'sum' or 'lebesgue'";
  if (int rc = frame_shape("lmssq_stft", false, own_fail, c, s)) return rc;
  const int64_t top = s->n_freqs - 1 < kLmsstMaxDelta ? s->n_freqs - 1 : (int64_t)kLmsstMaxDelta;
  if (delta >= 0 && (delta < 1 || delta > top)) SSQ_FAIL("lmssq_stft: delta must be from 1 to min(n_fft / 2, 256)");
  s->delta = delta;
  s->sfs = host::np_linspace(0.0, 0.5 * c.fs, s->n_freqs);
  s->dw = s->sfs[1] - s->sfs[0];
  return 0;
}

// The workspace of `cap` signals: the widened signals of a float32 call, nothing for a float64 one.  The only place that
// knows the layout: the workspace_bytes, exec and host doors all go through it.
int64_t lmsst_work_bytes(int dtype, int64_t cap, int64_t n_signal) { return widened_bytes(dtype, cap, n_signal); }

// lmssq_stft on device buffers (pipe_host, pipe_exec): the widening of a float32 call and ONE kernel
template <typename T>
struct LmsstPipe {
  static constexpr int kMid = 0;
  const FrameCall& c;
  const LmsstShape& s;
  DeviceBufs d;
  LmsstDev<T> p;
  double* xd;
  int tables() {
    const std::vector<double> tw = host::pass_twiddles(s.logn);
    void *d_tw, *d_wg;
    SSQ_HIP(d.upload(&d_tw, tw.data(), sizeof(double) * tw.size()));
    SSQ_HIP(d.upload(&d_wg, c.window, sizeof(double) * (size_t)c.n_fft));
    p = LmsstDev<T>{};
    p.tw = (const cpx<double>*)d_tw;
    p.wg = (const double*)d_wg;
    p.n_signal = c.n_signal;
    p.n_frames = s.n_frames;
    p.hop = (int)c.hop;
    p.padtype = c.padtype;
    p.rot = (c.variant & SSQ_VARIANT_MODULATED) ? (int)(c.n_fft / 2) : 0;
    return 0;
  }
  int bind(int64_t, void* const* outs /* Tx, Sx, bins */, void* work) {
    xd = (double*)work;                                    // (a float64 call has no workspace: not read)
    LmsstOut<T> o{};
    o.Tx = (cpx<T>*)outs[0];
    o.Sx = (cpx<T>*)outs[1];
    o.bins = (int*)outs[2];
    o.gamma = s.gamma;
    o.dw = (T)s.dw;
    o.leb = (T)((T)s.dw / (T)s.n_freqs);
    o.delta = s.delta;
    o.flip = (c.variant & SSQ_VARIANT_FLIPUD) ? 1 : 0;
    o.squeezing = c.squeezing;
    void* d_o;
    SSQ_HIP(d.upload(&d_o, &o, sizeof(o)));
    p.out = (const LmsstOut<T>*)d_o;
    return 0;
  }
  int run(int64_t nb, const void* d_x, const hipEvent_t*) {
    SSQ_HIP(frame_signals64((const T*)d_x, xd, (long long)nb * p.n_signal, nullptr, &p.x));
    SSQ_HIP(for_signal_runs(nb, [&](int64_t b0, int64_t n1) {
      p.b0 = (int)b0;
      return lmsst_launch<T>(p, s.logn, n1, nullptr);
    }));
    return 0;
  }
};

}  // namespace

extern "C" {

int ssq_lmssq_stft_host(int dtype, const void* x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                        int64_t hop, double fs, int padtype, int squeezing, double gamma, int variant, int delta, void* Tx,
                        double* ssq_freqs, void* Sx, int32_t* bins) {
  if (!x || !window || !Tx || !Sx) SSQ_FAIL("NULL argument");
  if (delta < 0) delta = 0;                                 // (only the workspace query leaves delta unchecked)
  const FrameCall c{dtype, batch, n_signal, window, n_fft, hop, fs, padtype, gamma, variant, squeezing};
  LmsstShape s;
  if (int rc = lmsst_shape(c, delta, &s)) return rc;
  fill_ssq_freqs(ssq_freqs, s.sfs, variant);
  if (int rc = require_device()) return rc;
  const size_t el = dtype == SSQ_F32 ? 4 : 8, map_sig = (size_t)s.n_freqs * (size_t)s.n_frames;
  const HostOut outs[] = {{Tx, 2 * el * map_sig}, {Sx, 2 * el * map_sig}, {bins, sizeof(int32_t) * map_sig}};
  const size_t work = (size_t)lmsst_work_bytes(dtype, 1, n_signal);
  return dtype == SSQ_F32 ? pipe_host<LmsstPipe<float>>(c, s, x, el * (size_t)n_signal, outs, work)
                          : pipe_host<LmsstPipe<double>>(c, s, x, el * (size_t)n_signal, outs, work);
}

int64_t ssq_lmssq_stft_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t n_fft, int64_t hop) {
  LmsstShape s;
  if (lmsst_shape(frame_sizes_call(dtype, batch, n_signal, n_fft, hop), -1, &s)) return -1;
  return lmsst_work_bytes(dtype, batch, n_signal);
}

int ssq_lmssq_stft_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                        int64_t hop, double fs, int padtype, int squeezing, double gamma, int variant, int delta, void* d_Tx,
                        void* d_Sx, int32_t* d_bins, void* d_workspace, int64_t workspace_bytes, float* kernel_ms) {
  if (!d_x || !window || !d_Tx || !d_Sx) SSQ_FAIL("NULL argument");
  if (delta < 0) delta = 0;
  const FrameCall c{dtype, batch, n_signal, window, n_fft, hop, fs, padtype, gamma, variant, squeezing};
  LmsstShape s;
  if (int rc = lmsst_shape(c, delta, &s)) return rc;
  const int64_t need = lmsst_work_bytes(dtype, batch, n_signal);
  if (workspace_bytes < need) SSQ_FAIL("lmssq_stft: workspace smaller than ssq_lmssq_stft_workspace_bytes");
  if (need > 0 && !d_workspace) SSQ_FAIL("NULL argument");      // (a float64 call needs none: NULL and 0 bytes go together)
  if (int rc = require_device()) return rc;
  void* const outs[] = {d_Tx, d_Sx, d_bins};
  return dtype == SSQ_F32 ? pipe_exec<LmsstPipe<float>>(c, s, d_x, outs, d_workspace, kernel_ms)
                          : pipe_exec<LmsstPipe<double>>(c, s, d_x, outs, d_workspace, kernel_ms);
}

}  // extern "C"
