// stft_frames64.h -- the fp64 frame pipeline that the operator kernels of stft_sst2.hip, stft_tsst.hip and
// stft_reassign.hip share: a workgroup of 256 lanes owns a tile of consecutive frames of one signal, a
// frame is held by n/16 lanes, 256/(n/16) frames side by side (fft_core.h; frames of 2048 points and more span several
// waves).  Here: the per-length configuration, the sample loader, the split of a packed pair of real-input spectra, the
// float32 -> fp64 widening of the signals (frame_signals64: the fp64 signals of a slice of either dtype), the dispatch on
// the transform length, the loop over runs of at most 65535 signals a launch (for_signal_runs), and the call struct,
// argument checks and shape the entry points have in common.  The kernels' own bodies (their transforms in order,
// operators and read-outs) stay in their files: what is here compiles to the same machine code in each of them.
#pragma once
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ssq_hip.h"
#include "fft_core.h"
#include "stft_kernels.h"

namespace ssq {

constexpr int kFrameThreads = 256;
constexpr int kFrameRoundsPerTile = 4;     // store tiles one workgroup of an operator kernel walks

// frames per round = per store tile (and the tile's padded pitch in the LDS stage) of one transform length
template <int LOGN>
struct FrameCfg {
  static constexpr int N = 1 << LOGN, L = N / 16, FPR = kFrameThreads / L, ROW = N + N / 16, F = N / 2 + 1;
  static constexpr bool MULTI = L > 64;
  static constexpr int TFS = FPR, SP = TFS >= 8 ? TFS + 1 : TFS;
};

// A zero the compiler cannot see through.  The tables of the transforms are loop invariant: an opaque zero offset per
// transform keeps their loads (and the twiddles') where they are used instead of in ~100 registers across the frame
// loop; added to the lane index it does the same for the LDS and table addresses built on it (another ~90 registers when
// hoisted).  The operator kernels sit at the 256-register limit.
__device__ __forceinline__ int opaque_zero() {
  int z;
  asm volatile("s_mov_b32 %0, 0" : "=s"(z));
  return z;
}

// The 16 samples of a lane: transform input t + L q is frame sample j (rotated by n/2 when modulated).  A frame inside
// the signal reads them directly.  An edge frame goes through the pad index map in a ROLLED loop, one sample at a time
// through the lane's own slots of the frame's idle exchange row (the lane reads back what it wrote: no ordering point):
// unrolled, the sixteen 64-bit index chains of the five pad types were the kernel's register peak.
// P: the kernel's parameter block (rot, n_signal, padtype).
template <int LOGN, typename P>
__device__ __forceinline__ void frame_samples(const P& p, const double* __restrict__ xs, long long pos0, int t, bool valid,
                                              bool interior, double* row, double (&xv)[16]) {
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
__device__ __forceinline__ void frame_split(const cpx<T> (&v)[16], cpx<T>* exch, int t, T h_a, T h_b, cpx<T> (&A)[9],
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

// the signals of a float32 call in fp64: the transforms and the operators run on these
template <typename I>
__global__ void widen_f64_kernel(const I* __restrict__ in, double* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (double)in[i];
}
inline hipError_t widen_f64(const float* d_in, double* d_out, long long n, hipStream_t stream) {
  hipLaunchKernelGGL(widen_f64_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_in, d_out, n);
  return hipGetLastError();
}

// *x64: the `count` samples at d_x in fp64 for the operator kernels: a float32 slice widened into d_xd on `stream`, a
// float64 slice as it is (d_xd is not read)
template <typename T>
hipError_t frame_signals64(const T* d_x, double* d_xd, long long count, hipStream_t stream, const double** x64) {
  if constexpr (sizeof(T) == 4) {
    *x64 = d_xd;
    return widen_f64(d_x, d_xd, count, stream);
  } else {
    *x64 = d_x;
    return hipSuccess;
  }
}

// f(b0, n1) on the runs of at most 65535 signals that make up `nb` (a grid's y and z end there: DESIGN 4.10.1), up to the
// first error
template <typename F>
hipError_t for_signal_runs(int64_t nb, F&& f) {
  for (int64_t b0 = 0; b0 < nb; b0 += 65535)
    if (hipError_t e = f(b0, nb - b0 < 65535 ? nb - b0 : (int64_t)65535); e != hipSuccess) return e;
  return hipSuccess;
}

// f(std::integral_constant<int, LOGN>) for the transform length 2^logn, 16 to 4096 points
template <typename F>
hipError_t dispatch_logn(int logn, F&& f) {
  switch (logn) {
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 9: return f(std::integral_constant<int, 9>{});
    case 10: return f(std::integral_constant<int, 10>{});
    case 11: return f(std::integral_constant<int, 11>{});
    case 12: return f(std::integral_constant<int, 12>{});
  }
  return hipErrorInvalidValue;
}

// the grid of an operator kernel over `batch` signals (at most 65535 a launch) and the frames a workgroup owns
template <int LOGN>
hipError_t frame_grid(long long n_frames, long long batch, int* tile_frames, dim3* grid) {
  *tile_frames = FrameCfg<LOGN>::TFS * kFrameRoundsPerTile;
  const long long tiles = (n_frames + *tile_frames - 1) / *tile_frames;
  if (tiles > 0x7fffffffLL || batch > 65535) return hipErrorInvalidValue;
  *grid = dim3((unsigned)tiles, (unsigned)batch);
  return hipSuccess;
}

struct FrameShape {
  int logn = 0, reach = 1;             // reach: H = ceil(n / (2 hop)), how far a clamped group delay moves a coefficient
  int64_t n_freqs = 0, n_frames = 0;
  double fs = 1.0, gamma = 0.0;
};

// The argument checks that the entry points of the three transforms share, in their order, and the shape they work on
// (sets the error and returns non-zero).  name: the entry point's prefix of the messages.  strict: a NaN gamma and a hop
// that does not fit an int are errors (tssq_stft, reassign_stft; ssq_stft2 accepts both).  own_fail: the message of the
// entry point's own argument check (squeezing, order), or nullptr where it passed; it is reported in its place.
inline int frame_shape(const char* name, bool strict, const char* own_fail, int dtype, int64_t batch, int64_t n_signal,
                       int64_t n_fft, int64_t hop, double fs, int padtype, double gamma, FrameShape* s) {
  const std::string pre = std::string(name) + ": ";
  if (dtype != SSQ_F32 && dtype != SSQ_F64) SSQ_FAIL("dtype must be SSQ_F32 or SSQ_F64");
  if (batch < 1) SSQ_FAIL("batch must be >= 1");
  if (n_fft < 16 || n_fft > 4096 || (n_fft & (n_fft - 1)) != 0) SSQ_FAIL(pre + "n_fft must be a power of two from 16 to 4096");
  if (n_signal < 1 || hop < 1) SSQ_FAIL(pre + "n_signal and hop must be >= 1");
  if (strict && hop > 0x7fffffffLL) SSQ_FAIL(pre + "hop does not fit an int");
  if (padtype < SSQ_PAD_REFLECT || padtype > 4) SSQ_FAIL(pre + "unknown padtype");
  if (own_fail) SSQ_FAIL(pre + own_fail);
  if (strict && gamma != gamma) SSQ_FAIL(pre + "gamma is NaN");
  if (!(fs > 0) || !std::isfinite(fs)) SSQ_FAIL(pre + "fs must be positive");
  s->logn = 0;
  while ((1LL << s->logn) < n_fft) ++s->logn;
  s->n_freqs = n_fft / 2 + 1;
  s->n_frames = (n_signal - 1) / hop + 1;
  if (s->n_frames > (1LL << 30)) SSQ_FAIL(pre + "too many frames");
  s->reach = (int)((n_fft / 2 - 1) / hop + 1);               // <= 2048
  s->fs = fs;
  s->gamma = gamma < 0 ? 10.0 * (dtype == SSQ_F64 ? 2.2204460492503131e-16 : 1.1920928955078125e-07) : gamma;
  return 0;
}

// The arguments of an entry point of the family as it received them (ssq_stft2, tssq_stft, reassign_stft, mssq_stft,
// tmssq_stft); a field the transform does not have keeps its default.
struct FrameCall {
  int dtype;
  int64_t batch, n_signal;
  const double* window;
  int64_t n_fft, hop;
  double fs;
  int padtype;
  double gamma;
  int variant;
  int squeezing = SSQ_SQUEEZE_SUM, order = 2, n_iter = 1;
};

// the call ssq_*_workspace_bytes checks its sizes with
inline FrameCall frame_sizes_call(int dtype, int64_t batch, int64_t n_signal, int64_t n_fft, int64_t hop) {
  return FrameCall{dtype, batch, n_signal, nullptr, n_fft, hop, 1.0, SSQ_PAD_REFLECT, -1.0, 0};
}

inline int frame_shape(const char* name, bool strict, const char* own_fail, const FrameCall& c, FrameShape* s) {
  return frame_shape(name, strict, own_fail, c.dtype, c.batch, c.n_signal, c.n_fft, c.hop, c.fs, c.padtype, c.gamma, s);
}

// bytes of the fp64 copy of `cap` signals that a float32 call widens into (a float64 call has none)
inline int64_t widened_bytes(int dtype, int64_t cap, int64_t n_signal) { return dtype == SSQ_F32 ? 8 * cap * n_signal : 0; }

// ssq_freqs (may be nullptr) of the linear grid `sfs`, reversed under SSQ_VARIANT_FLIPUD
inline void fill_ssq_freqs(double* ssq_freqs, const std::vector<double>& sfs, int variant) {
  if (!ssq_freqs) return;
  const size_t n = sfs.size();
  for (size_t i = 0; i < n; ++i) ssq_freqs[i] = (variant & SSQ_VARIANT_FLIPUD) ? sfs[n - 1 - i] : sfs[i];
}

}  // namespace ssq
