// stft_tsst.h -- what stft_tsst.hip lends to stft_tmsst.hip: the parameter blocks of its two kernels, the
// argument checks and the shape, the workspace layout, the call's tables on the device, and the two halves of the pipeline (operator, time
// scatter) on device buffers.  The kernels and the host code are compiled once, in stft_tsst.hip, for float and double;
// this header only declares them.
#pragma once
#include <cstdint>

#include "dev_buffers.h"
#include "stft_frames64.h"

namespace ssq {

constexpr int kTsstThreads = 256;          // the scatter kernel's workgroup
constexpr int kTsstNone = -32768;          // the relative target of a bin that is not kept
constexpr int kTsstMaxReach = 2048;        // H at n_fft = 4096, hop 1
constexpr int kTsstMaxTile = 4096;         // target frames of one scatter workgroup
constexpr int kTsstStage = kTsstMaxTile + 2 * kTsstMaxReach;
constexpr int kTsstWideReach = 16384;      // the reach of a walked map, n_iter H (tmssq_stft; an int16 holds it)
constexpr int kTsstWideStage = kTsstMaxTile + 2 * kTsstWideReach;     // 72 KB of the CU's 160 KB

// O: the dtype of the call (float or double: x in, Sx / tau / Tx out).  The transforms and the operator always run in
// fp64, on the widened signal, as in stft_sst2.hip.
// What the operator kernel needs only when it stores a tile.  It lives in device memory and is read there, behind an
// opaque offset: as kernel arguments these would sit in scalar registers across the transforms, which are at the limit.
template <typename O>
struct TsstOut {
  cpx<O>* Sx;              // [batch][F][n_frames]
  O* tau;                  // [batch][F][n_frames], or nullptr
  short* rel;              // [batch][F][n_frames]  m' - m, or kTsstNone
  double fs;
  O step;                  // hop / fs in the call's dtype: the target rule runs on the tau the call reports
};

template <typename O>
struct TsstDev {
  const double* x;         // [batch][n_signal], widened (widen_f64) for a float32 call
  const cpx<double>* tw;   // the passes' twiddle tables, passes 1, 2, .. back to back
  const cpx<double>* wa;   // order 2: (g, g1 a1); order 1: (g, tg at)      a*: powers of two that level the channels
  const double* wb;        // order 2: tg at
  const cpx<double>* wc;   // order 2: (tg1 at1, g2 a2)
  const TsstOut<O>* out;
  long long n_signal, n_frames;
  int hop, padtype, rot, tile_frames, b0;   // b0: the signal of blockIdx.y = 0
  double gamma, gamma_sq;
  double h1, it, ht1, h2;  // 0.5 / a1, 1 / at (order 1: 0.5 / at), 0.5 / at1, 0.5 / a2
};

template <typename O>
struct TsstScat {
  const cpx<O>* Sx;        // [batch][F][n_frames]
  const short* rel;        // [batch][F][n_frames]
  const cpx<double>* rot;  // [n]  exp(-2 pi i j / n)
  cpx<O>* Tx;              // [batch][F][n_frames]
  long long n_frames;
  int n_freqs, n, hop, reach, tile;    // tile + 2 reach <= the kernel's stage; tile <= kTsstMaxTile, a multiple of 256
};

struct TsstShape : FrameShape {
  int order = 2, tile = 1024;
};

// target frames of one workgroup for sources within `reach` frames: halo re-read (tile + 2 reach) / tile <= 2 while the
// tile is below kTsstMaxTile
inline int tsst_tile(long long reach) {
  if (2 * reach < 1024) return 1024;
  return 2 * reach >= kTsstMaxTile ? kTsstMaxTile : (int)((2 * reach + 255) / 256 * 256);
}

// The argument checks of the entry points, and the shape they work on (sets the error and returns non-zero).  name: the
// entry point's prefix of the messages; own_fail: the message of its own argument check that failed, or nullptr.
int tsst_shape(const char* name, const char* own_fail, const FrameCall& c, TsstShape* s);

// The workspace of `cap` signals of tssq_stft and (walked) tmssq_stft, as byte offsets: (float32 calls) the widened
// signals, the one-step int16 targets, then tmssq_stft's walked ones.  The only place that knows the layout: the
// workspace_bytes, exec and host doors all go through it.
struct TsstWork {
  int64_t xd, rel, rel2, bytes;
};
inline TsstWork tsst_work(int dtype, int64_t cap, int64_t n_signal, const FrameShape& s, bool walked) {
  const int64_t xd_b = widened_bytes(dtype, cap, n_signal), rel_b = 2 * cap * s.n_freqs * s.n_frames;
  return {0, xd_b, xd_b + rel_b, xd_b + (walked ? 2 : 1) * rel_b};
}

// the call's tables on the device (held by `d`) and the two parameter blocks without their signal / output pointers
template <typename T>
int tsst_tables(DeviceBufs& d, const TsstShape& s, const FrameCall& c, TsstDev<T>* p, TsstScat<T>* sc);

// the operator kernel's output block (TsstOut) on the device, held by `d`
template <typename T>
int tsst_out_block(DeviceBufs& d, const TsstShape& s, int64_t hop, void* d_Sx, void* d_tau, void* d_rel, TsstDev<T>* p);

// the operator kernel of `nb` signals on device buffers: Sx, tau and the relative targets named by p.out (d_xd: float32
// calls, [nb][n_signal])
template <typename T>
hipError_t tsst_operator_run(TsstDev<T> p, const TsstShape& s, const T* d_x, int64_t nb, double* d_xd);

// The time scatter of Sx under the relative targets d_rel, sources within sc.reach frames of a cell, sc.tile cells a
// workgroup (every cell of Tx is written).  trim: a workgroup walks only as far as the largest |target| it staged (the
// same sums); tssq_stft runs without.
template <typename T>
hipError_t tsst_scatter_run(TsstScat<T> sc, const TsstShape& s, int64_t nb, const cpx<T>* d_Sx, const short* d_rel,
                            cpx<T>* d_Tx, bool trim);

}  // namespace ssq
