// istft_fused.h -- the streaming inverse STFT: plan and launch of istft_fused.hip.
#pragma once
#include "ssq_common.h"

namespace ssq {

constexpr int kIstftAcc = 5120;       // fp64 samples of a workgroup's overlap-add accumulator (40 KB of LDS)
constexpr int kIstftThreads = 256;
constexpr int kIstftMinTiles = 256;   // tiles per signal below which the three-kernel path is taken

// How a (n_fft, hop, n_frames) problem is cut: a workgroup owns `tf` consecutive frames (a tile), starts `halo` frames
// before them and walks all of them in chunks of `rf` frames; the accumulator holds one chunk, rf * hop + n - hop
// samples.  Nothing here depends on the batch size or on the device, so that a signal's bits do not depend on what it is
// batched with.
struct IstftPlan {
  int logn = 0;
  int n = 0, hop = 0, keep = 0;       // keep = n - hop: the unfinished samples a chunk hands to the next
  int halo = 0;                       // (n - 1) / hop: the frames before a tile that reach into its samples
  int fpr = 0;                        // frames transformed per round by the 256 lanes
  int rf = 0, tf = 0;
  long long n_frames = 0, tiles = 0;  // tiles per signal
  bool preferred = false;             // enough tiles per signal to beat the three-kernel path
};

// false: the kernel does not take this length / hop (pl->preferred: whether it should, for this many frames)
bool istft_fused_plan(long long n, long long hop, long long n_frames, IstftPlan* pl);

// d_Sx [batch][n/2+1][n_frames], d_x [batch][n_signal] (overwritten), d_tw [n] = exp(-2 pi i j / n), d_wpow, d_wnorm [n].
// batch <= 65535.
template <typename T>
hipError_t launch_istft_fused(const IstftPlan& pl, const cpx<T>* d_Sx, long long batch, long long n_signal, int modulated,
                              const cpx<T>* d_tw, const double* d_wpow, const double* d_wnorm, T* d_x,
                              hipStream_t stream);

}  // namespace ssq
