// stft_sst2.h -- what stft_sst2.hip lends to stft_msst.hip: the parameter block of sst2_operator_kernel,
// the argument checks and the shape, the workspace layout, the call's tables on the device, and the two halves of the pipeline (operator,
// rows-ascending scatter) on device buffers.  The kernels and the host code are compiled once, in stft_sst2.hip, for
// float and double; this header only declares them.
#pragma once
#include <cstdint>
#include <vector>

#include "dev_buffers.h"
#include "stft_frames64.h"

namespace ssq {

// O: the dtype of the call (float or double: x in, Sx / map / Tx / w2 out).  The transforms and the operator always run
// in fp64: the operator is a quotient of two differences of products, and with fp32 transforms of 1024 points and more
// over one strong bin in a thousand lands in another bin than the fp64 result.
template <typename O>
struct Sst2Dev {
  const double* x;         // [batch][n_signal], widened (widen_f64) for a float32 call
  const cpx<double>* tw;   // the passes' twiddle tables [m][k] = exp(-2 pi i k m / (NS R)), passes 1, 2, .. back to back
  const cpx<double>* wa;   // (g, g1 a1)          by frame sample j; a*: powers of two that level the channels
  const double* wb;        // tg at
  const cpx<double>* wc;   // (tg1 at1, g2 a2)
  cpx<O>* Sx;              // [batch][F][n_frames]
  cpx<O>* map;             // [batch][F][n_frames]  (w2 or inf, bin or -1)
  long long n_signal, n_frames;
  int hop, pad_left, padtype, rot, flip, tile_frames;
  double gamma, gamma_sq, fs;   // gamma_sq: the second-order estimate is used where |D| > gamma_sq (ssq_stft2: gamma^2;
                                // +inf, mssq_stft's order 1: nowhere, so every bin reports fs |Re w1|)
  O dw;                    // Sfs[1] - Sfs[0] in the call's dtype: the bin rule runs on the w2 the call reports
  double h1, it, ht1, h2;  // 0.5 / a1, 1 / at, 0.5 / at1, 0.5 / a2
};

struct Sst2Shape : FrameShape {
  double dw = 0.0;
  std::vector<double> sfs;
};

// The argument checks of the entry points, and the shape they work on (sets the error and returns non-zero).  name: the
// entry point's prefix of the messages; own_fail: the message of its own argument check that failed, or nullptr.
int sst2_shape(const char* name, const char* own_fail, const FrameCall& c, Sst2Shape* s);

// The workspace of `cap` signals of ssq_stft2 and mssq_stft, as byte offsets: the packed map, then (float32 calls) the
// widened signals.  The only place that knows the layout: the workspace_bytes, exec and host doors all go through it.
struct Sst2Work {
  int64_t map, xd, bytes;
};
inline Sst2Work sst2_work(int dtype, int64_t cap, int64_t n_signal, const FrameShape& s) {
  const int64_t map_b = (int64_t)(dtype == SSQ_F32 ? 8 : 16) * cap * s.n_freqs * s.n_frames;
  return {0, map_b, map_b + widened_bytes(dtype, cap, n_signal)};
}

// the call's tables on the device (held by `d`) and the parameter block without its signal / output pointers
template <typename T>
int sst2_tables(DeviceBufs& d, const Sst2Shape& s, const FrameCall& c, Sst2Dev<T>* p);

// the operator kernel of `nb` signals on device buffers: Sx and the packed map (d_xd: float32 calls, [nb][n_signal])
template <typename T>
hipError_t sst2_operator_run(Sst2Dev<T> p, const Sst2Shape& s, const T* d_x, int64_t nb, cpx<T>* d_Sx, cpx<T>* d_map,
                             double* d_xd);

// Tx zeroed, then the rows-ascending scatter of Sx under the map's bin field; d_w (may be nullptr) receives its w field
template <typename T>
hipError_t sst2_scatter_run(const Sst2Shape& s, int squeezing, T dw, int64_t nb, const cpx<T>* d_Sx, const cpx<T>* d_map,
                            cpx<T>* d_Tx, T* d_w);

}  // namespace ssq
