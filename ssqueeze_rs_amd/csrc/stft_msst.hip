// stft_msst.hip -- multisynchrosqueezed STFT, `upstream.mssq_stft` (Yu, Wang and Zhao 2019).  Upstream has no
// such transform: the definition is the project's own, restated in numpy by tests/helpers/msst_ref.py.  Per column, with
// F = n_fft/2 + 1 rows and m[k] the one-step bin of row k (ssq_stft2's rule on the frequency the call reports, before any
// flip; -1 where |V| <= gamma; order 2: ssq_stft2's w2 with its fallback, order 1: fs |Re w1|):
//   c1[k] = m[k];   c(i+1)[k] = m[ci[k]] if ci[k] >= 0 and m[ci[k]] >= 0, else ci[k]      (i = 1 .. n_iter - 1)
//   Tx[r(c_n[k])] += Sx[k] dw ('sum') or dw / F ('lebesgue'), kept rows ascending;   r(b) = F - 1 - b under flipud, else b
// A coefficient still moves along frequency only and keeps its phase: every column keeps its sum.
//
//   sst2_operator_kernel : stft_sst2.hip's, unflipped, with gamma_sq = +inf for order 1 (|D| > gamma_sq nowhere, so every
//                          bin reports fs |Re w1|; the same three transforms run): Sx and the packed map (w, one-step
//                          bin or -1).
//   msst_walk_kernel     : a workgroup owns a tile of C consecutive columns of one signal and all rows.  It loads the
//                          tile's bins once, along columns, into LDS as 16-bit values (0xffff: no map), and after one
//                          barrier every thread walks its elements n_iter - 1 steps in LDS (the tile is read-only: no
//                          barrier between steps; a chain ends early on a fixed point or a missing map).  The final bin,
//                          flipped if asked, goes back into the map's bin field along columns: tiles are
//                          column-disjoint and a workgroup holds its whole tile before it writes, so in place is safe.
//                          Chasing m through global memory instead would touch up to 64 cache lines per wave-load.
//   sst2_scatter_kernel  : stft_sst2.hip's rows-ascending scatter, on the final map.
#include <cmath>
#include <vector>

#include "../../include/ssq_hip.h"
#include "dev_buffers.h"
#include "msst_tile.h"
#include "stft_sst2.h"

namespace ssq {

// (the tile's constants and walk_log_cols: msst_tile.h, shared with cwt_msst.hip)
// map: [batch][n_rows][n_cols] packed (w, bin or -1); only the bin field is read and written.  bins_out (may be nullptr):
// the final bins as int32, same shape.  n_rows << log_c <= kWalkTileWords.
template <typename T>
__global__ __launch_bounds__(kWalkThreads) void msst_walk_kernel(cpx<T>* __restrict__ map, int* __restrict__ bins_out,
                                                                 int n_rows, long long n_cols, int log_c, int n_iter,
                                                                 int flip) {
  __shared__ unsigned short tile[kWalkTileWords];
  const int cmask = (1 << log_c) - 1;
  const long long col0 = (long long)blockIdx.x << log_c;
  const long long left = n_cols - col0;
  const int nc = left < (long long)(cmask + 1) ? (int)left : cmask + 1;                 // the last tile of a signal is narrower
  const long long base = (long long)blockIdx.y * n_rows * n_cols + col0;
  const int n_el = n_rows << log_c;
  for (int e = threadIdx.x; e < n_el; e += kWalkThreads) {      // neighbouring lanes: neighbouring columns of a row
    const int r = e >> log_c, c = e & cmask;
    unsigned v = kWalkNoMap;
    if (c < nc) {
      const T b = map[base + (long long)r * n_cols + c].y;
      if (b >= (T)0 && b < (T)n_rows) v = (unsigned)(int)b;     // (a target outside the rows counts as no map)
    }
    tile[e] = (unsigned short)v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n_el; e += kWalkThreads) {
    const int r = e >> log_c, c = e & cmask;
    if (c >= nc) continue;
    const unsigned first = tile[e];
    unsigned cur = first;
    if (cur != kWalkNoMap) {
      for (int i = 1; i < n_iter; ++i) {
        const unsigned nx = tile[(cur << log_c) + c];
        if (nx == kWalkNoMap || nx == cur) break;               // no map of its own, or a fixed point: the chain stops
        cur = nx;
      }
    }
    const int out = cur == kWalkNoMap ? -1 : (flip ? n_rows - 1 - (int)cur : (int)cur);
    const long long o = base + (long long)r * n_cols + c;
    if (flip || cur != first) map[o].y = (T)out;                // (a chain that stayed on its one-step bin: nothing to write)
    if (bins_out) bins_out[o] = out;
  }
}

// the walk of `nb` maps on device buffers
template <typename T>
hipError_t msst_walk_run(cpx<T>* d_map, int* d_bins, int64_t nb, int n_rows, long long n_cols, int n_iter, int flip) {
  const int log_c = walk_log_cols(n_rows);
  const long long tiles = (n_cols + (1LL << log_c) - 1) >> log_c;
  if (n_rows < 1 || n_rows > kWalkMaxRows || tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t map_sig = (size_t)n_rows * (size_t)n_cols;
  for (int64_t b0 = 0; b0 < nb; b0 += 65535) {
    const int64_t n1 = nb - b0 < 65535 ? nb - b0 : 65535;
    hipLaunchKernelGGL(msst_walk_kernel<T>, dim3((unsigned)tiles, (unsigned)n1), dim3(kWalkThreads), 0, nullptr,
                       d_map + map_sig * b0, d_bins ? d_bins + map_sig * b0 : (int*)nullptr, n_rows, n_cols, log_c, n_iter,
                       flip);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace ssq

using namespace ssq;

namespace {

const char* msst_own_fail(int order, int n_iter) {
  if (order != 1 && order != 2) return "order must be 1 or 2";
  if (n_iter < 1 || n_iter > kWalkMaxIter) return "n_iter must be from 1 to 64";
  return nullptr;
}

// mssq_stft on device buffers (pipe_host, pipe_exec), in ssq_stft2's workspace (sst2_work): the operator, the walk, the
// scatter.  kernel_ms: three parts, the events recorded after the operator and after the walk.
template <typename T>
struct MsstPipe {
  static constexpr int kMid = 2;
  const FrameCall& c;
  const Sst2Shape& s;
  DeviceBufs d;
  Sst2Dev<T> p;
  cpx<T>*Tx, *Sx, *map;
  T* w;
  int* bins;
  double* xd;
  // the operator runs unflipped (the walk indexes rows by bin); the flip is applied when the final bin is written
  int tables() {
    FrameCall u = c;
    u.variant &= ~SSQ_VARIANT_FLIPUD;
    if (int rc = sst2_tables<T>(d, s, u, &p)) return rc;
    if (c.order == 1) p.gamma_sq = INFINITY;                 // |D| > gamma_sq nowhere: the operator reports fs |Re w1|
    return 0;
  }
  int bind(int64_t cap, void* const* outs /* Tx, Sx, w, bins */, void* work) {
    const Sst2Work k = sst2_work(c.dtype, cap, c.n_signal, s);
    Tx = (cpx<T>*)outs[0];
    Sx = (cpx<T>*)outs[1];
    w = (T*)outs[2];
    bins = (int*)outs[3];
    map = (cpx<T>*)((char*)work + k.map);
    xd = (double*)((char*)work + k.xd);
    return 0;
  }
  int run(int64_t nb, const void* d_x, const hipEvent_t* mid) {
    SSQ_HIP(sst2_operator_run<T>(p, s, (const T*)d_x, nb, Sx, map, xd));
    if (mid[0]) SSQ_HIP(hipEventRecord(mid[0], nullptr));
    const int flip = (c.variant & SSQ_VARIANT_FLIPUD) ? 1 : 0;
    if (c.n_iter > 1 || flip || bins)                        // (one step, unflipped, no bins asked for: the map is final)
      SSQ_HIP(msst_walk_run<T>(map, bins, nb, (int)s.n_freqs, (long long)s.n_frames, c.n_iter, flip));
    if (mid[1]) SSQ_HIP(hipEventRecord(mid[1], nullptr));
    SSQ_HIP(sst2_scatter_run<T>(s, c.squeezing, p.dw, nb, Sx, map, Tx, w));
    return 0;
  }
};

}  // namespace

extern "C" {

int ssq_mssq_stft_host(int dtype, const void* x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                       int64_t hop, double fs, int padtype, int squeezing, double gamma, int variant, int order, int n_iter,
                       void* Tx, double* ssq_freqs, void* Sx, void* w, int32_t* bins) {
  if (!x || !window || !Tx || !Sx) SSQ_FAIL("NULL argument");
  const FrameCall c{dtype, batch, n_signal, window, n_fft, hop, fs, padtype, gamma, variant, squeezing, order, n_iter};
  Sst2Shape s;
  if (int rc = sst2_shape("mssq_stft", msst_own_fail(order, n_iter), c, &s)) return rc;
  fill_ssq_freqs(ssq_freqs, s.sfs, variant);
  if (int rc = require_device()) return rc;
  const size_t el = dtype == SSQ_F32 ? 4 : 8, map_sig = (size_t)s.n_freqs * (size_t)s.n_frames;
  const HostOut outs[] = {{Tx, 2 * el * map_sig}, {Sx, 2 * el * map_sig}, {w, el * map_sig}, {bins, sizeof(int32_t) * map_sig}};
  const size_t work = (size_t)sst2_work(dtype, 1, n_signal, s).bytes;
  return dtype == SSQ_F32 ? pipe_host<MsstPipe<float>>(c, s, x, el * (size_t)n_signal, outs, work)
                          : pipe_host<MsstPipe<double>>(c, s, x, el * (size_t)n_signal, outs, work);
}

int64_t ssq_mssq_stft_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t n_fft, int64_t hop) {
  Sst2Shape s;
  if (sst2_shape("mssq_stft", nullptr, frame_sizes_call(dtype, batch, n_signal, n_fft, hop), &s)) return -1;
  return sst2_work(dtype, batch, n_signal, s).bytes;
}

int ssq_mssq_stft_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                       int64_t hop, double fs, int padtype, int squeezing, double gamma, int variant, int order, int n_iter,
                       void* d_Tx, void* d_Sx, void* d_w, int32_t* d_bins, void* d_workspace, int64_t workspace_bytes,
                       float* kernel_ms) {
  if (!d_x || !window || !d_Tx || !d_Sx || !d_workspace) SSQ_FAIL("NULL argument");
  const FrameCall c{dtype, batch, n_signal, window, n_fft, hop, fs, padtype, gamma, variant, squeezing, order, n_iter};
  Sst2Shape s;
  if (int rc = sst2_shape("mssq_stft", msst_own_fail(order, n_iter), c, &s)) return rc;
  if (workspace_bytes < sst2_work(dtype, batch, n_signal, s).bytes)
    SSQ_FAIL("mssq_stft: workspace smaller than ssq_mssq_stft_workspace_bytes");
  if (int rc = require_device()) return rc;
  void* const outs[] = {d_Tx, d_Sx, d_w, d_bins};
  return dtype == SSQ_F32 ? pipe_exec<MsstPipe<float>>(c, s, d_x, outs, d_workspace, kernel_ms)
                          : pipe_exec<MsstPipe<double>>(c, s, d_x, outs, d_workspace, kernel_ms);
}

int ssq_msst_tile_cols(int64_t n_rows) {
  if (n_rows < 1 || n_rows > kWalkMaxRows) {
    set_error("msst_walk: n_rows must be from 1 to 2049");
    return -1;
  }
  return 1 << walk_log_cols((int)n_rows);
}

int ssq_msst_walk_host(const int32_t* bins_in, int64_t batch, int64_t n_rows, int64_t n_cols, int n_iter, int32_t* bins_out) {
  if (!bins_in || !bins_out) SSQ_FAIL("NULL argument");
  if (batch < 1) SSQ_FAIL("batch must be >= 1");
  if (n_rows < 1 || n_rows > kWalkMaxRows) SSQ_FAIL("msst_walk: n_rows must be from 1 to 2049");
  if (n_cols < 1 || n_cols > (1LL << 30)) SSQ_FAIL("msst_walk: n_cols must be from 1 to 2^30");
  if (n_iter < 1 || n_iter > kWalkMaxIter) SSQ_FAIL("msst_walk: n_iter must be from 1 to 64");
  const size_t map_sig = (size_t)n_rows * (size_t)n_cols;
  for (size_t i = 0; i < map_sig * (size_t)batch; ++i)
    if (bins_in[i] < -1 || bins_in[i] >= n_rows) SSQ_FAIL("msst_walk: a target lies outside -1 .. n_rows - 1");
  if (int rc = require_device()) return rc;
  // the kernel's format is the packed map of a float32 call, (w, bin): packing to and from it is host plumbing
  DeviceBufs d;
  const int64_t slice = slice_signals(batch, (double)map_sig * (sizeof(cpx<float>) + sizeof(int32_t)), 0.0, batch);
  void *d_map, *d_bins;
  SSQ_HIP(d.alloc(&d_map, sizeof(cpx<float>) * map_sig * slice));
  SSQ_HIP(d.alloc(&d_bins, sizeof(int32_t) * map_sig * slice));
  std::vector<cpx<float>> packed(map_sig * (size_t)slice);
  for (int64_t b0 = 0; b0 < batch; b0 += slice) {
    const int64_t nb = batch - b0 < slice ? batch - b0 : slice;
    for (size_t i = 0; i < map_sig * (size_t)nb; ++i) packed[i] = {0.0f, (float)bins_in[map_sig * b0 + i]};
    SSQ_HIP(hipMemcpy(d_map, packed.data(), sizeof(cpx<float>) * map_sig * nb, hipMemcpyHostToDevice));
    SSQ_HIP(msst_walk_run<float>((cpx<float>*)d_map, (int*)d_bins, nb, (int)n_rows, (long long)n_cols, n_iter, 0));
    SSQ_HIP(hipMemcpy(bins_out + map_sig * b0, d_bins, sizeof(int32_t) * map_sig * nb, hipMemcpyDeviceToHost));
  }
  return 0;
}

}  // extern "C"
