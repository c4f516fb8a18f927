// stft_tmsst.hip -- time-reassigned multisynchrosqueezed STFT, `upstream.tmssq_stft`, orders 1 and 2 (Yu,
// Lin, Ma and He 2020).  Upstream has no such transform: the definition is the project's own, restated in numpy by
// tests/helpers/tmsst_ref.py.  Everything up to the one-step target is tssq_stft's (stft_tsst.hip).  Per row, with t[m]
// the one-step target frame of frame m (none where |V| <= gamma) and H = ceil(n / (2 hop)):
//   c1[m] = t[m];   c(i+1)[m] = t[ci[m]] if t[ci[m]] is kept, else ci[m]                       (i = 1 .. n_iter - 1)
//   Tx[k, c_n[m]] += Sx[k, m] exp(-2 pi i ((k (m - c_n[m]) hop) mod n) / n)                    kept m, ascending source frame
// |c_n[m] - m| <= n_iter H, which must not exceed kTsstWideReach = 16384.
//
//   tsst_operator_kernel : stft_tsst.hip's, as it is: Sx, tau and the one-step relative targets (int16).
//   tmsst_walk_kernel    : a workgroup owns a tile of T frames of one row and stages the int16 relative targets of the
//                          frames within (n_iter - 1) H of it in LDS, along frames.  After one barrier every thread walks
//                          its frames n_iter - 1 steps in LDS (the stage is read-only: no barrier between steps; a chain
//                          ends early on a fixed point or on a frame that is not kept) and writes the final relative
//                          target c_n - m, int16, along frames, and the absolute one as int32 where asked for.  Tiles
//                          read each other's halos, so the walk writes a SECOND int16 plane, never in place.
//   tsst_scatter_kernel  : stft_tsst.hip's algorithm on the final plane with reach n_iter H: its instantiations with a
//                          stage of 8192 (reach <= 2048) or 36864 targets, both trimmed to the largest |target| staged.
#include <cmath>
#include <vector>

#include "../../include/ssq_hip.h"
#include "dev_buffers.h"
#include "stft_tsst.h"

namespace ssq {

constexpr int kTmsstMaxIter = 64;

// rel, out: [rows][n_frames] int16 relative targets (kTsstNone: not kept), rows = batch x F folded; abs_out (may be
// nullptr): the final targets as int32 frames, -1 where not kept.  halo = (n_iter - 1) H; tile + 2 halo <= STAGE.
// A target of the map stays inside 0 .. n_frames - 1 and within H of its frame (the operator clips it, the host entry
// checks a caller's map), so after i steps a chain is within i H of its frame: inside the stage whenever it is read.
template <int STAGE>
__global__ __launch_bounds__(kTsstThreads) void tmsst_walk_kernel(const short* __restrict__ rel, short* __restrict__ out,
                                                                  int* __restrict__ abs_out, long long n_frames, int tile,
                                                                  int halo, int n_iter) {
  __shared__ short rel_s[STAGE];
  const long long base = (long long)blockIdx.y * n_frames;
  const long long t0 = (long long)blockIdx.x * tile;
  const long long t1 = t0 + tile < n_frames ? t0 + tile : n_frames;
  const long long s0 = t0 - halo > 0 ? t0 - halo : 0;
  const long long s1 = t1 + halo < n_frames ? t1 + halo : n_frames;
  const int ns = (int)(s1 - s0);
  for (int i = threadIdx.x; i < ns; i += kTsstThreads) rel_s[i] = rel[base + s0 + i];
  __syncthreads();
  const int off = (int)(t0 - s0);
  for (int j = threadIdx.x; j < (int)(t1 - t0); j += kTsstThreads) {
    const int first = rel_s[off + j];
    int c = off + j;                                           // the chain's frame, as an index of the stage
    if (first != kTsstNone) {
      c += first;
      for (int i = 1; i < n_iter; ++i) {
        if (c < 0 || c >= ns) break;                           // (cannot happen on a map as described above)
        const int r = rel_s[c];
        if (r == kTsstNone || r == 0) break;                   // not kept, or a fixed point: the chain stops
        c += r;
      }
    }
    const long long m = t0 + j;
    out[base + m] = (short)(first == kTsstNone ? kTsstNone : c - (off + j));
    if (abs_out) abs_out[base + m] = first == kTsstNone ? -1 : (int)(s0 + c);
  }
}

// the walk of `rows` rows of n_frames frames on device buffers; tile: tsst_tile(n_iter H), halo = (n_iter - 1) H
hipError_t tmsst_walk_run(const short* d_rel, short* d_out, int* d_abs, long long rows, long long n_frames, int tile, int halo,
                          int n_iter) {
  const long long tiles = (n_frames + tile - 1) / tile;
  const long long stage = (long long)tile + 2LL * halo;
  if (tile < 1 || halo < 0 || stage > kTsstWideStage || tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  for (long long r0 = 0; r0 < rows; r0 += 65535) {
    const long long n1 = rows - r0 < 65535 ? rows - r0 : 65535;
    const dim3 grid((unsigned)tiles, (unsigned)n1);
    const short* in = d_rel + r0 * n_frames;
    short* out = d_out + r0 * n_frames;
    int* ab = d_abs ? d_abs + r0 * n_frames : (int*)nullptr;
    if (stage <= kTsstStage)
      hipLaunchKernelGGL(tmsst_walk_kernel<kTsstStage>, grid, dim3(kTsstThreads), 0, nullptr, in, out, ab, n_frames, tile, halo,
                         n_iter);
    else
      hipLaunchKernelGGL(tmsst_walk_kernel<kTsstWideStage>, grid, dim3(kTsstThreads), 0, nullptr, in, out, ab, n_frames, tile,
                         halo, n_iter);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace ssq

using namespace ssq;

namespace {

const char* tmsst_own_fail(int order, int n_iter) {
  if (order != 1 && order != 2) return "order must be 1 or 2";
  if (n_iter < 1 || n_iter > kTmsstMaxIter) return "n_iter must be from 1 to 64";
  return nullptr;
}

// tssq_stft's checks and shape, then the reach of the walked map: s->reach stays H, s->tile becomes the tile of n_iter H
int tmsst_shape(const FrameCall& c, TsstShape* s) {
  if (int rc = tsst_shape("tmssq_stft", tmsst_own_fail(c.order, c.n_iter), c, s)) return rc;
  if ((long long)c.n_iter * s->reach > kTsstWideReach)
    SSQ_FAIL("tmssq_stft: n_iter * ceil(n_fft / (2 hop)) must not exceed 16384");
  s->tile = tsst_tile((long long)c.n_iter * s->reach);
  return 0;
}

// tmssq_stft on device buffers (pipe_host, pipe_exec), in tssq_stft's workspace with the walked plane (tsst_work): the
// operator, the walk, the time scatter.  kernel_ms: three parts, the events recorded after the operator and after the
// walk.  rel: the one-step plane the operator writes (p.out names it), rel2: the walked plane.
template <typename T>
struct TmsstPipe {
  static constexpr int kMid = 2;
  const FrameCall& c;
  const TsstShape& s;
  DeviceBufs d;
  TsstDev<T> p;
  TsstScat<T> sc;
  cpx<T>*Tx, *Sx;
  int* tgt;
  short *rel, *rel2;
  double* xd;
  int tables() { return tsst_tables<T>(d, s, c, &p, &sc); }
  int bind(int64_t cap, void* const* outs /* Tx, Sx, tau, targets */, void* work) {
    const TsstWork k = tsst_work(c.dtype, cap, c.n_signal, s, true);
    Tx = (cpx<T>*)outs[0];
    Sx = (cpx<T>*)outs[1];
    tgt = (int*)outs[3];
    xd = (double*)((char*)work + k.xd);
    rel = (short*)((char*)work + k.rel);
    rel2 = (short*)((char*)work + k.rel2);
    sc.reach = c.n_iter * s.reach;
    sc.tile = s.tile;
    return tsst_out_block<T>(d, s, c.hop, Sx, outs[2], rel, &p);
  }
  int run(int64_t nb, const void* d_x, const hipEvent_t* mid) {
    SSQ_HIP(tsst_operator_run<T>(p, s, (const T*)d_x, nb, xd));
    if (mid[0]) SSQ_HIP(hipEventRecord(mid[0], nullptr));
    const bool walk = c.n_iter > 1 || tgt;                   // (one step, no targets asked for: the map is final)
    if (walk)
      SSQ_HIP(tmsst_walk_run(rel, rel2, tgt, (long long)nb * s.n_freqs, (long long)s.n_frames, s.tile,
                             (c.n_iter - 1) * s.reach, c.n_iter));
    if (mid[1]) SSQ_HIP(hipEventRecord(mid[1], nullptr));
    SSQ_HIP(tsst_scatter_run<T>(sc, s, nb, Sx, walk ? rel2 : rel, Tx, true));
    return 0;
  }
};

// the checks ssq_tmsst_walk_host and ssq_tmsst_tile_frames share (sets the error and returns non-zero)
int tmsst_reach_ok(int64_t reach, int n_iter) {
  if (n_iter < 1 || n_iter > kTmsstMaxIter) SSQ_FAIL("tmsst_walk: n_iter must be from 1 to 64");
  if (reach < 1) SSQ_FAIL("tmsst_walk: reach must be >= 1");
  if (reach > kTsstWideReach || (long long)n_iter * reach > kTsstWideReach)
    SSQ_FAIL("tmsst_walk: n_iter * reach must not exceed 16384");
  return 0;
}

}  // namespace

extern "C" {

int ssq_tmssq_stft_host(int dtype, const void* x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                        int64_t hop, double fs, int padtype, int order, double gamma, int variant, int n_iter, void* Tx,
                        void* Sx, void* tau, int32_t* targets) {
  if (!x || !window || !Tx || !Sx) SSQ_FAIL("NULL argument");
  const FrameCall c{dtype, batch, n_signal, window, n_fft, hop, fs, padtype, gamma, variant, SSQ_SQUEEZE_SUM, order, n_iter};
  TsstShape s;
  if (int rc = tmsst_shape(c, &s)) return rc;
  if (int rc = require_device()) return rc;
  const size_t el = dtype == SSQ_F32 ? 4 : 8, map_sig = (size_t)s.n_freqs * (size_t)s.n_frames;
  const HostOut outs[] = {{Tx, 2 * el * map_sig}, {Sx, 2 * el * map_sig}, {tau, el * map_sig}, {targets, sizeof(int32_t) * map_sig}};
  const size_t work = (size_t)tsst_work(dtype, 1, n_signal, s, true).bytes;
  return dtype == SSQ_F32 ? pipe_host<TmsstPipe<float>>(c, s, x, el * (size_t)n_signal, outs, work)
                          : pipe_host<TmsstPipe<double>>(c, s, x, el * (size_t)n_signal, outs, work);
}

int64_t ssq_tmssq_stft_workspace_bytes(int dtype, int64_t batch, int64_t n_signal, int64_t n_fft, int64_t hop, int n_iter) {
  FrameCall c = frame_sizes_call(dtype, batch, n_signal, n_fft, hop);
  c.n_iter = n_iter;
  TsstShape s;
  if (tmsst_shape(c, &s)) return -1;
  return tsst_work(dtype, batch, n_signal, s, true).bytes;
}

int ssq_tmssq_stft_exec(int dtype, const void* d_x, int64_t batch, int64_t n_signal, const double* window, int64_t n_fft,
                        int64_t hop, double fs, int padtype, int order, double gamma, int variant, int n_iter, void* d_Tx,
                        void* d_Sx, void* d_tau, int32_t* d_targets, void* d_workspace, int64_t workspace_bytes,
                        float* kernel_ms) {
  if (!d_x || !window || !d_Tx || !d_Sx || !d_workspace) SSQ_FAIL("NULL argument");
  const FrameCall c{dtype, batch, n_signal, window, n_fft, hop, fs, padtype, gamma, variant, SSQ_SQUEEZE_SUM, order, n_iter};
  TsstShape s;
  if (int rc = tmsst_shape(c, &s)) return rc;
  if (workspace_bytes < tsst_work(dtype, batch, n_signal, s, true).bytes)
    SSQ_FAIL("tmssq_stft: workspace smaller than ssq_tmssq_stft_workspace_bytes");
  if (int rc = require_device()) return rc;
  void* const outs[] = {d_Tx, d_Sx, d_tau, d_targets};
  return dtype == SSQ_F32 ? pipe_exec<TmsstPipe<float>>(c, s, d_x, outs, d_workspace, kernel_ms)
                          : pipe_exec<TmsstPipe<double>>(c, s, d_x, outs, d_workspace, kernel_ms);
}

int ssq_tmsst_tile_frames(int64_t reach, int n_iter) {
  if (tmsst_reach_ok(reach, n_iter)) return -1;
  return tsst_tile((long long)n_iter * reach);
}

int ssq_tmsst_walk_host(const int32_t* targets_in, int64_t batch, int64_t n_rows, int64_t n_frames, int n_iter, int64_t reach,
                        int32_t* targets_out) {
  if (!targets_in || !targets_out) SSQ_FAIL("NULL argument");
  if (batch < 1 || n_rows < 1) SSQ_FAIL("tmsst_walk: batch and n_rows must be >= 1");
  if (n_frames < 1 || n_frames > (1LL << 30)) SSQ_FAIL("tmsst_walk: n_frames must be from 1 to 2^30");
  if (int rc = tmsst_reach_ok(reach, n_iter)) return rc;
  const size_t map_sig = (size_t)n_rows * (size_t)n_frames;
  for (size_t i = 0; i < map_sig * (size_t)batch; ++i) {
    const int64_t t = targets_in[i], m = (int64_t)(i % (size_t)n_frames);
    if (t == -1) continue;
    if (t < 0 || t >= n_frames) SSQ_FAIL("tmsst_walk: a target lies outside -1 .. n_frames - 1");
    if (t - m > reach || m - t > reach) SSQ_FAIL("tmsst_walk: a target lies farther than reach from its own frame");
  }
  if (int rc = require_device()) return rc;
  // the kernel's format is the int16 relative target: packing to it is host plumbing
  DeviceBufs d;
  const int64_t slice = slice_signals(batch, (double)map_sig * (2 * sizeof(short) + sizeof(int32_t)), 0.0, batch);
  void *d_rel, *d_rel2, *d_tgt;
  SSQ_HIP(d.alloc(&d_rel, sizeof(short) * map_sig * slice));
  SSQ_HIP(d.alloc(&d_rel2, sizeof(short) * map_sig * slice));
  SSQ_HIP(d.alloc(&d_tgt, sizeof(int32_t) * map_sig * slice));
  std::vector<short> packed(map_sig * (size_t)slice);
  const int tile = tsst_tile((long long)n_iter * reach);
  for (int64_t b0 = 0; b0 < batch; b0 += slice) {
    const int64_t nb = batch - b0 < slice ? batch - b0 : slice;
    for (size_t i = 0; i < map_sig * (size_t)nb; ++i) {
      const int32_t t = targets_in[map_sig * b0 + i];
      packed[i] = t < 0 ? (short)kTsstNone : (short)(t - (int64_t)(i % (size_t)n_frames));
    }
    SSQ_HIP(hipMemcpy(d_rel, packed.data(), sizeof(short) * map_sig * nb, hipMemcpyHostToDevice));
    SSQ_HIP(tmsst_walk_run((const short*)d_rel, (short*)d_rel2, (int*)d_tgt, (long long)nb * n_rows, (long long)n_frames, tile,
                           (int)((n_iter - 1) * reach), n_iter));
    SSQ_HIP(hipMemcpy(targets_out + map_sig * b0, d_tgt, sizeof(int32_t) * map_sig * nb, hipMemcpyDeviceToHost));
  }
  return 0;
}

}  // extern "C"
