// stft_fused.hip -- launches of the fused STFT / synchrosqueezed-STFT kernel (stft_fused_kernel.h) for power-of-two
// n_fft, and the 16-wave kernel for fp32 n_fft = 1024 (the headline path).
#include "stft_fused_kernel.h"
#include "tx1024_lds_layout.h"

namespace ssq {

// ---------------------------------------------------------------------------------------------
// High-occupancy variant for fp32, n_fft = 1024, SSQ_OUT_TX: 16 waves per CU (4 per SIMD) instead of 8.
// The 8-wave kernel is bound by exposed latency (two waves per SIMD cannot cover the LDS round trips);
// to fit 16 waves the per-wave LDS row shrinks to HALF a frame and the registers to <= 128:
//   * exchange 1 goes through the half-size row in two phases (lanes 0-31 write, all read their first
//     8 values; lanes 32-63 write, all read the other 8) -- the DS unit runs a wave's ops in order;
//   * exchange 2 is a 4x4 transpose between the four 16-lane rows and the low two bits of the register
//     index: v_permlane32_swap + v_permlane16_swap, no LDS;
//   * twiddles come from an LDS copy of the W_1024 table, samples are prefetched one tile ahead;
//   * window, twiddles and the exchange-1 row are laid out (tx1024_lds_layout.h) so that the two elements a lane
//     consumes together are adjacent: every such read is one ds_read_b128.
// One tile = one frame per wave, so the tile barrier comes once per frame per wave.
// ---------------------------------------------------------------------------------------------
// (Measured and not kept: the FFT on packed fp32 -- 25 % fewer vector instructions, same time, because two waves already
// share the SIMD's 32 lanes for scalar fp32 add/mul/fma, profiles/r03_ab_pk.txt; merging lane pairs with equal
// destinations before the LDS atomic, a net loss since the read-out/exchange rework, profiles/r02_ab_libs2.txt;
// 8-wave blocks two per CU, profiles/r01_ab_two_8wave_blocks.txt.)
struct Hi1024 {
  static constexpr int N = 1024, L = 64, NF = 513, W = 16, F = 16, PITCH = F + 1, THREADS = W * 64;
  static constexpr int PLANE = NF * PITCH;
  static constexpr int TILE_BYTES = (((2 * PLANE + F) * 4 + 15) / 16) * 16;
  // the register-half exchange lays a half row out as 32 blocks (r, g) of 8 values x 2 writers (+ pads)
  static constexpr int EXH_ELEMS = tx1024::EXCH_ELEMS;
  static constexpr int EXH_BYTES = W * EXH_ELEMS * 8;
  static constexpr int TAB_BYTES = tx1024::TAB_ELEMS * 8;   // window table [8][64][2]; twiddle tables [16][18] + [6][64][2]
  static constexpr int LDS_BYTES = TILE_BYTES + EXH_BYTES + TAB_BYTES;
  static constexpr int FRAC = 30, EMIN = -90;
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
  static_assert(N == tx1024::N && NF == tx1024::NF && W == tx1024::W && F == tx1024::F && PITCH == tx1024::PITCH &&
                    TILE_BYTES == tx1024::TILE_BYTES && LDS_BYTES == tx1024::LDS_BYTES,
                "tx1024_lds_layout.h describes this kernel's image (and asserts the 16-byte alignment of its parts)");
};

// two adjacent complex elements at a 16-byte aligned LDS address: one ds_read_b128
__device__ __forceinline__ void lds_pair(const cpx<float>* q, cpx<float>& a, cpx<float>& b) {
  const float4 w = *reinterpret_cast<const float4*>(q);
  a = {w.x, w.y};
  b = {w.z, w.w};
}

// 4x4 transpose of R[0..3] across the four 16-lane rows of the wave (one dword per lane per register)
__device__ __forceinline__ void rows_transpose4(float& r0, float& r1, float& r2, float& r3) {
  auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(r0), __float_as_uint(r2), false, false);
  auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(r1), __float_as_uint(r3), false, false);
  auto c = __builtin_amdgcn_permlane16_swap(a[0], b[0], false, false);
  auto d = __builtin_amdgcn_permlane16_swap(a[1], b[1], false, false);
  r0 = __uint_as_float(c[0]);
  r1 = __uint_as_float(c[1]);
  r2 = __uint_as_float(d[0]);
  r3 = __uint_as_float(d[1]);
}

// window multiply of a frame's prefetched samples (lane t holds x[t + 64 q]) and pass 0 of its FFT.  The multiply is the
// first use of xn[], so the vmcnt waits for the prefetch sit here; and it stays in ONE basic block with pass 0's first
// butterflies, because the compiler contracts the two (fma(x[q], w[q], x[q + 8] w[q + 8])): apart, the bits change.
__device__ __forceinline__ void tx1024_window_pass0(const cpx<float>* win_lds, int t, const float (&xn)[16],
                                                    const cpx<float> (&twr_unused)[3][16], cpx<float> (&v)[16]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    cpx<float> w0, w1;
    lds_pair(win_lds + tx1024::win_row(t, j), w0, w1);
    v[2 * j] = {xn[2 * j] * w0.x, xn[2 * j] * w0.y};
    v[2 * j + 1] = {xn[2 * j + 1] * w1.x, xn[2 * j + 1] * w1.y};
  }
  fft_compute<float, 10, 0, false, false>(v, twr_unused, nullptr, t);
}

// (Measured and removed in round 2: replacing the two tile barriers by arrival counters in LDS, with the read-out of
// tile i-1 placed inside tile i's FFT or at the loop top, ran 10-14 % SLOWER -- profiles/r02_ab_freerun.txt.)
// PAIRED picks the tile read-out at COMPILE time (see read_out): the host passes it for the interior Tx launch with
// even n_frames (launch_one).
template <bool EDGE, bool LEB, bool WKDBG = false, bool PAIRED = false>
__global__ __launch_bounds__(1024, 1) void stft_tx1024_kernel(StftDev<float> p) {
  static_assert(!PAIRED || (!EDGE && !WKDBG), "the paired read-out has no frame guard and no (w, k) form");
  using H = Hi1024;
  constexpr int THREADS = H::THREADS;
  using T = float;
  constexpr int N = H::N, L = H::L, NF = H::NF, F = H::F, PITCH = H::PITCH;
  __shared__ __attribute__((aligned(16))) unsigned char smem[H::LDS_BYTES];
  int* tile_re = reinterpret_cast<int*>(smem);               // [NF][PITCH] 64-bit (re, im) cells
  float* col_scale = reinterpret_cast<float*>(tile_re + 2 * H::PLANE);
  cpx<T>* exch_all = reinterpret_cast<cpx<T>*>(smem + H::TILE_BYTES);
  cpx<T>* win_lds = reinterpret_cast<cpx<T>*>(smem + H::TILE_BYTES + H::EXH_BYTES);
  namespace X = tx1024;
  cpx<T>* tw1 = win_lds + X::WIN_ELEMS;   // pass 1: [k = 0..15][m = 1..15, filler | 2 pad]   W_256^(k m)
  cpx<T>* tw2 = tw1 + X::TW1_ELEMS;       // pass 2: [pair i = 0..5][t = 0..63][2]   W_1024^((t + 64 b) m), (b, m) b-major

  const int tid = threadIdx.x;
  const int t = tid & 63;          // lane = position inside the frame
  // wave-uniform by construction: say so, and everything derived from it (exchange row, column-scale slot, frame index)
  // lives in scalar registers instead of (spilled) vector ones
  const int fl = __builtin_amdgcn_readfirstlane(tid >> 6);         // wave = frame inside the tile
  cpx<T>* exch = exch_all + fl * H::EXH_ELEMS;

  // table fill in SLOT order: consecutive threads store consecutive LDS elements (no bank conflicts) and gather the
  // 16 KiB of cached global tables instead; the pads of the pass-1 rows get W^0 like the filler
  for (int s = tid; s < X::WIN_ELEMS; s += THREADS) win_lds[s] = p.win2[X::win_elem(s)];
  for (int s = tid; s < X::TW1_ELEMS; s += THREADS) tw1[s] = p.tw[(X::tw1_k(s) * X::tw1_m(s) * 4) & (N - 1)];
  for (int s = tid; s < X::TW2_ELEMS; s += THREADS) tw2[s] = p.tw[(X::tw2_j(s) * X::tw2_m(s)) & (N - 1)];
  // 64-bit cells start at RE = 2^31: RE + 2^31 stays in [0, 2^32), so no borrow ever reaches the high word and the
  // read-out takes IM = high word, RE = low word ^ 2^31 -- one instruction less per cell than undoing a borrow
  constexpr long long CELL0 = WKDBG ? 0LL : 0x80000000LL;
  for (int i = tid; i < H::PLANE; i += THREADS) reinterpret_cast<long long*>(tile_re)[i] = CELL0;
  __syncthreads();
  const unsigned bid = blockIdx.x;
  if ((long long)bid >= p.total_tiles) return;

  const long long n_sig = p.total_tiles / p.tiles_per_signal;
  long long sig = (long long)(bid / (unsigned)p.tiles_per_signal);
  int jt = (int)(bid % (unsigned)p.tiles_per_signal);
  auto tile_frame0 = [&](int j) { return ((j < p.ta_n) ? p.ta0 + j : p.tb0 + (j - p.ta_n)) * F; };
  auto load_frame = [&](long long sg, int frame0, T (&xv)[16]) {
    const int frame = frame0 + fl;
    const T* xs = sig_base(p, sg);
    const long long pos0 = (long long)frame * p.hop - p.pad_left + t;
    if constexpr (!EDGE) {
#pragma unroll
      for (int q = 0; q < 16; ++q) xv[q] = xs[pos0 + L * q];
    } else {
      // one wave-uniform branch around two straight runs of loads (a branch per sample makes every load wait for itself)
      const bool valid = frame < p.n_frames;
      const long long first = pos0 - t;
      if (__all(valid && first >= 0 && first + N <= p.n_signal)) {
#pragma unroll
        for (int q = 0; q < 16; ++q) xv[q] = xs[pos0 + L * q];
      } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) xv[q] = load_padded_flat<false>(xs, pos0 + L * q, p.n_signal, p.padtype, valid);
      }
    }
  };
  T xn[16];
  load_frame(sig, tile_frame0(jt), xn);
  const cpx<T> twr_unused[3][16] = {};

  // ---- tile read-out: re-zeroes what it reads ----
  // EXACTLY ONE store sequence per instantiation, chosen by PAIRED and never by a run-time test of n_frames.  With both
  // sequences behind a test the loop body has a path from one tile barrier to the next that passes through neither, and
  // the compiler's wait counts must assume the fewest operations behind the prefetched samples: no store at all.  The
  // window multiply at the loop top then waits vmcnt(7..0) for xn[] -- loads and stores share that one in-order counter
  // -- and with it for every Tx store of the tile just read out, once per tile, all 16 waves at the same point.  With
  // one unguarded sequence (and the waits behind it, see PASS0_AT_END) they read vmcnt(>= number of stores) and the
  // stores stay in flight under the next tile's window multiply, pass 0 and exchange 1
  // (tests/test_tx1024_isa_waits.py holds this).  Do not fold the test of n_frames back in.
  auto read_out = [&](long long rsig, int rframe0) {
    if constexpr (PAIRED) {
      // thread -> (frame pair fp, rows k0 + 128 j): two adjacent cells per thread, ONE 16-byte store per row
      // (half as many store instructions; T21 of the programming guide).  Needs even n_frames for the alignment.
      constexpr int RS2 = THREADS / (F / 2);              // 128 rows per sweep
      const int fp = tid % (F / 2);
      const int k0 = tid / (F / 2);
      float4* __restrict__ og4 = reinterpret_cast<float4*>(p.out + rsig * (long long)NF * p.n_frames + rframe0 + 2 * fp +
                                                           (long long)k0 * p.n_frames);
      const long long gstep4 = (long long)RS2 * p.n_frames / 2;     // in float4 units
      // (round 3: a wave-uniform base + 32-bit per-thread offset does not make the compiler take the SGPR-base store form --
      //  loop strength reduction rebuilds the 64-bit vector address chain either way.  A raw buffer store through a
      //  per-signal descriptor does take it -- 10 vector instructions per sweep, no address arithmetic -- and so does a
      //  64-bit LDS exchange in place of the read + CELL0 store (one ds_wrxchg_rtn_b64 per cell); on top of the short
      //  Nyquist pass neither pays: +0.4 ... +0.7 % and +-0, profiles/readout_ab_parts.txt)
      const T sc0 = col_scale[2 * fp], sc1 = col_scale[2 * fp + 1];
      long long* tc = reinterpret_cast<long long*>(tile_re) + k0 * PITCH + 2 * fp;
      auto sweep2 = [&](int j) {
        const long long c0 = tc[j * RS2 * PITCH], c1 = tc[j * RS2 * PITCH + 1];
        tc[j * RS2 * PITCH] = CELL0;
        tc[j * RS2 * PITCH + 1] = CELL0;
        const int r0 = (int)c0 ^ (int)0x80000000, r1 = (int)c1 ^ (int)0x80000000;
        const int i0 = (int)(c0 >> 32), i1 = (int)(c1 >> 32);
        const float4 val = make_float4((T)r0 * sc0, (T)i0 * sc0, (T)r1 * sc1, (T)i1 * sc1);
        // nontemporal: Tx is written once, never read back here (-0.7 % on the bench shape, profiles/r02_ab_nt.txt)
        typedef float vf4 __attribute__((ext_vector_type(4)));
        const vf4 nv = {val.x, val.y, val.z, val.w};
        __builtin_nontemporal_store(nv, reinterpret_cast<vf4*>(&og4[j * gstep4]));
      };
      constexpr int NFULL2 = NF / RS2;                      // 4 full sweeps
#pragma unroll
      for (int j = 0; j < NFULL2; ++j) sweep2(j);
      if (k0 + NFULL2 * RS2 < NF) sweep2(NFULL2);
      return;
    }
    // thread -> (frame f, rows k0 + 64 j)
    constexpr int RSTEP = THREADS / F;                    // 64 rows per sweep
    const int f = tid % F;
    const int k0 = tid / F;
    cpx<T>* __restrict__ og = p.out + rsig * (long long)NF * p.n_frames + rframe0 + f + (long long)k0 * p.n_frames;
    const long long gstep = (long long)RSTEP * p.n_frames;
    const bool fvalid = EDGE ? (rframe0 + f < p.n_frames) : true;
    const T sc = col_scale[f];
    constexpr int NFULL = NF / RSTEP;                     // 8 full sweeps
    long long* tc = reinterpret_cast<long long*>(tile_re) + k0 * PITCH + f;
    auto sweep = [&](int j) {
      const long long c = tc[j * RSTEP * PITCH];
      tc[j * RSTEP * PITCH] = CELL0;
      if constexpr (WKDBG) {
        if (fvalid) og[j * gstep] = cpx<T>{__int_as_float((int)c), __int_as_float((int)(c >> 32))};
        return;
      }
      const int ire = (int)c ^ (int)0x80000000;
      const int iim = (int)(c >> 32);
      if (fvalid) og[j * gstep] = cpx<T>{(T)ire * sc, (T)iim * sc};
    };
#pragma unroll
    for (int j = 0; j < NFULL; ++j) sweep(j);
    if (k0 + NFULL * RSTEP < NF) sweep(NFULL);
  };

  const int grid_n = (int)gridDim.x;          // (read once: inside the loop it is a scalar load + wait per tile)
  // The interior instantiations take the window multiply and pass 0 of the block's FIRST tile ahead of the loop and
  // those of every later tile at the loop's end, behind the read-out -- the same instruction order tile after tile.
  // At the loop top the waits for xn[] would also be reached from the block's first sample load, which has no store
  // behind it, and the wait counts take the fewest: vmcnt(7..0) again, the drain read_out's comment speaks of.  At the
  // loop's end the only way in is through the read-out's stores.
  // (The edge kernel's stores are guarded per frame and make their own store-free path; it keeps the plain loop.)
  constexpr bool PASS0_AT_END = !EDGE && !WKDBG;
  cpx<T> vw[16];                              // (dead in the plain loop)
  if constexpr (PASS0_AT_END) tx1024_window_pass0(win_lds, t, xn, twr_unused, vw);
#pragma unroll 1
  while (true) {
    const int frame0 = tile_frame0(jt);
    const bool valid = EDGE ? (frame0 + fl < p.n_frames) : true;
    // next tile of this block; prefetch its samples behind this frame's FFT
    long long nsig = sig;
    int njt = jt + grid_n;
    while (njt >= p.tiles_per_signal) {
      njt -= p.tiles_per_signal;
      ++nsig;
    }
    const bool has_next = nsig < n_sig;
    cpx<T> v[16];
    if constexpr (PASS0_AT_END) {
#pragma unroll
      for (int q = 0; q < 16; ++q) v[q] = vw[q];
    } else {
      // (tx1024_window_pass0 written out: through the call the compiler schedules the edge kernel's sample loads
      //  differently, and this change leaves that kernel's code as it was)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        cpx<T> w0, w1;
        lds_pair(win_lds + X::win_row(t, j), w0, w1);
        v[2 * j] = {xn[2 * j] * w0.x, xn[2 * j] * w0.y};
        v[2 * j + 1] = {xn[2 * j + 1] * w1.x, xn[2 * j + 1] * w1.y};
      }
      // ---- pass 0: radix 16 over elements t + 64q ----
      fft_compute<T, 10, 0, false, false>(v, twr_unused, nullptr, t);
    }
    // ---- exchange 1 by REGISTER halves: in phase ph EVERY lane writes its values u = 8 ph .. 8 ph + 7 (elements
    //      16 t + u) -- full-width stores -- and the lanes whose element residue (t & 15) lies in that half read all 16
    //      of their elements t + 64 q = 16 ((t >> 4) + 4 q) + (t & 15).
    //      Row layout (tx1024_lds_layout.h): the values of writers (t >> 4) + 8 g and + 8 g + 4 are adjacent, so the
    //      16 loads are 8 of 16 bytes; store groups and load groups stay on distinct banks.
    {
      cpx<T> nv[16];
      const int sbase = X::exch_store_base(t), lbase = X::exch_load_base(t);
#pragma unroll
      for (int ph = 0; ph < 2; ++ph) {
#pragma unroll
        for (int u = 0; u < 8; ++u) exch[sbase + X::exch_val(u)] = v[8 * ph + u];
        frame_sync<false>();
        if (((t >> 3) & 1) == ph) {
#pragma unroll
          for (int g = 0; g < 8; ++g) lds_pair(exch + lbase + X::exch_load_off(g), nv[2 * g], nv[2 * g + 1]);
        }
        frame_sync<false>();
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) v[q] = nv[q];
    }
    // the next tile's samples: issued only now, after exchange 1 -- during the exchange both the old and the new
    // register set of the frame are live, and 16 more registers in flight there push the kernel into scratch; the rest
    // of this tile (pass 1, pass 2, epilogue, read-out: > 10k cycles) still covers the HBM latency many times over
    if (has_next) load_frame(nsig, tile_frame0(njt), xn);
    // ---- pass 1: twiddle W_256^(k m), radix 16 (fft_compute's multiply order, the twiddles fetched in pairs) ----
    {
      const cpx<T>* row = tw1 + X::tw1_row(t & 15, 0);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        cpx<T> w0, w1;
        lds_pair(row + 2 * i, w0, w1);
        v[2 * i + 1] = cmul(v[2 * i + 1], w0);
        if (i < 7) v[2 * i + 2] = cmul(v[2 * i + 2], w1);       // (the pair of m = 15 is the filler)
      }
      constexpr int R = pass_radix(10, 1), NB = 16 / R;
      butterflies<false, R, NB>(v, std::make_integer_sequence<int, NB>{});
    }
    // ---- exchange 2: producer (row m, k), reg u = 4 uh + ul  ->  consumer (row ul, k), reg 4 m + uh ----
    {
#pragma unroll
      for (int uh = 0; uh < 4; ++uh) {
        rows_transpose4(v[4 * uh + 0].x, v[4 * uh + 1].x, v[4 * uh + 2].x, v[4 * uh + 3].x);
        rows_transpose4(v[4 * uh + 0].y, v[4 * uh + 1].y, v[4 * uh + 2].y, v[4 * uh + 3].y);
      }
      // slot 4*uh + a now holds consumer register q = 4*a + uh: transpose the register indices
#define SSQ_SWAP(i, j)       \
  {                          \
    const cpx<T> t_ = v[i];  \
    v[i] = v[j];             \
    v[j] = t_;               \
  }
      SSQ_SWAP(1, 4) SSQ_SWAP(2, 8) SSQ_SWAP(3, 12) SSQ_SWAP(6, 9) SSQ_SWAP(7, 13) SSQ_SWAP(11, 14)
#undef SSQ_SWAP
    }
    // ---- pass 2: twiddle W_1024^((t + 64 b) m), four radix-4 butterflies ----
    {
      constexpr int R = pass_radix(10, 2), NB = 16 / R;
      static_assert(R == 4 && NB == 4, "tw2 rows hold (b, m), b < 4, m = 1..3");
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        cpx<T> w0, w1;
        lds_pair(tw2 + X::tw2_row(t, i), w0, w1);
        const int e0 = 2 * i, e1 = 2 * i + 1;                  // entry e = 3 b + (m - 1) multiplies v[b + m NB]
        v[e0 / 3 + (e0 % 3 + 1) * NB] = cmul(v[e0 / 3 + (e0 % 3 + 1) * NB], w0);
        v[e1 / 3 + (e1 % 3 + 1) * NB] = cmul(v[e1 / 3 + (e1 % 3 + 1) * NB], w1);
      }
      butterflies<false, R, NB>(v, std::make_integer_sequence<int, NB>{});
    }
    // lane t now holds Z[t + 64 q]

    // ---- partner Z[N-k] for the bins this lane owns ----
    cpx<T> zp[9];
    {
      const int src = (L - t) & (L - 1);
      // lane 0 pairs with ITSELF one register up (N - 64 q = 64 (16 - q)): rotate its upper registers once (16 moves
      // under a one-lane mask) instead of 16 selects; nobody else reads lane 0's upper half (src == 0 only for t == 0)
      // (re-fetching them by 16 one-lane ds_bpermute instead: +17 %, profiles/r02_ab_libs4.txt)
      zp[8] = v[8];
      if (t == 0) {
#pragma unroll
        for (int j = 8; j < 15; ++j) v[j] = v[j + 1];
        v[15] = v[0];
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        zp[q].x = __shfl(v[15 - q].x, src);
        zp[q].y = __shfl(v[15 - q].y, src);
      }
      v[8] = zp[8];
    }

    // ---- unpack, phase transform, bin index, fixed-point scatter (same arithmetic as stft_fused_kernel) ----
    {
      cpx<T> cv[9];
      int dstb[9];
      T wdbg[9];
      int kdbg[9];
      T l1 = 0.0f;
      constexpr int CELL = 8;                                  // bytes per tile cell (interleaved re, im)
      const float lane_on = valid ? 1.0f : 0.0f;
      const float sfs0 = (float)t * p.sfs_step, sfs_q = (float)L * p.sfs_step;
      const int neg_last = -(p.n_freqs - 1);
      // sum mode: the wave-wide loop serves bins t + 64 q, q < 8, and k = 512 follows it in a shorter form.  The Lebesgue
      // instantiation keeps the ninth pass: with the split it spills 10 dwords instead of none.
      constexpr bool NYQ = !LEB;
      constexpr int NQ = NYQ ? 8 : 9;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const cpx<T> zk = v[q], zn = zp[q];
        const cpx<T> S = {zk.x + zn.x, zk.y - zn.y};
        const cpx<T> dS = {zk.y + zn.y, zn.x - zk.x};
        const float den = S.x * S.x + S.y * S.y;
        const float num = dS.y * S.x - dS.x * S.y;
        const float pd = num * __builtin_amdgcn_rcpf(den * p.two_pi_eff);
        // d = Sfs - pd; w = |d| (ssq_stft.rs:33) is only ever used through modifiers: the finiteness mask ignores the sign and
        // the bin fma takes -|d| (round 3: nine v_and per frame less -- those do not pair with another wave's instruction)
        const float d = (sfs0 + (float)q * sfs_q) - pd;
        const float w = fabsf(d);
        float m = fma_clamp01(den, p.keep_big, p.keep_bias) * fma_clamp01(d, 0.0f, 1.0f);
        if constexpr (LEB) m = leb_keep_f32(m, den, w, p.gamma2);
        if (EDGE) m *= lane_on;
        if (q == 8) m *= (t == 0) ? 1.0f : 0.0f;
        const cpx<T> c = LEB ? cpx<T>{p.leb_unit * m, 0.0f} : cpx<T>{S.x * m, S.y * m};
        cv[q] = c;
        int kneg = cvt_floor_i32(__builtin_fmaf(-w, p.inv_dw, 0.5f));
        kneg = kneg < neg_last ? neg_last : kneg;
        if constexpr (LEB) kneg = (w != w) ? 0 : kneg;          // a kept NaN bin: the scan leaves k = 0 (leb_keep_f32)
        dstb[q] = __mul24(kneg, -(PITCH * CELL)) + fl * CELL;
        l1 += fabsf(c.x) + fabsf(c.y);
        if constexpr (WKDBG) {
          wdbg[q] = w;
          kdbg[q] = (m != 0.0f) ? -kneg : -1;
        }
      }
      if constexpr (NYQ) {
        // ---- k = 512 (Nyquist), owned by lane 0: the loop body at q = 8 with zn = zk (zp[8] IS v[8], on every lane),
        //      every step below equal to the general one in value, NaN cases included (-1.5 %, same bits:
        //      profiles/readout_ab_parts.txt):
        //   S.x = zk.x + zk.x;  S.y = zk.y - zk.y = +0, or NaN for a non-finite zk.y;  dS.x = zk.y + zk.y;
        //   dS.y = zk.x - zk.x = +0, or NaN exactly when S.x is not finite either;
        //   den = S.x^2 + S.y^2 = round(S.x^2) (+ 0), NaN with S.y: fma(S.x, S.x, S.y) under either contraction;
        //   num = dS.y S.x - dS.x S.y is +-0, or NaN exactly when S.x or dS.x is not finite (a NaN S.y comes with a
        //         non-finite dS.x): 0 S.x + 0 dS.x has the same NaN cases and is +-0 otherwise -- the sign of a zero pd is
        //         lost in Sfs - pd, Sfs(512) > 0;  pd = num * rcp(..) still turns NaN for den = 0 (0 * inf);
        //   so d is Sfs(512) or NaN, and the masks, w and the bin index are taken from that true d as before;
        //   c.y = S.y m is +-0 or (m is finite) the NaN of S.y: |c.y| = |S.y| for the column's L1, and its fixed-point
        //         value rounds to 0 both ways (the conversion takes NaN to 0), so the 64-bit add is hi = ia >> 31, lo = ia.
        const cpx<T> zk = v[8];
        const float sx = zk.x + zk.x, sy = zk.y - zk.y, dsx = zk.y + zk.y;
        const float den = __builtin_fmaf(sx, sx, sy);
        const float num = __builtin_fmaf(0.0f, sx, 0.0f * dsx);
        const float pd = num * __builtin_amdgcn_rcpf(den * p.two_pi_eff);
        const float d = (sfs0 + 8.0f * sfs_q) - pd;
        const float w = fabsf(d);
        float m = fma_clamp01(den, p.keep_big, p.keep_bias) * fma_clamp01(d, 0.0f, 1.0f);
        if (EDGE) m *= lane_on;
        m *= (t == 0) ? 1.0f : 0.0f;
        cv[8] = cpx<T>{sx * m, 0.0f};
        int kneg = cvt_floor_i32(__builtin_fmaf(-w, p.inv_dw, 0.5f));
        kneg = kneg < neg_last ? neg_last : kneg;
        dstb[8] = __mul24(kneg, -(PITCH * CELL)) + fl * CELL;
        l1 += fabsf(cv[8].x) + fabsf(sy);
        if constexpr (WKDBG) {
          wdbg[8] = w;
          kdbg[8] = (m != 0.0f) ? -kneg : -1;
        }
      }
      const T tot = frame_allreduce<T, L, false>(l1, t, nullptr, t) * p.dw;
      T scale, inv_scale;
      column_scale<T, H::FRAC, H::EMIN>(tot, p.dw, scale, inv_scale);
      if (t == 0 && valid) col_scale[fl] = inv_scale;
      // fixed-point contributions; scatter one 64-bit add per bin into the (re, im) cell, which holds the integer
      // IM * 2^32 + RE + 2^31: a negative RE carries its borrow into IM at the add (hi = IM + (RE >> 31))
      char* ptile = reinterpret_cast<char*>(tile_re);
      if constexpr (WKDBG) {
#pragma unroll
        for (int q = 0; q < 9; ++q) {
          if ((q < 8 || t == 0) && valid) {
            const unsigned lo = (unsigned)__float_as_int(wdbg[q]), hi = (unsigned)__float_as_int((float)kdbg[q]);
            reinterpret_cast<unsigned long long*>(ptile)[(t + L * q) * PITCH + fl] = ((unsigned long long)hi << 32) | lo;
          }
        }
      } else {
#pragma unroll
        for (int q = 0; q < 9; ++q) {
          const int ia = cvt_round_i32(cv[q].x * scale);
          const int ib = (LEB || q == 8) ? 0 : cvt_round_i32(cv[q].y * scale);
          if (q < 8 || t == 0) {
            if (LEB) {
              atomicAdd(reinterpret_cast<unsigned*>(ptile + dstb[q]), (unsigned)ia);             // RE >= 0: no borrow
            } else {
              const unsigned hi = (unsigned)(ib + (ia >> 31));
              atomicAdd(reinterpret_cast<unsigned long long*>(ptile + dstb[q]),
                        ((unsigned long long)hi << 32) | (unsigned)ia);
            }
          }
        }
      }
    }
    __syncthreads();
    read_out(sig, frame0);
    __syncthreads();
    if (!has_next) break;
    sig = nsig;
    jt = njt;
    if constexpr (PASS0_AT_END) tx1024_window_pass0(win_lds, t, xn, twr_unused, vw);
  }
}

// ------------------------------------------------------------------ launch ----
template <typename T>
bool fused_supported(int n_fft) {
  return n_fft >= 64 && n_fft <= 4096 && (n_fft & (n_fft - 1)) == 0;
}

// The launches of one pass of the power-of-two kernels: the ONLY place that decides tile size, launch split and grid.
// launch_one launches what this returns; ssq_stft_plan_launch_info reports it.
template <typename T, int LOGN>
static FusedLaunchShape shape_one(const StftDev<T>& p0, int cu_count, long long batch) {
  using C = FusedCfg<T, LOGN>;
  FusedLaunchShape s;
  int per_cu = (160 * 1024) / C::LDS_BYTES;
  if (per_cu < 1) per_cu = 1;
  if (per_cu * C::W > 32) per_cu = 32 / C::W;
  // fp32 n_fft = 1024 Tx (and its (w, k) hook, SSQ_OUT_WK) runs stft_tx1024_kernel: 16 waves, one block per CU
  // (the generic 8-wave kernel and 8-wave blocks two per CU measured slower: profiles/r01_ab_hiocc.txt,
  // profiles/r01_ab_two_8wave_blocks.txt)
  bool tx1024 = false;
  if constexpr (sizeof(T) == 4 && LOGN == 10) tx1024 = (p0.out_kind == 0 || p0.out_kind == 3) && p0.n_eff == C::N;
  s.tx1024 = tx1024;
  s.split = C::SPLIT;
  const int TF = tx1024 ? Hi1024::F : C::F;   // frames per tile of the kernel that will run
  s.tile_frames = TF;
  // interior tiles [lo, hi): every frame of the tile reads only inside the signal
  const long long span = (long long)TF * p0.hop;
  const int tps_all = (p0.n_frames + TF - 1) / TF;
  long long lo = (p0.pad_left + span - 1) / span;
  long long hi_num = p0.n_signal - C::N - (long long)(TF - 1) * p0.hop + p0.pad_left;
  long long hi = hi_num >= 0 ? hi_num / span + 1 : 0;
  const long long full = p0.n_frames / TF;
  if (hi > full) hi = full;
  if (lo > tps_all) lo = tps_all;
  if (hi < lo) hi = lo;
  // small jobs (a few waves of blocks, e.g. one to four 2^20-sample signals): ONE launch of the edge-capable kernel
  // over all tiles beats two launches -- the second launch costs more than the validity logic of the first
  const long long blocks_one_wave = (long long)cu_count * (tx1024 ? 1 : per_cu);
  bool single_launch = (long long)tps_all * batch <= 4 * blocks_one_wave;   // measured break-even: a few waves
  if (const char* e = std::getenv("SSQ_SINGLE_LAUNCH")) single_launch = std::atoi(e) != 0;   // tests: force either path
  for (int edge = single_launch ? 1 : 0; edge < 2; ++edge) {
    FusedLaunchShape::Launch l;
    l.edge = edge;
    if (single_launch) {
      l.ta0 = 0;
      l.ta_n = tps_all;
      l.tb0 = 0;
      l.tiles_per_signal = tps_all;
    } else if (!edge) {
      l.ta0 = (int)lo;
      l.ta_n = (int)(hi - lo);
      l.tb0 = 0;
      l.tiles_per_signal = l.ta_n;
    } else {
      l.ta0 = 0;
      l.ta_n = (int)lo;
      l.tb0 = (int)hi;
      l.tiles_per_signal = (int)lo + (tps_all - (int)hi);
    }
    l.total_tiles = (long long)l.tiles_per_signal * batch;
    if (l.total_tiles <= 0) continue;
    l.blocks = tx1024 ? (long long)cu_count : (long long)cu_count * per_cu;   // tx1024: one block per CU
    if (l.blocks > l.total_tiles) l.blocks = l.total_tiles;
    s.launch[s.n_launch++] = l;
  }
  return s;
}

template <typename T, int LOGN>
static hipError_t launch_one(const StftDev<T>& p0, int cu_count, long long batch, hipStream_t stream) {
  using C = FusedCfg<T, LOGN>;
  const FusedLaunchShape s = shape_one<T, LOGN>(p0, cu_count, batch);
  const bool tx1024 = s.tx1024;
  for (int i = 0; i < s.n_launch; ++i) {
    const FusedLaunchShape::Launch& l = s.launch[i];
    const int edge = l.edge;
    StftDev<T> p = p0;
    p.ta0 = l.ta0;
    p.ta_n = l.ta_n;
    p.tb0 = l.tb0;
    p.tiles_per_signal = l.tiles_per_signal;
    p.total_tiles = l.total_tiles;
    const dim3 g((unsigned)l.blocks), b(C::W * 64);
    if constexpr (sizeof(T) == 4 && LOGN == 10) {
      if (tx1024) {
        const dim3 gh((unsigned)l.blocks), bh(Hi1024::THREADS);
        // the 16-byte paired read-out needs even n_frames (alignment); the edge and (w, k) kernels stay per-frame
        const bool paired = !edge && p.out_kind == 0 && (p.n_frames & 1) == 0;
        if (p.out_kind == 3) {
          if (edge) hipLaunchKernelGGL((stft_tx1024_kernel<true, false, true>), gh, bh, 0, stream, p);
          else hipLaunchKernelGGL((stft_tx1024_kernel<false, false, true>), gh, bh, 0, stream, p);
        } else if (p.squeezing == 1) {
          if (edge) hipLaunchKernelGGL((stft_tx1024_kernel<true, true>), gh, bh, 0, stream, p);
          else if (paired) hipLaunchKernelGGL((stft_tx1024_kernel<false, true, false, true>), gh, bh, 0, stream, p);
          else hipLaunchKernelGGL((stft_tx1024_kernel<false, true>), gh, bh, 0, stream, p);
        } else {
          if (edge) hipLaunchKernelGGL((stft_tx1024_kernel<true, false>), gh, bh, 0, stream, p);
          else if (paired) hipLaunchKernelGGL((stft_tx1024_kernel<false, false, false, true>), gh, bh, 0, stream, p);
          else hipLaunchKernelGGL((stft_tx1024_kernel<false, false>), gh, bh, 0, stream, p);
        }
        const hipError_t eh = hipGetLastError();
        if (eh != hipSuccess) return eh;
        continue;
      }
    }
    if (p.out_kind == 0 && p.squeezing == 1) {
      if (edge) hipLaunchKernelGGL((stft_fused_kernel<T, LOGN, true, true, true>), g, b, 0, stream, p);
      else hipLaunchKernelGGL((stft_fused_kernel<T, LOGN, true, false, true>), g, b, 0, stream, p);
    } else if (p.out_kind == 0) {
      if (edge) hipLaunchKernelGGL((stft_fused_kernel<T, LOGN, true, true, false>), g, b, 0, stream, p);
      else hipLaunchKernelGGL((stft_fused_kernel<T, LOGN, true, false, false>), g, b, 0, stream, p);
    } else if (p.out_kind == 3) {
      // (w, k) test hook: the Tx epilogue's own bins
      if (edge) hipLaunchKernelGGL((stft_fused_kernel<T, LOGN, true, true, false, true>), g, b, 0, stream, p);
      else hipLaunchKernelGGL((stft_fused_kernel<T, LOGN, true, false, false, true>), g, b, 0, stream, p);
    } else {
      if (edge) hipLaunchKernelGGL((stft_fused_kernel<T, LOGN, false, true, false>), g, b, 0, stream, p);
      else hipLaunchKernelGGL((stft_fused_kernel<T, LOGN, false, false, false>), g, b, 0, stream, p);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <typename T>
int fused_tile_frames(int n_fft) {
  return for_fused_len(n_fft, 0, [](auto L) { return (int)FusedCfg<T, decltype(L)::value>::F; });
}

template <typename T>
hipError_t launch_stft_fused(const StftDev<T>& p, int n_fft, int cu_count, long long batch, hipStream_t stream) {
  if (p.n_eff != n_fft) return launch_stft_anylen<T>(p, n_fft, cu_count, batch, stream);   // stft_anylen.hip
  return for_fused_len(n_fft, hipErrorInvalidValue,
                       [&](auto L) { return launch_one<T, decltype(L)::value>(p, cu_count, batch, stream); });
}

template <typename T>
hipError_t fused_launch_shape(const StftDev<T>& p, int n_fft, int cu_count, long long batch, FusedLaunchShape& shape) {
  if (p.n_eff != n_fft) return anylen_launch_shape<T>(p, n_fft, cu_count, batch, shape);   // stft_anylen.hip
  return for_fused_len(n_fft, hipErrorInvalidValue, [&](auto L) {
    shape = shape_one<T, decltype(L)::value>(p, cu_count, batch);
    return hipSuccess;
  });
}

template bool fused_supported<float>(int);
template bool fused_supported<double>(int);
template int fused_tile_frames<float>(int);
template int fused_tile_frames<double>(int);
template hipError_t launch_stft_fused<float>(const StftDev<float>&, int, int, long long, hipStream_t);
template hipError_t launch_stft_fused<double>(const StftDev<double>&, int, int, long long, hipStream_t);
template hipError_t fused_launch_shape<float>(const StftDev<float>&, int, int, long long, FusedLaunchShape&);
template hipError_t fused_launch_shape<double>(const StftDev<double>&, int, int, long long, FusedLaunchShape&);

}  // namespace ssq
