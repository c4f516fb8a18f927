// issq_components.hip -- component inversion of a synchrosqueezed transform: upstream ssqueezepy's
// issq_cwt / issq_stft with curve centres cc and half-widths cw (old/ssqueezepy/_ssq_cwt.py:381-417,
// `_invert_components` and `_process_component_inversion_args`).
//
// For signal b, column j and component k the band is the rows lo .. hi of
//   lo = clip(cc - cw, 0, F), hi = clip(cc + cw, 0, F)   (int32 arithmetic, as numpy's on astype('int32') arrays)
// cut at F - 1 like a Python slice, and empty where cc == -1 (upstream sets lo = 1, hi = 0 there).
//   x[b][k][j] = scale * sum_{rows in band k} Re Tx[b][row][j]                       (bands may overlap)
//   x[b][K][j] = scale * sum_{rows in no band} Re Tx[b][row][j]                      (the remainder)
// Everything accumulates in fp64 for both dtypes.
//
// Kernel shape: a block is 64 lanes along the columns (each lane CPL adjacent columns, so one wave reads a row's
// 64 * CPL complex values contiguously) by W waves that split the rows into W contiguous ranges.  A lane holds the
// bands of one register tile of KT components and adds every row's real part to each component whose band holds the
// row (a predicated add, no branch on data).  The waves' partial sums meet in LDS and wave 0 adds them in wave order,
// so the result depends only on (F, W) and not on the batch or the launch: identical run to run.  W is a function
// of F alone.  More than kTile components: grid.z runs the tiles (each block re-reads its Tx columns); the tile-0
// blocks also sum the remainder, whose row coverage they build per 32-row segment as a bit mask from all K bands.
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/ssq_hip.h"
#include "dev_buffers.h"

using namespace ssq;

namespace {

constexpr int kTile = 8;           // components per register tile
constexpr int kMaxWaves = 8;       // waves per block splitting a column's rows
constexpr int kRowsPerWave = 32;   // W = clamp(F / 32, 1, 8)
constexpr int kUnroll = 8;         // rows loaded before they are summed
constexpr int64_t kMaxComp = (int64_t)65535 * kTile;

// One band as (lo, span): row r is in it iff (unsigned)(r - lo) <= span.  An empty band has lo = F, which no row
// r < F reaches (r - F < 0 wraps above any span).
struct Band {
  int lo;
  unsigned span;
};

__device__ __forceinline__ Band band_of(int64_t ccv, int64_t cwv, int F) {
  const int c = (int)(unsigned)(uint64_t)ccv;             // astype('int32'): the low 32 bits
  const int w = (int)(unsigned)(uint64_t)cwv;
  const int up = (int)((unsigned)c + (unsigned)w);        // int32 sums wrap as numpy's do
  const int dn = (int)((unsigned)c - (unsigned)w);
  const int lo = min(max(dn, 0), F);
  const int hi = min(min(max(up, 0), F), F - 1);          // the slice lo:hi+1 stops at F
  Band b;
  const bool empty = c == -1 || lo > hi;
  b.lo = empty ? F : lo;
  b.span = empty ? 0u : (unsigned)(hi - lo);
  return b;
}

// the real parts of a lane's CPL columns in one row, as fp64; one load of 8 * CPL (fp32) or 16 bytes (fp64)
template <typename T, int CPL>
struct RowLoad;
template <>
struct RowLoad<float, 1> {
  __device__ static void load(const float* p, double* re) { re[0] = (double)reinterpret_cast<const float2*>(p)->x; }
};
template <>
struct RowLoad<float, 2> {
  __device__ static void load(const float* p, double* re) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    re[0] = (double)v.x;
    re[1] = (double)v.z;
  }
};
template <>
struct RowLoad<double, 1> {
  __device__ static void load(const double* p, double* re) { re[0] = reinterpret_cast<const double2*>(p)->x; }
};

// Tx [B][F][N] interleaved complex; cc, cw [B][N][K] int64 (cw NULL: cw_const); x [B][K+1][N] float64.
// grid (ceil(N / (64 CPL)), min(B, 65535), n_tiles), block (64, W).  ALLK: every component is in this one tile, so
// the remainder's coverage is the OR of the tile's own predicates.
template <typename T, int CPL, int KT, bool ALLK>
__global__ __launch_bounds__(64 * kMaxWaves) void issq_components_kernel(
    const T* __restrict__ Tx, long long B, int F, long long N, const int64_t* __restrict__ cc,
    const int64_t* __restrict__ cw, long long cw_const, int K, double scale, double* __restrict__ x) {
  __shared__ double red[kMaxWaves][64 * CPL];
  const int lane = threadIdx.x, wave = threadIdx.y, W = blockDim.y;
  const long long j0 = ((long long)blockIdx.x * 64 + lane) * CPL;
  const bool live = j0 < N;                              // N % CPL == 0 when CPL > 1: a lane has all or none
  const int k0 = blockIdx.z * KT;
  const int kc = min(KT, K - k0);
  const bool do_rem = blockIdx.z == 0;
  const int R = (F + W - 1) / W;
  const int r0 = min(F, wave * R), r1 = min(F, r0 + R);

  for (long long b = blockIdx.y; b < B; b += gridDim.y) {
    Band bd[CPL][KT];
#pragma unroll
    for (int c = 0; c < CPL; ++c)
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        bd[c][k].lo = F;
        bd[c][k].span = 0u;
        if (live && k < kc) {
          const long long o = (b * N + j0 + c) * K + k0 + k;
          bd[c][k] = band_of(cc[o], cw ? cw[o] : cw_const, F);
        }
      }
    double acc[CPL][KT], rem[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      rem[c] = 0.0;
#pragma unroll
      for (int k = 0; k < KT; ++k) acc[c][k] = 0.0;
    }
    const T* base = Tx + ((b * F) * N + j0) * 2;
    for (int s = r0; s < r1; s += 32) {                  // 32-row segments: the remainder's coverage mask
      const int se = min(s + 32, r1);
      unsigned cover[CPL];
#pragma unroll
      for (int c = 0; c < CPL; ++c) cover[c] = 0u;
      if (!ALLK && do_rem && live) {
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int c = 0; c < CPL; ++c) {
            const long long o = (b * N + j0 + c) * K + k;
            const Band q = band_of(cc[o], cw ? cw[o] : cw_const, F);
            const int a = max(q.lo, s);
            const int e = min(q.lo + (int)q.span, se - 1);
            const int n = e - a + 1;                     // rows of this band inside the segment
            const unsigned long long m = n > 0 ? ((1ull << n) - 1ull) << (a - s) : 0ull;
            cover[c] |= (unsigned)m;
          }
      }
      for (int r = s; r < se; r += kUnroll) {
        double v[kUnroll][CPL];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          if (live && r + u < se) {
            RowLoad<T, CPL>::load(base + (long long)(r + u) * N * 2, v[u]);
          } else {
#pragma unroll
            for (int c = 0; c < CPL; ++c) v[u][c] = 0.0;
          }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int row = r + u;
          const bool in = row < se;
#pragma unroll
          for (int c = 0; c < CPL; ++c) {
            bool cov = false;
#pragma unroll
            for (int k = 0; k < KT; ++k) {
              const bool p = in && (unsigned)(row - bd[c][k].lo) <= bd[c][k].span;
              acc[c][k] += p ? v[u][c] : 0.0;
              cov = cov || p;
            }
            if (do_rem) {
              const bool covered = ALLK ? cov : ((cover[c] >> (row - s)) & 1u) != 0u;
              rem[c] += (in && !covered) ? v[u][c] : 0.0;
            }
          }
        }
      }
    }
    // the waves' partials, one quantity at a time, summed by wave 0 in wave order
    const int nq = kc + (do_rem ? 1 : 0);
#pragma unroll
    for (int q = 0; q < KT + 1; ++q) {
      if (q >= nq) continue;                               // uniform over the block
      const bool is_rem = q == kc;
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        double val = rem[c];
#pragma unroll
        for (int k = 0; k < KT; ++k)
          if (k == q && !is_rem) val = acc[c][k];       // q == kc < KT is the remainder, not slot kc
        red[wave][lane * CPL + c] = val;
      }
      __syncthreads();
      if (wave == 0 && live) {
        const long long row_out = b * (K + 1) + (is_rem ? K : k0 + q);
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
          double t = red[0][lane * CPL + c];
          for (int w = 1; w < W; ++w) t += red[w][lane * CPL + c];
          x[row_out * N + j0 + c] = t * scale;
        }
      }
      __syncthreads();
    }
  }
}

template <typename T, int CPL, int KT, bool ALLK>
void launch_typed(dim3 grid, dim3 block, hipStream_t st, const void* Tx, int64_t B, int F, int64_t N,
                  const int64_t* cc, const int64_t* cw, int64_t cw_const, int K, double scale, double* x) {
  hipLaunchKernelGGL((issq_components_kernel<T, CPL, KT, ALLK>), grid, block, 0, st, static_cast<const T*>(Tx),
                     (long long)B, F, (long long)N, cc, cw, (long long)cw_const, K, scale, x);
}

template <typename T, int CPL>
void launch_tile(int K, dim3 grid, dim3 block, hipStream_t st, const void* Tx, int64_t B, int F, int64_t N,
                 const int64_t* cc, const int64_t* cw, int64_t cw_const, double scale, double* x) {
  // the smallest register tile that holds every component; above kTile, tiles of kTile over grid.z
  if (K == 1) launch_typed<T, CPL, 1, true>(grid, block, st, Tx, B, F, N, cc, cw, cw_const, K, scale, x);
  else if (K == 2) launch_typed<T, CPL, 2, true>(grid, block, st, Tx, B, F, N, cc, cw, cw_const, K, scale, x);
  else if (K <= 4) launch_typed<T, CPL, 4, true>(grid, block, st, Tx, B, F, N, cc, cw, cw_const, K, scale, x);
  else if (K <= kTile) launch_typed<T, CPL, kTile, true>(grid, block, st, Tx, B, F, N, cc, cw, cw_const, K, scale, x);
  else launch_typed<T, CPL, kTile, false>(grid, block, st, Tx, B, F, N, cc, cw, cw_const, K, scale, x);
}

int check_args(int dtype, int64_t batch, int64_t rows, int64_t cols, int64_t n_comp) {
  if (dtype != SSQ_F32 && dtype != SSQ_F64) SSQ_FAIL("dtype must be SSQ_F32 or SSQ_F64");
  if (batch < 1 || batch > INT32_MAX) SSQ_FAIL("batch must be in [1, 2^31)");
  if (rows < 1 || rows > INT32_MAX - 64) SSQ_FAIL("rows must be in [1, 2^31 - 64)");
  if (cols < 1) SSQ_FAIL("cols must be >= 1");
  if (n_comp < 1 || n_comp > kMaxComp) SSQ_FAIL("n_comp must be in [1, 524280]");
  if ((double)batch * (double)rows * (double)cols * 16.0 > 9.0e18 || (double)batch * (double)cols * (double)(n_comp + 1) * 8.0 > 9.0e18)
    SSQ_FAIL("Tx too large");
  return 0;
}

bool fits_int32(int64_t v) { return v >= INT32_MIN && v <= INT32_MAX; }

}  // namespace

extern "C" {

int ssq_issq_components_exec(int dtype, const void* d_Tx, int64_t batch, int64_t rows, int64_t cols,
                             const int64_t* d_cc, const int64_t* d_cw, int64_t cw_const, int64_t n_comp, double scale,
                             double* d_x, void* stream) {
  if (int rc = check_args(dtype, batch, rows, cols, n_comp)) return rc;
  if (!d_Tx || !d_cc || !d_x) SSQ_FAIL("NULL argument");
  if (!d_cw && !fits_int32(cw_const)) SSQ_FAIL("|cw_const| must be below 2^31");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int F = (int)rows, K = (int)n_comp;
  const int W = std::min(kMaxWaves, std::max(1, F / kRowsPerWave));
  // two columns per lane (16-byte loads) for fp32 when the rows stay 16-byte aligned and the grid still has two
  // blocks per CU; this changes no arithmetic, so the choice may depend on the batch
  int cus = 256, dev = 0;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  const bool wide = dtype == SSQ_F32 && cols % 2 == 0 && (reinterpret_cast<uintptr_t>(d_Tx) % 16) == 0 &&
                    ((cols + 127) / 128) * batch >= 2 * (int64_t)cus;
  const int cpl = wide ? 2 : 1;
  const int64_t tiles = (cols + 64 * cpl - 1) / (64 * cpl);
  if (tiles > INT32_MAX) SSQ_FAIL("cols too large");
  const int n_tiles = K <= kTile ? 1 : (K + kTile - 1) / kTile;
  const dim3 grid((unsigned)tiles, (unsigned)std::min<int64_t>(batch, 65535), (unsigned)n_tiles);
  const dim3 block(64, (unsigned)W);
  if (dtype == SSQ_F64)
    launch_tile<double, 1>(K, grid, block, st, d_Tx, batch, F, cols, d_cc, d_cw, cw_const, scale, d_x);
  else if (wide)
    launch_tile<float, 2>(K, grid, block, st, d_Tx, batch, F, cols, d_cc, d_cw, cw_const, scale, d_x);
  else
    launch_tile<float, 1>(K, grid, block, st, d_Tx, batch, F, cols, d_cc, d_cw, cw_const, scale, d_x);
  SSQ_HIP(hipGetLastError());
  return 0;
}

int ssq_issq_components_host(int dtype, const void* Tx, int64_t batch, int64_t rows, int64_t cols, const int64_t* cc,
                             const int64_t* cw, int64_t cw_const, int64_t n_comp, double scale, double* x_out) {
  if (int rc = check_args(dtype, batch, rows, cols, n_comp)) return rc;
  if (!Tx || !cc || !x_out) SSQ_FAIL("NULL argument");
  const size_t nb = (size_t)(batch * cols * n_comp);
  for (size_t i = 0; i < nb; ++i)
    if (!fits_int32(cc[i])) SSQ_FAIL("|cc| must be below 2^31");
  if (cw) {
    for (size_t i = 0; i < nb; ++i)
      if (!fits_int32(cw[i])) SSQ_FAIL("|cw| must be below 2^31");
  } else if (!fits_int32(cw_const)) {
    SSQ_FAIL("|cw_const| must be below 2^31");
  }
  if (int rc = require_device()) return rc;
  const size_t tx_bytes = (size_t)(batch * rows * cols) * (dtype == SSQ_F64 ? 16 : 8);
  const size_t x_bytes = (size_t)(batch * (n_comp + 1) * cols) * sizeof(double);
  DeviceBufs d;
  void *dT, *dcc, *dcw = nullptr, *dx;
  SSQ_HIP(d.upload(&dT, Tx, tx_bytes));
  SSQ_HIP(d.upload(&dcc, cc, nb * sizeof(int64_t)));
  if (cw) SSQ_HIP(d.upload(&dcw, cw, nb * sizeof(int64_t)));
  SSQ_HIP(d.alloc(&dx, x_bytes));
  if (int rc = ssq_issq_components_exec(dtype, dT, batch, rows, cols, static_cast<const int64_t*>(dcc),
                                        static_cast<const int64_t*>(dcw), cw_const, n_comp, scale, static_cast<double*>(dx),
                                        nullptr))
    return rc;
  SSQ_HIP(hipMemcpy(x_out, dx, x_bytes, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
