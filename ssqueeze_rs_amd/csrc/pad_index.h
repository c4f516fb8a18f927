// pad_index.h -- the one index map behind every padded fetch of the input signal, shared by host and device.
//
// Padding here is never a copy: a loader asks for padded position m (any integer; m < 0 lies left of the signal,
// m >= n right of it) and fetches source sample pad_index(padtype, m, n), or takes zero where that is negative.
//   0 reflect    one mirror about the end sample (-m | 2n - 2 - m), zero beyond it   stft_utils.rs:19-65
//   1 zero       zero outside [0, n); any code the table does not know behaves like it
//   2 symmetric  np.pad(mode='symmetric'): period 2n, the end sample repeated
//   3 replicate  np.pad(mode='edge'): clamp(m, 0, n - 1)
//   4 wrap       np.pad(mode='wrap'): m mod n, the non-negative modulo
// Codes 2 and 4 are closed forms: they hold for any pad width, wider than the signal included.
// Plain C++ as well as HIP (the sanitizer harness tests/helpers/pad_index_san.cpp includes it with g++).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SSQ_PAD_HD __host__ __device__ __forceinline__
#else
#define SSQ_PAD_HD inline
#endif

namespace ssq {

enum : int { PAD_REFLECT = 0, PAD_ZERO = 1, PAD_SYMMETRIC = 2, PAD_REPLICATE = 3, PAD_WRAP = 4 };

// m mod period, in [0, period), without a 64-bit division: two conditional add / subtract steps settle every
// -2 period <= m < 3 period (a pad of up to two periods on either side -- a pad is rarely wider than the signal);
// beyond that, behind a branch the loaders of an ordinary geometry never take, one multiply by the fp64 reciprocal and
// one more conditional step.  The quotient estimate is off by at most one while |m / period| < 2^50, so the result is
// exact for every |m| < 2^50.  That branch depends on m, so unlike the one on `padtype` it can split a wave: the lanes
// more than two periods out take it, the others wait.  It holds one fp64 division (the reciprocal of the period), which
// costs nothing where no lane of the wave is that far out.
SSQ_PAD_HD long long pad_fold(long long m, long long period) {
  for (int i = 0; i < 2; ++i) m = m < 0 ? m + period : (m >= period ? m - period : m);
  if (m < 0 || m >= period) {
    m -= (long long)floor((double)m * (1.0 / (double)period)) * period;
    m = m < 0 ? m + period : (m >= period ? m - period : m);
  }
  return m;
}

// Source index in [0, n) of padded position m, or -1 for "zero".  n >= 1.  Codes 0 and 1 are index selects only; the
// branch on `padtype` is uniform over a launch (the one inside pad_fold is not: see there).  NEW_MODES = false compiles codes 0 and 1 alone (every other code pads
// with zeros): the fused STFT kernels, which unroll sixteen fetches per frame in dozens of instantiations and serve
// plans that know those two codes only (api_stft.hip asserts it).
template <bool NEW_MODES = true>
SSQ_PAD_HD long long pad_index(int padtype, long long m, long long n) {
  const bool in = m >= 0 && m < n;
  if (NEW_MODES && padtype >= PAD_SYMMETRIC) {
    if (padtype == PAD_SYMMETRIC) {
      const long long r = pad_fold(m, 2 * n);
      return r < n ? r : 2 * n - 1 - r;
    }
    if (padtype == PAD_REPLICATE) return m < 0 ? 0 : (m < n ? m : n - 1);
    if (padtype == PAD_WRAP) return pad_fold(m, n);
    return in ? m : -1;
  }
  const long long mm = (m < 0) ? -m : (2 * n - 2 - m);
  const bool ok = in || (padtype == PAD_REFLECT && mm >= 0 && mm < n);
  return ok ? (in ? m : mm) : -1;
}

}  // namespace ssq
