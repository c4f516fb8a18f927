// fft_passes.h -- the pass tables of the in-register FFTs (fft_core.h), shared by device code and by the host code that
// builds their twiddle tables.  Plain C++ as well as HIP (sst_tables.h includes it without HIP).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SSQ_PASS_HD __host__ __device__
#else
#define SSQ_PASS_HD
#endif

namespace ssq {

// N = 2^LOGN points handled by L = N/16 threads holding E = 16 elements each
// (thread t owns elements t + L*q).  Radix list: 16,16,..., then the remainder.
SSQ_PASS_HD constexpr int num_passes(int logn) { return (logn + 3) / 4; }
SSQ_PASS_HD constexpr int pass_radix(int logn, int p) {
  return (p < logn / 4) ? 16 : (1 << (logn % 4));
}
SSQ_PASS_HD constexpr int pass_ns(int logn, int p) {   // product of earlier radices
  return 1 << (4 * p);
}

}  // namespace ssq
