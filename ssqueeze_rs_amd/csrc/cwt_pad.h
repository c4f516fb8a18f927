// cwt_pad.h -- the first step of the frequency-domain fp64 CWT pipelines (cwt_sst2.hip, cwt_reassign.hip): the signals
// padded (pad_index.h, no padded real copy) and widened to complex fp64, ready for fft_any_batched's forward transform.
#pragma once
#include <algorithm>

#include "pad_index.h"
#include "ssq_common.h"

namespace ssq {

constexpr int kCwtPadThreads = 256;

// a grid of 256-lane workgroups along `cols`, its y blocks striding over `rows`
inline dim3 cwt_rows_grid(int64_t cols, int64_t rows) {
  return dim3((unsigned)((cols + kCwtPadThreads - 1) / kCwtPadThreads), (unsigned)std::min<int64_t>(rows, 65535));
}

// xh[b][m] = (x[b][pad_index(m - n1)], 0) in fp64, m < P.  grid (ceil(P / 256), min(batch, 65535))
template <typename O>
__global__ __launch_bounds__(kCwtPadThreads) void cwt_pad_kernel(const O* __restrict__ x, cpx<double>* __restrict__ xh,
                                                                 long long batch, long long N, long long P, long long n1,
                                                                 int padtype) {
  const long long m = (long long)blockIdx.x * kCwtPadThreads + threadIdx.x;
  if (m >= P) return;
  const long long src = pad_index(padtype, m - n1, N);
  for (long long b = blockIdx.y; b < batch; b += gridDim.y)
    xh[b * P + m] = {src >= 0 ? (double)x[b * N + src] : 0.0, 0.0};
}

template <typename O>
hipError_t cwt_pad(const O* d_x, cpx<double>* d_xh, int64_t batch, int64_t N, int64_t P, int64_t n1, int padtype,
                   hipStream_t st) {
  hipLaunchKernelGGL((cwt_pad_kernel<O>), cwt_rows_grid(P, batch), dim3(kCwtPadThreads), 0, st, d_x, d_xh, (long long)batch,
                     (long long)N, (long long)P, (long long)n1, padtype);
  return hipGetLastError();
}

}  // namespace ssq
