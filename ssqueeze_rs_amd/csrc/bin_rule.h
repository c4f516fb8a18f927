// bin_rule.h -- upstream's rule that takes a frequency w to a row of ssq_freqs, for the kernels that run it on a w they
// hold (ssqueeze.hip, cwt_reassign.hip): the parameter block, the device function and the host builder.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/ssq_hip.h"
#include "ssq_common.h"

namespace ssq {

// the bin rule of algos.py for a finite w: clamped round-half-even on 'log' / 'linear' frequencies (:173-180,
// :231-239), the two-segment map on 'log-piecewise' ones (:196-209); NaN lands in row 0, as in the fused kernels
template <typename T>
struct BinRule {
  T bin_min, bin_step;       // log2 f[0], log2 f[1] - log2 f[0]  (linear: f[0], f[1] - f[0])
  T vlmin1, dvl1;            // log-piecewise: the second segment (algos.py:364-370)
  int idx1;
  int kind;                  // SSQ_FREQS_*
  int omax;                  // rows - 1
  int flipud;
};

template <typename T>
__device__ __forceinline__ int bin_of(const BinRule<T>& r, T w) {
  int bin;
  if (r.kind == SSQ_FREQS_LOG_PIECEWISE) {
    const T wl = log2(w);
    T v;
    if (wl > r.vlmin1) v = rint((wl - r.vlmin1) / r.dvl1) + (T)r.idx1;
    else v = rint(fmax((wl - r.bin_min) / r.bin_step, (T)0));
    bin = (v >= (T)r.omax) ? r.omax : (v == v ? (int)v : 0);
  } else {
    const T v = fmax(((r.kind == SSQ_FREQS_LOG ? log2(w) : w) - r.bin_min) / r.bin_step, (T)0);
    bin = (v >= (T)r.omax) ? r.omax : (int)rint(v);
    if (!(v == v)) bin = 0;
  }
  return r.flipud ? (r.omax - bin) : bin;
}

// algos.py:341-370 (`_get_params_find_closest_log`, `_ensure_nonzero_nonnegative`) and :84-90 in fp64, as
// ssq_bin_params (api_cwt.hip) sets up the fused kernels (sets the error and returns non-zero)
template <typename T>
int bin_rule(const double* f, int64_t rows, int kind, int64_t idx, int flipud, BinRule<T>& r) {
  if (!f) SSQ_FAIL("ssq_freqs_asc is NULL");
  if (rows < 2) SSQ_FAIL("ssqueeze needs at least 2 rows");
  if (kind != SSQ_FREQS_LOG && kind != SSQ_FREQS_LINEAR && kind != SSQ_FREQS_LOG_PIECEWISE)
    SSQ_FAIL("freq_kind must be SSQ_FREQS_LOG, _LINEAR or _LOG_PIECEWISE");
  std::memset(&r, 0, sizeof(r));
  const bool lg = kind != SSQ_FREQS_LINEAR;
  const double vmin = lg ? std::log2(f[0]) : f[0];
  double dv = lg ? std::log2(f[1]) - std::log2(f[0]) : f[1] - f[0];
  if (kind == SSQ_FREQS_LOG_PIECEWISE) {
    if (idx < 2 || idx > rows - 1) SSQ_FAIL("freq_transition must be 2 .. rows-1 for SSQ_FREQS_LOG_PIECEWISE");
    r.idx1 = (int)idx - 1;
    r.vlmin1 = (T)std::log2(f[idx - 1]);
    r.dvl1 = (T)std::max(std::log2(f[idx]) - std::log2(f[idx - 1]), 2.220446049250313e-16);
    dv = std::max(dv, 2.220446049250313e-16);
  }
  r.bin_min = (T)vmin;
  r.bin_step = (T)dv;
  r.kind = kind;
  r.omax = (int)rows - 1;
  r.flipud = flipud ? 1 : 0;
  return 0;
}

}  // namespace ssq
