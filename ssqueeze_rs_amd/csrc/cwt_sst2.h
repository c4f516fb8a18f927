// cwt_sst2.h -- what cwt_sst2.hip lends to cwt_msst.hip: the call struct and the argument checks of
// ssq_cwt2, the call's tables on the device, and the two halves of the pipeline on device buffers (the operator half:
// cwt_maps64.h's pipeline through cwt2_operator_kernel; the squeeze half: ssq_ssqueeze_w_exec).  The kernel and the host
// code are compiled once, in cwt_sst2.hip, for float and double; this header only declares them.
#pragma once
#include <cstdint>

#include "cwt_maps64.h"

namespace ssq {

constexpr int kCwt2Maps = cwt_map_count(kMapsAll);            // W, W1, W2, Wt, Wt1

struct Cwt2Call : CwtMapsCall {
  int freq_kind, squeezing, variant;
  int64_t freq_transition;
  const double *row_const, *f_asc;
};

// Every argument check of the entry points (sets the error and returns non-zero; nothing here touches the GPU).  k: the
// entry point's messages and limits; own_fail: the message of its own argument check that failed, or nullptr.
int cwt2_check(const CwtMapsKind& k, const char* own_fail, const Cwt2Call& c, CwtMapsShape* s);

// the call's tables on the device (held by `d`): the scales in fp64 and the row weights in the call's dtype
template <typename T>
int cwt2_tables(DeviceBufs& d, const Cwt2Call& c, void** d_scales, void** d_rc);

// The operator half on device buffers: Wx and the one-step frequency, [batch][na][N] in the call's dtype, in the
// workspace d_work of s.work_bytes behind its head.  gamma_sq: the second-order estimate is used where |D| > gamma_sq
// (ssq_cwt2: gamma^2; +inf, mssq_cwt's order 1: nowhere, so every element reports |Im om1| / (2 pi dt)).  Asynchronous
// on c.st.
template <typename T>
int cwt2_operator_run(const Cwt2Call& c, const CwtMapsShape& s, double gamma_sq, const void* d_x, const void* d_scales,
                      void* d_Wx, void* d_w2, void* d_work);

// The squeeze half: Tx = ssqueeze(Wx, w) by ssq_ssqueeze_w_exec (Tx zeroed there; the flip is applied there).
// Asynchronous on c.st.
int cwt2_squeeze_run(const Cwt2Call& c, const void* d_Wx, const void* d_w, const void* d_rc, void* d_Tx);

}  // namespace ssq
