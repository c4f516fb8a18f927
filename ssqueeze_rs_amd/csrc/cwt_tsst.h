// cwt_tsst.h -- what cwt_tsst.hip lends to cwt_tmsst.hip: the parameter blocks of its kernels, the argument
// checks and the shape, and the two halves of the pipeline on device buffers (the operator part: the chunked maps with
// cwt_tsst_operator_kernel writing the int32 one-step plane; the scatter with its read-out).  The kernels and the host
// code are compiled once, in cwt_tsst.hip, for float and double; this header only declares them.
#pragma once
#include <cstdint>

#include "cwt_maps64.h"

namespace ssq {

constexpr int kCwtTQuantumBitsMax = 38;                       // upstream.TSSQ_CWT_QUANTUM_LOG2_MAX

constexpr unsigned cwt_tsst_map_set(int order) { return order == 2 ? kMapsAll : kMapW | kMapWt; }
constexpr int cwt_tsst_maps(int order) { return cwt_map_count(cwt_tsst_map_set(order)); }

template <typename O>
struct CwtTOpDev {
  const cpx<double>* maps;   // [rows][maps][P]: the unnormalised inverse transforms
  const double* nu;          // [na]: the rows' frequencies, cycles/sample
  cpx<O>* Wx;                // [batch * na][N], these three at the chunk's first row
  O* tau;                    // or nullptr
  int* mm;
  unsigned long long* emax;  // [batch]: bit pattern of max |Wx|^2, zeroed before the first chunk
  long long P, N, n1, r0, rows;
  int na;
  double inv_P, gamma, gamma_sq, dt;
  O dt_o;                    // dt in the call's dtype: the time rule runs on the tau the call reports
};

template <typename O>
struct CwtTScatDev {
  const cpx<O>* Wx;                  // [batch][na][N]
  const int* mm;                     // [batch][na][N]: target column, -1 where the bin is not kept
  const double* nu;                  // [na]
  const unsigned long long* emax;    // [batch]
  unsigned long long* acc;           // [batch][na][N][2]: the fixed-point cells, zeroed before the scatter
  cpx<O>* Tx;                        // [batch][na][N]
  long long batch, plane, N;         // plane = na N <= 2^40
  int qbits;
};

struct CwtTCall : CwtMapsCall {
  int order;
  const double* nu;
};

inline const char* cwtt_order_fail(int order) { return order != 1 && order != 2 ? "order must be 1 or 2" : nullptr; }

// Every argument check of an entry point of kind `k` and the shape it works on (sets the error and returns non-zero;
// nothing here touches the GPU).  own_fail: the message of the entry point's own checks (order, n_iter), or nullptr.
int cwtt_check(const CwtMapsKind& k, const char* own_fail, const CwtTCall& c, CwtMapsShape* s);

// The head of a workspace of either kind is cwt_maps64.h's cwt_head: the signals' maxima, the accumulators [cells][2] and
// behind them the int32 planes [cells] of the kind (tssq_cwt: one; tmssq_cwt: two).

// c.scales and c.nu on the device, held by `d`
int cwtt_tables(DeviceBufs& d, const CwtTCall& c, void** d_scales, void** d_nu);

// The operator part on device buffers, asynchronous on c.st: zeroes the maxima and the accumulators at the head of
// d_work, then walks the chunks (s.work_bytes sets the rows per chunk) with cwt_tsst_operator_kernel: Wx, tau (d_tau may
// be nullptr) and the int32 one-step plane `mm`, -1 where a bin is not kept.
template <typename T>
int cwtt_operator_run(const CwtTCall& c, const CwtMapsShape& s, const void* d_x, const void* d_scales, const void* d_nu,
                      void* d_Wx, void* d_tau, int* mm, void* d_work);

// The scatter of Wx under the plane `mm` into the accumulators at the head of d_work, and the read-out into every cell of
// Tx; asynchronous on c.st.  mid (may be nullptr): an event recorded between the two kernels.
template <typename T>
int cwtt_scatter_run(const CwtTCall& c, const CwtMapsShape& s, const void* d_nu, const void* d_Wx, const int* mm,
                     void* d_work, void* d_Tx, hipEvent_t mid);

}  // namespace ssq
