// sst_tables.h -- the host tables of the fp64 frame pipeline (stft_frames64.h) that ssq_stft2, tssq_stft and
// reassign_stft share: the five windows, their levelled and packed channels, and the passes' twiddle table, in fp64.
// Pure host C++, no device code and no HIP (tests/helpers/host_math_san.cpp runs it under the CPU sanitizers).  Complex
// tables are interleaved (re, im) pairs, the layout of cpx<double>.
#pragma once
#include "fft_passes.h"
#include "host_math.h"

namespace ssq {
namespace host {

// a power of two a with a * max|tab| within a factor two of `level` (exact to apply and to undo)
inline double level_scale(const std::vector<double>& tab, double level) {
  double m = 0;
  for (double v : tab) m = std::fmax(m, std::fabs(v));
  if (!(m > 0) || !(level > 0) || !std::isfinite(level / m)) return 1.0;
  int e = 0;
  std::frexp(level / m, &e);
  return std::ldexp(1.0, e - 1);
}

// g1 = g', g2 = g'' (spectral derivatives, Nyquist term zeroed), tg = u g, tg1 = u g1 with u = j - n/2, in fp64.
// second = false leaves g2 and tg1 empty (the first-order operators need neither).
struct SstWindows {
  std::vector<double> g1, g2, tg, tg1;
};
inline SstWindows sst_window_tables(const double* window, int64_t n, bool second = true) {
  SstWindows w;
  w.g1 = diff_window(window, n, true);
  if (second) w.g2 = diff_window(w.g1.data(), n, true);
  w.tg.resize((size_t)n);
  if (second) w.tg1.resize((size_t)n);
  for (int64_t j = 0; j < n; ++j) {
    const double u = (double)(j - n / 2);
    w.tg[j] = u * window[j];
    if (second) w.tg1[j] = u * w.g1[j];
  }
  return w;
}

// The channels as the transforms read them, by frame sample j, levelled to max|g| by powers of two a* and packed in
// pairs, and half the inverse scales that the packed split applies (`it` undoes a channel that is transformed alone):
//   kSstSecond     wa = (g, g1 a1)   wb = tg at   wc = (tg1 at1, g2 a2)    h1 = 0.5/a1  it = 1/at    ht1 = 0.5/at1  h2 = 0.5/a2
//   kSstTimeFirst  wa = (g, tg at)   the rest as kSstSecond (not read)     it = 0.5/at: tg is the packed partner of g
//   kSstFirst      wa = (g, g1 a1)   wb = tg at   no wc                    h1 = 0.5/a1  it = 1/at
enum SstPack { kSstSecond, kSstTimeFirst, kSstFirst };
struct SstTables {
  std::vector<double> wa, wb, wc;      // wa, wc: [n][2]
  double h1 = 0, it = 0, ht1 = 0, h2 = 0;
};
inline SstTables sst_level_tables(const double* window, int64_t n, SstPack pack) {
  const bool second = pack != kSstFirst;
  const SstWindows w = sst_window_tables(window, n, second);
  double mg = 0;
  for (int64_t j = 0; j < n; ++j) mg = std::fmax(mg, std::fabs(window[j]));
  const double a1 = level_scale(w.g1, mg), at = level_scale(w.tg, mg);
  SstTables t;
  t.wa.resize(2 * (size_t)n);
  t.wb.resize((size_t)n);
  for (int64_t j = 0; j < n; ++j) {
    t.wa[2 * j] = window[j];
    t.wa[2 * j + 1] = pack == kSstTimeFirst ? w.tg[j] * at : w.g1[j] * a1;
    t.wb[j] = w.tg[j] * at;
  }
  t.h1 = 0.5 / a1;
  t.it = pack == kSstTimeFirst ? 0.5 / at : 1.0 / at;
  if (second) {
    const double a2 = level_scale(w.g2, mg), at1 = level_scale(w.tg1, mg);
    t.wc.resize(2 * (size_t)n);
    for (int64_t j = 0; j < n; ++j) {
      t.wc[2 * j] = w.tg1[j] * at1;
      t.wc[2 * j + 1] = w.g2[j] * a2;
    }
    t.ht1 = 0.5 / at1;
    t.h2 = 0.5 / a2;
  }
  return t;
}

// the passes' twiddle tables [m][k] = exp(-2 pi i k m / (NS R)) of a 2^logn-point transform, passes 1, 2, .. back to
// back (read coalesced by fft_pass_compact), as (re, im) pairs
inline std::vector<double> pass_twiddles(int logn) {
  std::vector<double> tw;
  for (int P = 1; P < num_passes(logn); ++P) {
    const int R = pass_radix(logn, P), NS = pass_ns(logn, P);
    for (int m = 0; m < R; ++m)
      for (int k = 0; k < NS; ++k) {
        const long double ang = 2.0L * 3.14159265358979323846264338327950288L * (long double)((long long)k * m) /
                                (long double)((long long)NS * R);
        tw.push_back((double)cosl(ang));
        tw.push_back((double)(-sinl(ang)));
      }
  }
  return tw;
}

}  // namespace host
}  // namespace ssq
