// cwt_sst2_wavelets.h -- the analytic wavelets of the second-order synchrosqueezed CWT (cwt_sst2.hip) and
// their derivatives in omega, in fp64, one definition for the kernel that builds the product spectra and for the host
// (`ssq_ssq_cwt2_tables`).  Plain C++ as well as HIP.
//
//   'gmw' (gamma, beta; bandpass norm, order 0)   psih(w)  = 2 exp(-beta ln wc + wc^gamma + beta ln w - w^gamma)   (gmw_l1)
//                                                  psih'(w) = psih(w) (beta / w - gamma w^(gamma - 1)),  both 0 for w <= 0
//   'morlet' (mu)                                  psih(w)  = C (e^{-(w - mu)^2 / 2} - ks e^{-w^2 / 2})            (morlet_up)
//                                                  psih'(w) = C (-(w - mu) e^{-(w - mu)^2 / 2} + ks w e^{-w^2 / 2})
//
// The GMW is evaluated about its peak wc = (beta / gamma)^(1 / gamma), where wc^gamma = beta / gamma: with
// u = ln w - ln wc and e = expm1(gamma u),
//   psih = 2 exp(beta (u - e / gamma))            psih' = -psih beta e / w
// which are the expressions above without their cancellations: the four terms of the exponent are each ~ beta ln w (some
// hundred ulps of the result) and cancel to O(1) over the passband, and beta / w - gamma w^(gamma - 1) crosses zero at
// the peak.  The operator of cwt_sst2.hip is a quotient of differences of products of transforms with these tables, so
// rounding noise on them that differs between host and device would show on every ill-conditioned bin.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SSQ_W2_HD __host__ __device__ __forceinline__
#else
#define SSQ_W2_HD inline
#endif

namespace ssq {

// the constants of one wavelet, formed once on the host (cwt2_wavelet)
struct Cwt2Wavelet {
  int kind;          // SSQ_WAVELET_GMW = 0, SSQ_WAVELET_MORLET = 1
  double gamma, beta, ln_wc;     // GMW
  double mu, C, ks;              // Morlet: C = sqrt(2) cs pi^(1/4), ks = e^{-mu^2 / 2}   (wavelets.py:497-523)
};

inline Cwt2Wavelet cwt2_wavelet(int kind, double p0, double p1) {
  Cwt2Wavelet w{};
  w.kind = kind;
  if (kind == 0) {
    w.gamma = p0;
    w.beta = p1;
    w.ln_wc = (1.0 / p0) * (log(p1) - log(p0));               // _gmw.py:611-657 (morsefreq)
  } else {
    w.mu = p0;
    w.ks = exp(-0.5 * p0 * p0);
    w.C = sqrt(2.0) * pow(1.0 + exp(-p0 * p0) - 2.0 * exp(-0.75 * p0 * p0), -0.5) * pow(3.14159265358979323846, 0.25);
  }
  return w;
}

// psih(w) -> *t0, psih'(w) -> *t1
SSQ_W2_HD void cwt2_psih(const Cwt2Wavelet& wv, double w, double* t0, double* t1) {
  if (wv.kind == 0) {
    if (!(w > 0.0)) {
      *t0 = 0.0;
      *t1 = 0.0;
      return;
    }
    const double u = log(w) - wv.ln_wc;
    const double e = expm1(wv.gamma * u);
    const double psi = 2.0 * exp(wv.beta * (u - e / wv.gamma));
    *t0 = psi;
    *t1 = psi > 0.0 ? -psi * wv.beta * e / w : 0.0;           // (0 * inf past the underflow of psih)
    return;
  }
  const double d = w - wv.mu;
  const double g = exp(-0.5 * d * d), h = wv.ks * exp(-0.5 * w * w);
  *t0 = wv.C * (g - h);
  *t1 = wv.C * (h * w - d * g);
}

// T0(k) = psih(a xi_k), T1(k) = a psih'(a xi_k) on xi_k = 2 pi k / P, k <= P/2, both halved at 2k == P (as upstream
// halves psih there)
SSQ_W2_HD void cwt2_tables_at(const Cwt2Wavelet& wv, double a, long long k, long long P, double* xi, double* T0,
                              double* T1) {
  const double x = 6.283185307179586 * (double)k / (double)P;
  double t0, t1;
  cwt2_psih(wv, a * x, &t0, &t1);
  t1 *= a;
  if (2 * k == P) {
    t0 *= 0.5;
    t1 *= 0.5;
  }
  *xi = x;
  *T0 = t0;
  *T1 = t1;
}

}  // namespace ssq
