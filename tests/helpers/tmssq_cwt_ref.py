"""Numpy model of the time-reassigned multisynchrosqueezed CWT (`upstream.tmssq_cwt`) on top of
tests/helpers/tssq_cwt_ref.py (the one-step map) and tests/helpers/tmsst_ref.py (the walk).  No GPU, no library.

Per row i, with t[j] the one-step target column of column j (`tssq_cwt_ref`'s, -1 where the bin is not kept):
    c1[j] = t[j];    c(k+1)[j] = t[ck[j]] if t[ck[j]] >= 0, else ck[j]                          (k = 1 .. n_iter - 1)
    Tx[i, c_n[j]] += Wx[i, j] exp(-2 pi i frac(nu_i (j - c_n[j])))                               kept j"""
from __future__ import annotations

import numpy as np

from . import tssq_cwt_ref as m1
from .cwt_sst2_ref import gmw_wc
from .tmsst_ref import delay_signal, walk


def tmssq_cwt_ref(x, wavelet, scales, dt=1.0, padtype="reflect", order=2, gamma=None, n_iter=4, arith="fft", tabs=None,
                  rdt=np.float64, squeeze=True):
    """-> (W, tau, mm, Tx): W [na, N] complex128 (unrounded); tau the ONE-step map in `rdt` (+inf where a bin is not kept);
    mm int64, the column of Tx each coefficient went to (-1 where not kept); Tx in the complex dtype of `rdt` (None with
    squeeze=False)."""
    rdt = np.dtype(rdt).type
    cdt = np.complex64 if rdt == np.float32 else np.complex128
    W, tau, t1, _ = m1.tssq_cwt_ref(x, wavelet, scales, dt=dt, padtype=padtype, order=order, gamma=gamma, arith=arith,
                                    tabs=tabs, rdt=rdt, squeeze=False)
    mm = walk(t1, n_iter)
    Tx = None
    if squeeze:
        re, im, _, _ = m1.scatter(W.astype(cdt), mm, m1.row_freqs(wavelet, scales))
        Tx = (re.astype(np.float64) + 1j * im.astype(np.float64)).astype(cdt)
    return W, tau, mm, Tx


def table_scales(wavelet, count=160, nv=32):
    """DESIGN 4.22's scales: S0 2^(k / nv), k < count, S0 = wc / pi (the scale whose peak sits at Nyquist)."""
    wc = gmw_wc(float(wavelet[1]), float(wavelet[2])) if wavelet[0] == "gmw" else float(wavelet[1])
    return wc / np.pi * 2.0 ** (np.arange(count) / nv)


def top_cell_share(Tx, nu, lo=0.06, hi=0.40):
    """sum_i max_m |Tx[i, m]|^2 / sum_i sum_m |Tx[i, m]|^2 over the rows with lo < nu_i < hi."""
    nu = np.asarray(nu)
    P = np.abs(Tx[(nu > lo) & (nu < hi)]) ** 2
    return float(P.max(1).sum() / P.sum())


__all__ = ["tmssq_cwt_ref", "table_scales", "top_cell_share", "delay_signal", "walk"]
