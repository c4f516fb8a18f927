"""Numpy model of the time-reassigned multisynchrosqueezed STFT (`upstream.tmssq_stft`; Yu, Lin, Ma and He
2020) on top of tests/helpers/tsst_ref.py.  No GPU, no library.

Per row, with t[m] the one-step target frame of frame m (`tsst_ref`'s, -1 where the bin is not kept):
    c1[m] = t[m];    c(i+1)[m] = t[ci[m]] if t[ci[m]] >= 0, else ci[m]                          (i = 1 .. n_iter - 1)
    Tx[k, c_n[m]] += V[k, m] exp(-2 pi i ((k (m - c_n[m]) hop) mod n) / n)                      kept m, ascending source frame"""
from __future__ import annotations

import numpy as np

from tests.helpers import tsst_ref as m1


def walk(t, n_iter):
    """The walk by the definition.  t: integer [..., n], targets index the last axis, -1 means none -> same shape and dtype."""
    t = np.asarray(t)
    c = t.copy()
    for _ in range(int(n_iter) - 1):
        nxt = np.take_along_axis(t, np.maximum(c, 0), axis=-1)
        c = np.where((c >= 0) & (nxt >= 0), nxt, c)
    return c


def tmsst_ref(x, window, n_fft, hop_len=1, fs=1.0, padtype="reflect", modulated=True, order=2, gamma=None, n_iter=4,
              arith="fft", dtype=np.complex128, tables=None):
    """-> (V, tau, tgt, Tx): V [F, n_frames] in `dtype`; tau the ONE-step map (+inf where a bin is not kept); tgt int64,
    the frame of Tx each coefficient went to (-1 where not kept); Tx in `dtype`."""
    V, tau, t1, _ = m1.tsst_ref(x, window, n_fft, hop_len=hop_len, fs=fs, padtype=padtype, modulated=modulated, order=order,
                                gamma=gamma, arith=arith, dtype=dtype, tables=tables, squeeze=False)
    tgt = walk(t1, n_iter)
    keep = tgt >= 0
    return V, tau, tgt, m1.scatter(V, np.maximum(tgt, 0), keep, int(hop_len), int(n_fft), np.dtype(dtype).type)


def delay_signal(N=1024, centre=512.0, depth=150.0, cycles=4):
    """The signal of DESIGN 4.21's table: X(f) = exp(-i phi(f)) on rfftfreq(N) with group delay
    phi'(f) / (2 pi) = centre + depth sin(2 pi cycles f) samples, X[0] = X[N/2] = 0, x = irfft(X) sqrt(N) -> x, the delay."""
    f = np.fft.rfftfreq(N)
    w = 2 * np.pi * cycles
    phi = 2 * np.pi * (centre * f - depth / w * (np.cos(w * f) - 1))
    X = np.exp(-1j * phi)
    X[0] = X[-1] = 0
    return np.fft.irfft(X, N) * np.sqrt(N), centre + depth * np.sin(w * f)


def top_cell_share(Tx, lo=0.06, hi=0.44):
    """sum_k max_m |Tx[k, m]|^2 / sum_k sum_m |Tx[k, m]|^2 over the rows with lo < k / n < hi."""
    F = Tx.shape[0]
    fr = np.arange(F) / (2.0 * (F - 1))
    P = np.abs(Tx[(fr > lo) & (fr < hi)]) ** 2
    return float(P.max(1).sum() / P.sum())
