"""Numpy model of the multisynchrosqueezed STFT (`upstream.mssq_stft`; Yu, Wang and Zhao 2019) on top of
tests/helpers/sst2_ref.py.  No GPU, no library.

Per column, with m[k] the one-step bin of row k (unflipped, -1 where the bin is not kept):
    c1[k] = m[k];    c(i+1)[k] = m[ci[k]] if ci[k] >= 0 and m[ci[k]] >= 0, else ci[k]          (i = 1 .. n_iter - 1)
    Tx[r(c_n[k])] += Sx[k] dw ('sum') or dw / F ('lebesgue'), kept rows ascending;     r(b) = F - 1 - b under flipud, else b
order 2 takes the map of `sst2_ref`; order 1 takes fs |Re w1| (its `details`' re_w1) on every bin."""
from __future__ import annotations

import numpy as np

from tests.helpers import sst2_ref as m2


def walk(m, n_iter):
    """The walk by the definition.  m: integer [..., F, n], targets index axis -2, -1 means no map -> same shape and dtype."""
    m = np.asarray(m)
    cols = np.arange(m.shape[-1])
    lead = np.ix_(*[np.arange(s) for s in m.shape[:-2]]) if m.ndim > 2 else ()
    lead = tuple(a[..., None, None] for a in lead)
    c = m.copy()
    for _ in range(int(n_iter) - 1):
        nxt = m[lead + (np.maximum(c, 0), cols)]
        c = np.where((c >= 0) & (nxt >= 0), nxt, c)
    return c


def bins_of(w, F, fs, rdt):
    """The upstream rule on a frequency map in the dtype `rdt`, unflipped -> int64 bins (-1 where w is inf), dw."""
    Sfs = np.linspace(0, .5 * fs, F)
    dw = rdt(Sfs[1] - Sfs[0])
    with np.errstate(all="ignore"):
        v = np.maximum((w.astype(rdt) - rdt(Sfs[0])) / dw, rdt(0))
        kk = np.minimum(np.rint(v), F - 1)
    kk = np.where(np.isnan(kk), 0, kk).astype(np.int64)
    return np.where(np.isinf(w), -1, kk), dw


def scatter(Sx, bins, dw, squeezing="sum"):
    """Rows-ascending scatter of Sx [F, n] under final rows `bins` (-1: not kept), accumulated in Sx's dtype."""
    F, n = Sx.shape
    cdt = Sx.dtype.type
    rdt = np.float32 if cdt == np.complex64 else np.float64
    add = np.full((F, n), rdt(dw) / rdt(F), dtype=cdt) if squeezing == "lebesgue" else (Sx * rdt(dw)).astype(cdt)
    Tx = np.zeros((F, n), dtype=cdt)
    cols = np.arange(n)
    for i in range(F):
        k = bins[i] >= 0
        Tx[bins[i, k], cols[k]] += add[i, k]
    return Tx


def mssq_stft_ref(x, window, n_fft, hop_len=1, fs=1.0, padtype="reflect", modulated=True, squeezing="sum", gamma=None,
                  flipud=False, order=2, n_iter=4, arith="fft", dtype=np.complex128, tables=None):
    """-> (V, w, bins, Tx): V [F, n_frames] in `dtype`; w the one-step frequency map (inf where a bin is not kept); bins
    int64, the row of Tx each coefficient went to (-1 where not kept); Tx in `dtype`."""
    cdt = np.dtype(dtype).type
    rdt = np.float32 if cdt == np.complex64 else np.float64
    V, w2, _, _, det = m2.sst2_ref(x, window, n_fft, hop_len=hop_len, fs=fs, padtype=padtype, modulated=modulated,
                                   squeezing=squeezing, gamma=gamma, flipud=False, arith=arith, dtype=dtype, details=True,
                                   tables=tables)
    F = V.shape[0]
    if order == 2:
        w = w2
    elif order == 1:
        w = np.where(det["keep"], rdt(fs) * np.abs(det["re_w1"].astype(rdt)), rdt(np.inf)).astype(rdt)
    else:
        raise ValueError(order)
    m, dw = bins_of(w, F, fs, rdt)
    c = walk(m, n_iter)
    bins = np.where(c >= 0, F - 1 - c, -1) if flipud else c
    return V, w, bins, scatter(V, bins, dw, squeezing)


def fm_signal(N=1024, f0=0.25, depth=0.15, cycles=3):
    """cos of the phase whose instantaneous frequency is f0 + depth sin(2 pi cycles t / N) cycles/sample, and that fi."""
    t = np.arange(N, dtype=np.float64)
    fi = f0 + depth * np.sin(2 * np.pi * cycles * t / N)
    phase = 2 * np.pi * (f0 * t - depth * N / (2 * np.pi * cycles) * (np.cos(2 * np.pi * cycles * t / N) - 1))
    return np.cos(phase), fi


def top_cell_share(Tx, n_fft):
    """The share of each column's |Tx|^2 that sits in the column's largest cell, over columns n_fft .. N - n_fft."""
    P = np.abs(Tx[:, n_fft:Tx.shape[1] - n_fft]) ** 2
    return float(P.max(0).sum() / P.sum())
