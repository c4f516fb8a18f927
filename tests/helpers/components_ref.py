"""NumPy restatement of upstream's component inversion (old/ssqueezepy/_ssq_cwt.py:381-417, `_invert_components` and
`_process_component_inversion_args`), the oracle of the GPU kernel in issq_components.hip.

TEST INFRASTRUCTURE ONLY.  It keeps upstream's dtypes: the curves are int32 (so `cc - cw` and `cc + cw` wrap as
int32 sums do), every component is summed in float64, and the remainder is summed in the real dtype of `Tx` (upstream
sums it from a copy of `Tx`, complex64 for complex64 input).  The result is float64 [K + 1, N], unscaled.
"""
from __future__ import annotations

import numpy as np


def curves(cc, cw):
    """A 1-D curve array is one curve (a column); both are cast with astype('int32'), floats truncating toward 0."""
    cc, cw = np.asarray(cc), np.asarray(cw)
    cc = cc[:, None] if cc.ndim == 1 else cc
    cw = cw[:, None] if cw.ndim == 1 else cw
    return cc.astype(np.int32), cw.astype(np.int32)


def band_edges(c, w, F):
    """First and last row of each column's band: both ends clipped to [0, F]; a centre of exactly -1 means no curve in
    that column, which upstream encodes as the empty range first = 1, last = 0.  Other negative centres are ordinary."""
    first = np.clip(c - w, 0, F)
    last = np.clip(c + w, 0, F)
    absent = c == -1
    return np.where(absent, 1, first), np.where(absent, 0, last)


def band_mask(c, w, F):
    """[F, N] bool: row r of column m is in the band iff first <= r <= last; rows stop at F - 1, as a slice does."""
    first, last = band_edges(c, w, F)
    r = np.arange(F)[:, None]
    return (r >= first[None, :]) & (r <= last[None, :])


def invert_components(Tx, cc, cw):
    """-> float64 [K + 1, N]: rows 0 .. K-1 the sums of Re Tx over each curve's band (overlaps count in every band),
    row K the sum over the rows that no band covers."""
    cc, cw = curves(cc, cw)
    F, N = Tx.shape
    K = cc.shape[1]
    re = np.real(Tx)
    out = np.zeros((K + 1, N), dtype=np.float64)
    covered = np.zeros((F, N), dtype=bool)
    for k in range(K):
        m = band_mask(cc[:, k], cw[:, k], F)
        out[k] = np.where(m, re.astype(np.float64), 0.0).sum(axis=0)
        covered |= m
    out[K] = np.where(covered, re.dtype.type(0), re).sum(axis=0)
    return out


def issq_cwt(Tx, cc, cw, adm):
    """issq_cwt's component path: the inversion times 2 / adm_ssq(wavelet)."""
    x = invert_components(Tx, cc, cw)
    x *= 2 / adm
    return x


def issq_stft(Tx, cc, cw, window):
    """issq_stft's component path: the inversion times 2 / window[len(window) // 2]."""
    x = invert_components(Tx, cc, cw)
    x *= 2 / window[len(window) // 2]
    return x
