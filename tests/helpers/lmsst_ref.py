"""Numpy model of the local maximum synchrosqueezing transforms (`upstream.lmssq_stft`, `upstream.lmssq_cwt`,
`upstream.lmsst_rows`; Yu, Wang, Zhao and Liu 2019) on top of tests/helpers/sst2_ref.py and
msst_ref.py.  No GPU, no library.

Per column, with R rows and an int delta >= 1:
    A[k] = re^2 + im^2 of the coefficient as the call reports it (in the call's dtype), evaluated in fp64
    m[k] = the row of the maximum of A over max(0, k - delta) .. min(R - 1, k + delta), scanned ascending and taken only
           where strictly greater: the lowest row wins a tie; rows that are not kept take part in the window
    STFT: kept where |V| > gamma;  Tx[r(m[k])] += Sx[k] dw ('sum') or dw / F ('lebesgue'), kept rows ascending
    CWT:  kept unless |W| < gamma;  w[k] = nu_hz[m[k]], +inf where not kept;  Tx = ssqueeze(Wx, w)"""
from __future__ import annotations

import numpy as np

from tests.helpers import msst_ref as ms
from tests.helpers import sst2_ref as m2


def energy(Z):
    """A of a complex map in the call's dtype: float64, the two products and the sum rounded one by one."""
    re, im = Z.real.astype(np.float64), Z.imag.astype(np.float64)
    return re * re + im * im


def rows_of(A, delta):
    """m by the definition, vectorised over the offsets.  A: real [..., R, n] -> int64, same shape."""
    A = np.asarray(A, dtype=np.float64)
    R = A.shape[-2]
    delta = int(delta)
    k = np.arange(R)
    lo = np.maximum(k - delta, 0)
    hi = np.minimum(k + delta, R - 1)
    best = A[..., lo, :]                                        # the first row of every window
    m = np.broadcast_to(lo[:, None], A.shape).astype(np.int64)
    for off in range(1, 2 * delta + 1):                          # row lo + off of the window, ascending
        r = lo + off
        ok = (r <= hi)[:, None]
        cand = A[..., np.minimum(r, R - 1), :]
        with np.errstate(invalid="ignore"):
            take = ok & (cand > best)
        best = np.where(take, cand, best)
        m = np.where(take, r[:, None], m)
    return m


def rows_brute(A, delta):
    """m by the definition, a triple loop.  A: real [R, n]."""
    A = np.asarray(A, dtype=np.float64)
    R, n = A.shape
    m = np.zeros((R, n), dtype=np.int64)
    for j in range(n):
        for k in range(R):
            lo, hi = max(0, k - delta), min(R - 1, k + delta)
            best, at = A[lo, j], lo
            for r in range(lo + 1, hi + 1):
                if A[r, j] > best:
                    best, at = A[r, j], r
            m[k, j] = at
    return m


def stft_bins(Sx, delta, gamma=None, flipud=False):
    """The bins of `lmssq_stft` on a reported Sx [F, n]: the row of Tx each coefficient goes to, -1 where |Sx| <= gamma."""
    rdt = np.float32 if Sx.dtype == np.complex64 else np.float64
    if gamma is None:
        gamma = 10 * float(np.finfo(rdt).eps)
    F = Sx.shape[0]
    m = rows_of(energy(Sx), delta)
    keep = np.abs(Sx.astype(np.complex128)) > gamma
    return np.where(keep, F - 1 - m if flipud else m, -1)


def cwt_rows(Wx, delta, gamma=None):
    """The rows of `lmssq_cwt` on a reported Wx [na, N]: m, -1 where |Wx| < gamma."""
    rdt = np.float32 if Wx.dtype == np.complex64 else np.float64
    if gamma is None:
        gamma = 10 * float(np.finfo(rdt).eps)
    m = rows_of(energy(Wx), delta)
    return np.where(np.abs(Wx.astype(np.complex128)) < gamma, -1, m)


def stft_V(x, window, n_fft, hop_len=1, padtype="reflect", modulated=True, arith="fft", dtype=np.complex128):
    """V [F, n_frames] in `dtype`: the STFT of sst2_ref, with the window alone."""
    cdt = np.dtype(dtype).type
    rdt = np.float32 if cdt == np.complex64 else np.float64
    x = np.asarray(x, dtype=np.float64)
    N, n = len(x), int(n_fft)
    nfr = (N - 1) // hop_len + 1
    xp = np.pad(x, [n // 2, n - 1 - n // 2], mode=m2.NP_PAD[padtype]).astype(rdt)
    frames = xp[np.arange(n)[:, None] + hop_len * np.arange(nfr)[None, :]]
    return m2._stft(frames, m2.size_window(window, n), modulated, arith, cdt)


def lmssq_stft_ref(x, window, n_fft, hop_len=1, fs=1.0, padtype="reflect", modulated=True, squeezing="sum", gamma=None,
                   flipud=False, delta=1, arith="fft", dtype=np.complex128):
    """-> (V, bins, Tx): V [F, n_frames] in `dtype`; bins int64, the row of Tx each coefficient went to (-1 where not
    kept); Tx in `dtype`."""
    V = stft_V(x, window, n_fft, hop_len, padtype, modulated, arith, dtype)
    F = V.shape[0]
    rdt = np.float32 if V.dtype == np.complex64 else np.float64
    bins = stft_bins(V, delta, gamma, flipud)
    dw = rdt(np.linspace(0, .5 * fs, F)[1])
    return V, bins, ms.scatter(V, bins, dw, squeezing)


def default_delta_stft(window, n_fft):
    """`upstream.lmsst_default_delta` restated: the main lobe's half-width at the 1e-3 level, or where it ends."""
    G = np.abs(np.fft.rfft(m2.size_window(window, n_fft), n_fft))
    F = len(G)
    for d in range(1, F - 1):
        if G[d] <= 1e-3 * G[0] or G[d + 1] >= G[d]:
            return min(d, 256)
    return min(F - 1, 256)
