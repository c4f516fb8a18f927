"""Numpy model of the time-reassigned synchrosqueezed CWT (`upstream.tssq_cwt`).  No GPU, no library.

Per-sample units throughout, `dt` enters at the end.  With P, n1, n2, xh, xi_k, T0, T1 and gamma exactly those of
`cwt_sst2_ref`, in float64 for either call dtype, on columns n1 .. n1 + N - 1:
    W = F^-1[xh T0]   W1 = F^-1[xh i xi T0]   W2 = F^-1[xh (-xi^2) T0]   Wt = F^-1[xh (-i) T1]   Wt1 = F^-1[xh xi T1]
    nu_i = wc / (2 pi a_i) cycles/sample      wc = (beta / gamma)^(1 / gamma) for the GMW, mu for the Morlet wavelet
    d1  = Re(Wt / W)
    D   = W^2 + Wt1 W - Wt W1                 num = W2 W - W1^2
    d2  = d1 - Im((D / num) (2 pi nu_i + i W1 / W))
    off = d2 where order = 2, |num| > gamma^2, d2 is finite and |d2| <= N, else d1; clamped to [-N, N] (a NaN stays)
    tau = off dt, rounded once to `rdt`; +inf where |W| < gamma
    m'  = clip(j + rint(tau / dt), 0, N - 1)  in `rdt`, on the reported tau (`reassign_cwt_ref.time_targets`)
    Tx[i, m'] += Wx[i, j] exp(-2 pi i frac(nu_i (j - m')))      Wx: W rounded to the call's complex dtype
`arith` = 'fft' or 'dft' as in `cwt_sst2_ref`, so that a test's tolerance can come from the model's disagreement with
itself.  The scatter sums in extended precision, and forms the rotation's angle there too."""
from __future__ import annotations

import numpy as np

from .cwt_sst2_ref import NP_PAD, _forward, _inverse, gmw_wc, p2up, tables
from .reassign_cwt_ref import time_targets

LD = np.longdouble


def row_freqs(wavelet, scales):
    """nu [na] float64, cycles/sample: the peak frequency of every row.  wavelet: ('gmw', gamma, beta) or ('morlet', mu)."""
    wc = gmw_wc(float(wavelet[1]), float(wavelet[2])) if wavelet[0] == "gmw" else float(wavelet[1])
    return wc / (2 * np.pi * np.asarray(scales, dtype=np.float64).reshape(-1))


def rotation(nu, j, m_to):
    """exp(-2 pi i frac(nu (j - m'))) as (re, im) in extended precision; nu [.., 1] or like j.  The product is taken on
    11-bit pieces of |j - m'| (a float64 times 11 bits is exact in a 64-bit significand, and so is the fraction of each
    piece), so the angle's error does not grow with |j - m'| < 2^33."""
    r = np.asarray(j, dtype=np.int64) - np.asarray(m_to, dtype=np.int64)
    sign, a = np.sign(r).astype(LD), np.abs(r)
    nu = np.asarray(nu, dtype=np.float64).astype(LD)
    f = np.zeros(np.broadcast(nu, a).shape, dtype=LD)
    for k in range(3):
        t = nu * ((a >> (11 * k)) & 2047).astype(LD) * LD(2.0 ** (11 * k))
        f = f + (t - np.rint(t))
    f = sign * (f - np.rint(f))
    ang = -8 * np.arctan(LD(1)) * f
    return np.cos(ang), np.sin(ang)


def scatter(Wx, mm, nu):
    """The extended-precision scatter of coefficients Wx [na, N] under the targets mm (-1: not kept; a NaN coefficient
    adds nothing) with the rotation at nu [na] -> (re, im: longdouble [na, N]; cnt: contributions of every cell; mass:
    sum of |Re Wx| + |Im Wx| over a cell's contributions, float64)."""
    na, N = Wx.shape
    keep = (mm >= 0) & ~(np.isnan(Wx.real) | np.isnan(Wx.imag))
    i, j = np.nonzero(keep)
    to = mm[i, j].astype(np.int64)
    c, s = rotation(np.asarray(nu, dtype=np.float64)[i], j, to)
    a, b = Wx.real[i, j].astype(LD), Wx.imag[i, j].astype(LD)
    re, im = np.zeros((na, N), dtype=LD), np.zeros((na, N), dtype=LD)
    np.add.at(re, (i, to), a * c - b * s)
    np.add.at(im, (i, to), a * s + b * c)
    cnt = np.zeros((na, N), dtype=np.int64)
    np.add.at(cnt, (i, to), 1)
    mass = np.zeros((na, N), dtype=np.float64)
    np.add.at(mass, (i, to), (np.abs(a) + np.abs(b)).astype(np.float64))
    return re, im, cnt, mass


def marginal(A, nu, keep=None):
    """sum_j A[i, j] exp(-2 pi i nu_i j) per row, in extended precision -> (re, im) longdouble [na]; keep: the bins that
    count (default: all that are not NaN)."""
    na, N = A.shape
    ok = ~(np.isnan(A.real) | np.isnan(A.imag)) if keep is None else keep
    c, s = rotation(np.asarray(nu, dtype=np.float64)[:, None], np.arange(N)[None, :], np.zeros((1, N), dtype=np.int64))
    a, b = np.where(ok, A.real, 0).astype(LD), np.where(ok, A.imag, 0).astype(LD)
    return (a * c - b * s).sum(axis=1), (a * s + b * c).sum(axis=1)


def tssq_cwt_ref(x, wavelet, scales, dt=1.0, padtype="reflect", order=2, gamma=None, arith="fft", tabs=None,
                 rdt=np.float64, squeeze=True, details=False):
    """-> (W, tau, mm, Tx): W [na, N] complex128 (unrounded); tau in `rdt` (+inf where a bin is not kept); mm int64 targets
    (-1 where not kept); Tx in the complex dtype of `rdt` (None with squeeze=False).  tabs: (T0, T1) [na, P] to use instead
    of `cwt_sst2_ref.tables`' own.  gamma default: 10 eps of `rdt`.  details=True appends a dict with d1, d2, offset
    (samples, clamped), num, use2, keep and nu."""
    if order not in (1, 2):
        raise ValueError(order)
    rdt = np.dtype(rdt).type
    cdt = np.complex64 if rdt == np.float32 else np.complex128
    x = np.asarray(x, dtype=np.float64)
    scales = np.asarray(scales, dtype=np.float64).reshape(-1)
    N, na = len(x), len(scales)
    P, n1, n2 = p2up(N)
    if gamma is None:
        gamma = 10 * float(np.finfo(rdt).eps)
    K = P // 2 + 1
    nu = row_freqs(wavelet, scales)
    xp = np.pad(x, [n1, n2], mode=NP_PAD[padtype])
    xh = _forward(xp, arith)
    T0, T1 = tables(wavelet, scales, P) if tabs is None else tabs
    T0, T1 = np.asarray(T0)[:, :K], np.asarray(T1)[:, :K]
    xi = 2 * np.pi * np.arange(K) / P
    with np.errstate(all="ignore"):
        if order == 1:
            maps = _inverse(np.concatenate([xh * T0, xh * (-1j) * T1], axis=0), P, n1, N, arith)
            W, Wt = maps[:na], maps[na:]
            d1 = (Wt / W).real
            d2, num, use2 = d1, np.zeros_like(W), np.zeros(W.shape, dtype=bool)
        else:
            spectra = [xh * T0, xh * (1j * xi) * T0, xh * (-xi * xi) * T0, xh * (-1j) * T1, xh * xi * T1]
            maps = _inverse(np.concatenate(spectra, axis=0), P, n1, N, arith)
            W, W1, W2, Wt, Wt1 = (maps[i * na:(i + 1) * na] for i in range(5))
            d1 = (Wt / W).real
            D = W * W + Wt1 * W - Wt * W1
            num = W2 * W - W1 * W1
            d2 = d1 - ((D / num) * (2 * np.pi * nu[:, None] + 1j * W1 / W)).imag
            use2 = (np.abs(num) > gamma * gamma) & np.isfinite(d2) & (np.abs(d2) <= N)
        off = np.where(use2, d2, d1)
        off = np.where(np.isnan(off), off, np.clip(off, -float(N), float(N)))
        keep = ~(np.abs(W) < gamma)
        tau = np.where(keep, off * dt, np.inf).astype(rdt)
        keep &= ~np.isinf(tau)                               # (an offset that overflows the dtype is not a target)
    mm = np.where(keep, time_targets(tau, dt), -1)
    Tx = None
    if squeeze:
        re, im, _, _ = scatter(W.astype(cdt), mm, nu)
        Tx = (re.astype(np.float64) + 1j * im.astype(np.float64)).astype(cdt)
    out = (W, tau, mm, Tx)
    if details:
        out += (dict(d1=d1, d2=d2, offset=off, num=num, use2=use2, keep=keep, nu=nu),)
    return out
