"""Numpy model of the second-order synchrosqueezed CWT (`upstream.ssq_cwt2`).  No GPU, no library.

Per-sample units throughout, `dt` enters at the end.  With P, n1, n2 = p2up(N), xh the DFT of the padded signal,
xi_k = 2 pi k / P for k <= P/2 (analytic tables: zero above) and, for scale a, T0 = psih(a xi), T1 = a psih'(a xi) (both
halved at 2k == P):
    W = F^-1[xh T0]   W1 = F^-1[xh i xi T0]   W2 = F^-1[xh (-xi^2) T0]   Wt = F^-1[xh (-i) T1]   Wt1 = F^-1[xh xi T1]
    D = W^2 + Wt1 W - Wt W1      c = (W2 W - W1^2) / D      om1 = W1 / W      om2 = om1 - c Wt / W
    w2 = |Im om2| / (2 pi dt) where |D| > gamma^2 and Im om2 is finite, else |Im om1| / (2 pi dt); inf where |W| < gamma
each map kept on columns n1 .. n1 + N - 1.  Everything is float64.  `arith` = 'fft' (np.fft) or 'dft' (explicit DFT
matrices, built in row blocks of at most 100 MB) exists so that a test's tolerance can come from the model's
disagreement with itself.  The scatter follows `upstream.ssqueeze` from `w`: rows ascending, bins by the clamped
round-half-even rule on 'log' / 'linear' frequencies and the two-segment rule on 'log-piecewise' ones."""
from __future__ import annotations

import numpy as np

NP_PAD = {"reflect": "reflect", "zero": "constant", "symmetric": "symmetric", "replicate": "edge", "wrap": "wrap"}
BLOCK_BYTES = 100e6


def p2up(n):                                             # utils/common.py:32-51
    up = int(2 ** (1 + np.round(np.log2(n))))
    n2 = (up - n) // 2
    return up, up - n - n2, n2


def gmw_wc(gamma, beta):
    return (beta / gamma) ** (1 / gamma)


def psih(wavelet, w):
    """(psih(w), psih'(w)) of ('gmw', gamma, beta) or ('morlet', mu) on float64 w >= 0, by the textbook expressions."""
    w = np.asarray(w, dtype=np.float64)
    if wavelet[0] == "gmw":
        gamma, beta = float(wavelet[1]), float(wavelet[2])
        wc = gmw_wc(gamma, beta)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            p = 2 * np.exp(-beta * np.log(wc) + wc ** gamma + beta * np.log(w) - w ** gamma)
            d = p * (beta / w - gamma * w ** (gamma - 1))
        pos = w > 0
        return np.where(pos, p, 0.0), np.where(pos & (p > 0), d, 0.0)
    mu = float(wavelet[1])
    cs = (1 + np.exp(-mu ** 2) - 2 * np.exp(-0.75 * mu ** 2)) ** -0.5
    ks = np.exp(-0.5 * mu ** 2)
    C = np.sqrt(2) * cs * np.pi ** 0.25
    g, h = np.exp(-0.5 * (w - mu) ** 2), ks * np.exp(-0.5 * w ** 2)
    return C * (g - h), C * (-(w - mu) * g + w * h)


def tables(wavelet, scales, P):
    """(T0, T1), each [na, P] float64, zero above P/2 and halved at 2k == P."""
    scales = np.asarray(scales, dtype=np.float64).reshape(-1)
    K = P // 2 + 1
    xi = 2 * np.pi * np.arange(K) / P
    T0, T1 = np.zeros((len(scales), P)), np.zeros((len(scales), P))
    for i, a in enumerate(scales):
        p, d = psih(wavelet, a * xi)
        T0[i, :K], T1[i, :K] = p, a * d
    T0[:, P // 2] *= 0.5
    T1[:, P // 2] *= 0.5
    return T0, T1


def _unit(m, P):
    return np.exp(2j * np.pi * (m % P) / P)


def _forward(xp, arith):
    """DFT of the padded signal on k <= P/2."""
    P = len(xp)
    K = P // 2 + 1
    if arith == "fft":
        return np.fft.fft(xp)[:K]
    out = np.empty(K, dtype=np.complex128)
    step = max(1, int(BLOCK_BYTES // (16 * P)))
    n = np.arange(P)
    for k0 in range(0, K, step):
        k = np.arange(k0, min(K, k0 + step))
        out[k0:k0 + len(k)] = np.conj(_unit(k[:, None] * n[None, :], P)) @ xp
    return out


def _inverse(S, P, n1, N, arith):
    """F^-1 of spectra S [rows, P/2 + 1] (zero above P/2) on columns n1 .. n1 + N - 1."""
    K = S.shape[1]
    if arith == "fft":
        full = np.zeros((S.shape[0], P), dtype=np.complex128)
        full[:, :K] = S
        return np.fft.ifft(full, axis=1)[:, n1:n1 + N]
    out = np.empty((S.shape[0], N), dtype=np.complex128)
    step = max(1, int(BLOCK_BYTES // (16 * K)))
    k = np.arange(K)
    for c0 in range(0, N, step):
        n = n1 + np.arange(c0, min(N, c0 + step))
        out[:, c0:c0 + len(n)] = (S @ _unit(k[:, None] * n[None, :], P)) / P
    return out


def bin_positions(w, f_asc, kind, f_idx=None):
    """The bin rule of `upstream.ssqueeze` on finite frequencies w -> (bins int64 before any flip, v: the position that
    was rounded).  kind 'log' / 'linear' / 'log-piecewise' (f_idx: the transition of the frequencies)."""
    f = np.asarray(f_asc, dtype=np.float64)
    omax = len(f) - 1
    with np.errstate(all="ignore"):
        if kind == "linear":
            v = np.maximum((w - f[0]) / (f[1] - f[0]), 0)
        else:
            wl = np.log2(w)
            vmin, dv = np.log2(f[0]), np.log2(f[1]) - np.log2(f[0])
            v = np.maximum((wl - vmin) / dv, 0)
            if kind == "log-piecewise":
                vmin1 = np.log2(f[f_idx - 1])
                dv1 = max(np.log2(f[f_idx]) - np.log2(f[f_idx - 1]), 2.220446049250313e-16)
                v = np.where(wl > vmin1, (wl - vmin1) / dv1 + (f_idx - 1), v)
        b = np.rint(v)
    b = np.where(b >= omax, omax, b)
    return np.where(np.isnan(b), 0, b).astype(np.int64), v


def cwt_sst2_ref(x, wavelet, scales, f_asc, kind="log", f_idx=None, row_const=None, dt=1.0, padtype="reflect",
                 squeezing="sum", gamma=None, flipud=False, arith="fft", tabs=None, details=False):
    """-> (W, w2, bins, Tx): W [na, N] complex128; w2 float64 (inf where a bin is not kept); bins int64 (-1 where not
    kept; flipped with `flipud`); Tx complex128.  wavelet: ('gmw', gamma, beta) or ('morlet', mu).  tabs: (T0, T1)
    [na, P] to use instead of this module's own.  row_const [na]: the weight of every row (default 1).  details=True
    appends a dict with w1 (the first-order frequency), use2, D and v (the positions the bins were rounded from)."""
    x = np.asarray(x, dtype=np.float64)
    scales = np.asarray(scales, dtype=np.float64).reshape(-1)
    N, na = len(x), len(scales)
    P, n1, n2 = p2up(N)
    if gamma is None:
        gamma = 10 * float(np.finfo(np.float64).eps)
    K = P // 2 + 1
    xp = np.pad(x, [n1, n2], mode=NP_PAD[padtype])
    xh = _forward(xp, arith)
    T0, T1 = tables(wavelet, scales, P) if tabs is None else tabs
    T0, T1 = np.asarray(T0)[:, :K], np.asarray(T1)[:, :K]
    xi = 2 * np.pi * np.arange(K) / P
    spectra = [xh * T0, xh * (1j * xi) * T0, xh * (-xi * xi) * T0, xh * (-1j) * T1, xh * xi * T1]
    maps = _inverse(np.concatenate(spectra, axis=0), P, n1, N, arith)
    W, W1, W2, Wt, Wt1 = (maps[i * na:(i + 1) * na] for i in range(5))
    with np.errstate(all="ignore"):
        D = W * W + Wt1 * W - Wt * W1
        c = (W2 * W - W1 * W1) / D
        om1 = W1 / W
        om2 = om1 - c * Wt / W
        use2 = (np.abs(D) > gamma * gamma) & np.isfinite(om2.imag)
        w = np.abs(np.where(use2, om2.imag, om1.imag)) / (2 * np.pi * dt)
        keep = ~(np.abs(W) < gamma)
        w2 = np.where(keep, w, np.inf)
        bins, v = bin_positions(w2, f_asc, kind, f_idx)
    if flipud:
        bins = na - 1 - bins
    keep = np.isfinite(w2) | np.isnan(w2)                 # (the scatter skips infinite frequencies alone)
    rc = np.ones(na) if row_const is None else np.asarray(row_const, dtype=np.float64)
    add = (np.full((na, N), 1.0 / na) if squeezing == "lebesgue" else W) * rc[:, None]
    Tx = np.zeros((na, N), dtype=np.complex128)
    cols = np.arange(N)
    for i in range(na):                                    # rows ascending: one target per column and row
        m = keep[i]
        Tx[bins[i, m], cols[m]] += add[i, m]
    out = (W, w2, np.where(keep, bins, -1), Tx)
    if details:
        out += (dict(w1=np.abs(om1.imag) / (2 * np.pi * dt), use2=use2, D=D, v=v),)
    return out


def chirp(N, f0, f1, sigma=None):
    """cos of a linear sweep f0 -> f1 cycles/sample over N samples (under a Gaussian envelope of `sigma` samples about
    the middle, if given), and its instantaneous frequency."""
    t = np.arange(N, dtype=np.float64)
    c = (f1 - f0) / N
    x = np.cos(2 * np.pi * (f0 * t + 0.5 * c * t * t))
    if sigma is not None:
        x = x * np.exp(-0.5 * ((t - N / 2) / sigma) ** 2)
    return x, f0 + c * t


def log_freqs(N, na, dt=1.0):
    """The 'maximal' log frequency grid of `ssq_cwt` (ssqueezing.py:218-290), ascending."""
    fm, fM = 1 / (dt * N), 1 / (2 * dt)
    return fm * np.power(fM / fm, np.arange(na) / (na - 1))
