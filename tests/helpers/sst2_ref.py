"""Numpy model of the second-order synchrosqueezed STFT (`upstream.ssq_stft2`).  No GPU, no library.

Per-sample units throughout, `fs` enters at the end.  With n = n_fft, F = n//2 + 1, u[m] = m - n//2:
    g   the sized window                      g1 = spectral derivative of g (Nyquist term zeroed)      g2 = the same of g1
    tg  = u g                                 tg1 = u g1
    V, V1, V2, Vt, Vt1 = STFTs of x with those windows (padding, hop and `modulated` rotation of upstream's stft)
    w1 = k/n - (V1/V) / (2 pi i)              D = Vt V1 - Vt1 V              q = (V2 V - V1^2) / (2 pi i D)
    w2 = w1 - q Vt/V     where |D| > gamma^2 and Re w2 is finite, else w1;   reported as fs |Re .|, inf where |V| <= gamma
Two switches exist so that a test's tolerance can come from the model's disagreement with itself: `arith` = 'fft'
(np.fft.rfft) or 'dft' (an explicit DFT-matrix product), and `dtype` = complex128 or complex64 (ALL arithmetic in that
precision).  The scatter accumulates every column's rows in ascending order, as the GPU's scatter kernel does."""
from __future__ import annotations

import numpy as np

NP_PAD = {"reflect": "reflect", "zero": "constant", "symmetric": "symmetric", "replicate": "edge", "wrap": "wrap"}


def diff_window(g):
    """Re ifft(fft(g) i xi), xi_k = 2 pi k~/n (k~ signed), the Nyquist term of an even length zeroed; float64."""
    g = np.asarray(g, dtype=np.float64)
    n = len(g)
    k = np.arange(n, dtype=np.float64)
    k[n // 2 + 1:] -= n
    xi = 2 * np.pi * k / n
    if n % 2 == 0:
        xi[n // 2] = 0
    return np.fft.ifft(np.fft.fft(g) * 1j * xi).real


def size_window(window, n_fft):
    """Centre zero-pad of an ndarray window to n_fft (upstream's get_window)."""
    w = np.asarray(window, dtype=np.float64)
    pl = (n_fft - len(w)) // 2
    return np.pad(w, [pl, n_fft - len(w) - pl])


def window_tables(window, n_fft):
    """(g, g1, g2, tg, tg1) in float64."""
    g = size_window(window, n_fft)
    g1 = diff_window(g)
    g2 = diff_window(g1)
    u = np.arange(n_fft, dtype=np.float64) - n_fft // 2
    return g, g1, g2, u * g, u * g1


def _stft(frames, tab, modulated, arith, cdt):
    """rfft over axis 0 of frames * tab ([n, n_frames]), rotated by n//2 when modulated, in the precision of `cdt`."""
    rdt = np.float32 if cdt == np.complex64 else np.float64
    n = frames.shape[0]
    z = frames * tab.astype(rdt)[:, None]
    if modulated:
        z = np.roll(z, -(n // 2), axis=0)
    if arith == "fft":
        out = np.fft.rfft(z, axis=0)
    elif arith == "dft":
        k = np.arange(n // 2 + 1)[:, None] * np.arange(n)[None, :]
        W = np.exp(-2j * np.pi * (k % n) / n).astype(cdt)
        out = W @ z.astype(cdt)
    else:
        raise ValueError(arith)
    assert out.dtype == cdt, out.dtype
    return out


def sst2_ref(x, window, n_fft, hop_len=1, fs=1.0, padtype="reflect", modulated=True, squeezing="sum", gamma=None,
             flipud=False, arith="fft", dtype=np.complex128, details=False, tables=None):
    """-> (V, w2, kk, Tx): V [F, n_frames] in `dtype`; w2 real (inf where a bin is not kept); kk int64 (-1 where not
    kept); Tx in `dtype`.  tables: (g, g1, g2, tg, tg1) float64 to use instead of this module's own (g2, a second
    derivative by FFT, carries 1e-11 of rounding noise that differs between FFT implementations and moves w2 on
    ill-conditioned bins: a comparison with the library takes the library's tables).  details=True appends a dict with
    re_w1, re_w2 (per sample, before |.| and fs), D and keep."""
    cdt = np.dtype(dtype).type
    rdt = np.float32 if cdt == np.complex64 else np.float64
    x = np.asarray(x, dtype=np.float64)
    N, n = len(x), int(n_fft)
    F, nfr = n // 2 + 1, (N - 1) // hop_len + 1
    if gamma is None:
        gamma = 10 * float(np.finfo(rdt).eps)
    gamma = rdt(gamma)
    xp = np.pad(x, [n // 2, n - 1 - n // 2], mode=NP_PAD[padtype]).astype(rdt)
    frames = xp[np.arange(n)[:, None] + hop_len * np.arange(nfr)[None, :]]
    g, g1, g2, tg, tg1 = window_tables(window, n) if tables is None else tables
    V, V1, V2, Vt, Vt1 = (_stft(frames, t, modulated, arith, cdt) for t in (g, g1, g2, tg, tg1))
    two_pi_i = cdt(2j * np.pi)
    eta = (np.arange(F, dtype=rdt) / rdt(n))[:, None]
    with np.errstate(all="ignore"):
        w1 = eta - (V1 / V) / two_pi_i
        D = Vt * V1 - Vt1 * V
        q = (V2 * V - V1 * V1) / (two_pi_i * D)
        w2c = w1 - q * (Vt / V)
        use2 = (np.abs(D) > gamma * gamma) & np.isfinite(w2c.real)
        re_w = np.where(use2, w2c.real, w1.real).astype(rdt)
        w2 = rdt(fs) * np.abs(re_w)
        keep = np.abs(V) > gamma
        Sfs = np.linspace(0, .5 * fs, F)
        f0, dw = rdt(Sfs[0]), rdt(Sfs[1] - Sfs[0])
        v = np.maximum((w2 - f0) / dw, rdt(0))
        kk = np.minimum(np.rint(v), F - 1)
        kk = np.where(np.isnan(kk), 0, kk).astype(np.int64)
    if flipud:
        kk = F - 1 - kk
    Tx = np.zeros((F, nfr), dtype=cdt)
    cols = np.arange(nfr)
    add = np.full((F, nfr), dw / rdt(F), dtype=cdt) if squeezing == "lebesgue" else (V * dw).astype(cdt)
    for i in range(F):                                     # rows ascending: one target per column and row
        m = keep[i]
        Tx[kk[i, m], cols[m]] += add[i, m]
    out = (V, np.where(keep, w2, rdt(np.inf)).astype(rdt), np.where(keep, kk, -1), Tx)
    if details:
        out += (dict(re_w1=w1.real, re_w2=w2c.real, D=D, keep=keep, use2=use2, dw=dw, Sfs=Sfs),)
    return out


def gauss_window(n_fft, sigma):
    u = np.arange(n_fft, dtype=np.float64) - n_fft // 2
    return np.exp(-0.5 * (u / sigma) ** 2)


def chirp(N, f0, f1):
    """cos of a linear sweep f0 -> f1 cycles/sample over N samples, and its instantaneous frequency."""
    t = np.arange(N, dtype=np.float64)
    c = (f1 - f0) / N
    return np.cos(2 * np.pi * (f0 * t + 0.5 * c * t * t)), f0 + c * t
