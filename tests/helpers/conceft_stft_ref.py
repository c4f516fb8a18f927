"""NumPy fp64 model of ConceFT on the STFT, `upstream.conceft_stft` (Daubechies, Wang and Wu 2016).  Upstream
has no such transform; the definition is the project's.  Built from the restatements the suite already holds: the frames,
`diff_window` and `size_window` of tests/helpers/sst2_ref.py and the `gauge` and `combine` of tests/helpers/conceft_ref.py.

    tapers  h_j sized to n = n_fft, c = n // 2, g1_j = diff_window(h_j)                      (`sized`)
    planes  V_j, V1_j = the STFTs of x with h_j, g1_j                                        (`planes`)
    gauge   r_m <- r_m conj(c_m) / |c_m|,  c_m = sum_j r_mj h_j[c]                           (`conceft_ref.gauge`)
    draw    S = sum_j r_mj V_j, dS likewise; w = fs |k/n - Im(dS / S) / (2 pi)|, kept where |S| > gamma
    bin     the clamped round-half-even bin of w on linspace(0, fs / 2, F), NaN -> 0, flipped under flipud   (`bins`)
    Tx      Tx[bin, t] += S dw h_0[c] / sum_m c_m                                            (`squeeze_planes`)

Test infrastructure only."""
from __future__ import annotations

import math

import numpy as np

from tests.helpers import conceft_ref as cr
from tests.helpers import sst2_ref as s2


def hermite(n_fft, n_tapers, sigma=None):
    """The orthonormal Hermite functions from numpy's physicists' polynomials (not the recurrence the package runs):
    H_k(u) exp(-u^2 / 2) / sqrt(2^k k! sqrt(pi) sigma) at u = (i - n_fft // 2) / sigma."""
    sigma = n_fft / 16 if sigma is None else float(sigma)
    u = (np.arange(n_fft, dtype=np.float64) - n_fft // 2) / sigma
    out = []
    for k in range(n_tapers):
        ck = np.zeros(k + 1)
        ck[k] = 1
        out.append(np.polynomial.hermite.hermval(u, ck) * np.exp(-0.5 * u * u)
                   / math.sqrt(2.0 ** k * math.factorial(k) * math.sqrt(math.pi) * sigma))
    return np.stack(out)


def sized(tapers, n_fft):
    """The tapers [J, win_len] centre zero-padded to n_fft."""
    return np.stack([s2.size_window(h, n_fft) for h in np.asarray(tapers, dtype=np.float64)])


def frames(x, n_fft, hop_len=1, padtype="reflect"):
    """[n_fft, n_frames]: the padded signal cut into frames (upstream's stft: n_fft // 2 samples on the left)."""
    x = np.asarray(x, dtype=np.float64)
    n = int(n_fft)
    nfr = (len(x) - 1) // hop_len + 1
    xp = np.pad(x, [n // 2, n - 1 - n // 2], mode=s2.NP_PAD[padtype])
    return xp[np.arange(n)[:, None] + hop_len * np.arange(nfr)[None, :]]


def planes(x, tapers, n_fft, hop_len=1, padtype="reflect", modulated=True, arith="fft"):
    """(V, V1) [J, F, n_frames] complex128: the STFTs with every sized taper and with its spectral derivative."""
    fr = frames(x, n_fft, hop_len, padtype)
    h = sized(tapers, n_fft)
    V = np.stack([s2._stft(fr, hj, modulated, arith, np.complex128) for hj in h])
    V1 = np.stack([s2._stft(fr, s2.diff_window(hj), modulated, arith, np.complex128) for hj in h])
    return V, V1


def phase(S, dS, n_fft, fs, gamma_t):
    """The draw's frequency fs |k/n - Im(dS/S)/(2 pi)| in the expression the kernel uses; +inf where |S| > gamma_t does
    not hold."""
    F = S.shape[0]
    eta = (np.arange(F, dtype=np.float64) * (1.0 / n_fft))[:, None]
    with np.errstate(all="ignore"):
        den = S.real ** 2 + S.imag ** 2
        w = fs * np.abs(eta - (dS.imag * S.real - dS.real * S.imag) / (den * 6.283185307179586))
    return np.where(np.abs(S) > gamma_t, w, np.inf)


def bin_positions(w, F, fs):
    """(k: the clamped round-half-even bin before any flip, v: the position that was rounded) of frequencies w on
    linspace(0, fs / 2, F)."""
    Sfs = np.linspace(0, .5 * fs, F)
    dw = Sfs[1] - Sfs[0]
    with np.errstate(all="ignore"):
        v = np.maximum(np.asarray(w, dtype=np.float64) / dw, 0.0)
        k = np.minimum(np.rint(v), F - 1)
        k = np.where(np.isnan(k), 0, k).astype(np.int64)
    return k, v


def squeeze_planes(V, V1, r, c, h0c, n_fft, fs=1.0, flipud=False, gamma_t=None, details=False):
    """Tx [F, n_frames] from the planes V, V1 [J, F, n_frames] and GAUGED vectors r [M, J] with their c [M].  details:
    also the draws' S [M, F, n_frames] and w [M, F, n_frames]."""
    F, nfr = V.shape[1:]
    if gamma_t is None:
        gamma_t = 10 * float(np.finfo(np.float64).eps)
    Sfs = np.linspace(0, .5 * fs, F)
    fac = (Sfs[1] - Sfs[0]) * h0c / np.sum(c)
    Tx = np.zeros((F, nfr), dtype=np.complex128)
    cols = np.arange(nfr)
    Ss, ws = [], []
    for m in range(r.shape[0]):
        S, dS = cr.combine(V, r[m]), cr.combine(V1, r[m])
        w = phase(S, dS, n_fft, fs, gamma_t)
        k, _ = bin_positions(w, F, fs)
        if flipud:
            k = F - 1 - k
        keep = ~np.isinf(w)
        np.add.at(Tx, (k[keep], np.broadcast_to(cols, k.shape)[keep]), S[keep] * fac)        # (rows ascending per column)
        if details:
            Ss.append(S)
            ws.append(w)
    return (Tx, np.stack(Ss), np.stack(ws)) if details else Tx


def conceft_stft_ref(x, tapers, n_fft, r, hop_len=1, fs=1.0, padtype="reflect", modulated=True, flipud=False,
                     gamma_t=None, details=False):
    """The whole transform from raw vectors r [M, J] (gauged here)."""
    h = sized(tapers, n_fft)
    adm = h[:, n_fft // 2]
    rg, c = cr.gauge(r, adm)
    V, V1 = planes(x, tapers, n_fft, hop_len, padtype, modulated)
    return squeeze_planes(V, V1, rg, c, adm[0], n_fft, fs, flipud, gamma_t, details)


def draws(n_draws, n_tapers, seed):
    """`default_rng(seed)` complex normals with unit rows (the package's raw draws)."""
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((n_draws, n_tapers)) + 1j * rng.standard_normal((n_draws, n_tapers))
    return r / np.linalg.norm(r, axis=1, keepdims=True)


def ridge_share(Tx, f1, f2, fs=1.0, flipud=False, half=2):
    """The share of |Tx|^2 within +-half rows of the two true instantaneous-frequency rows (f1, f2 in the units of fs,
    one value per column) over the columns N/8 .. 7N/8."""
    F, N = Tx.shape
    E = np.abs(Tx) ** 2
    cols = np.arange(N // 8, 7 * N // 8)
    mask = np.zeros((F, N), dtype=bool)
    for f in (f1, f2):
        k, _ = bin_positions(f, F, fs)
        if flipud:
            k = F - 1 - k
        for d in range(-half, half + 1):
            kk = k + d
            ok = (kk >= 0) & (kk < F)
            mask[kk[ok], np.arange(N)[ok]] = True
    return float(E[:, cols][mask[:, cols]].sum() / E[:, cols].sum())
