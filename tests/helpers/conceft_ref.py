"""NumPy fp64 model of ConceFT, the multitaper synchrosqueezed CWT `upstream.conceft_cwt` (Daubechies, Wang
and Wu 2016).  Upstream has no such transform; the definition is the project's.  Built from the restatements the suite
already holds: the order-k GMW and its transform (tests/helpers/gmw_order_ref.py: `gmw_l1_k`, `cwt_psih`) and upstream's
squeeze from dWx (tests/helpers/ssqueeze_ref.py: `ssqueeze_fast`).

    C_k     = int psih_k(w) / w dw = A sum_m kc[m] 2^m Gamma(beta / gamma + m) / gamma      (`adm`)
    gauge   r_m <- r_m conj(c_m) / |c_m|,  c_m = sum_j r_mj C_kj                            (`gauge`)
    draw    W^(m) = sum_j r_mj W_j, dW^(m) likewise, j ascending                            (`combine`)
    Tx      = (C_0 / sum_m c_m) sum_m ssqueeze_fast(W^(m), dW^(m), ...)                     (`squeeze_planes`)

Test infrastructure only."""
from __future__ import annotations

import math

import numpy as np

from oracle import upstream_oracle as u
from tests.helpers import gmw_order_ref as g
from tests.helpers import pad_ref
from tests.helpers import ssqueeze_ref as sq

MIN_ADMITTANCE = 1e-6


def adm(gamma, beta, k):
    """The closed form of C_k (bandpass norm)."""
    kc = g.gmw_k_constants(gamma, beta, k)
    q = beta / gamma
    wc = q ** (1 / gamma)
    A = math.exp(-beta * math.log(wc) + wc ** gamma)
    return float(A * sum(kc[m] * 2.0 ** m * math.gamma(q + m) for m in range(k + 1)) / gamma)


def adm_quadrature(gamma, beta, k, n=400001, w_max=12.0):
    """C_k by the trapezoid rule on gmw_l1_k(w) / w over (0, w_max]: the integrand vanishes at both ends with all its
    derivatives to working precision (w^(beta - 1) at 0, exp(-w^gamma) at w_max), so the rule converges spectrally."""
    w = np.linspace(0.0, w_max, n)[1:]
    f = g.gmw_l1_k(w, gamma, beta, k) / w
    return float(np.sum(f) * (w[1] - w[0]))


def gauge(r, adm_k):
    """-> (r [M, J] with unit rows and c_m real and positive, c [M]); ValueError for a zero or degenerate draw."""
    r = np.array(r, dtype=np.complex128)
    adm_k = np.asarray(adm_k, dtype=np.float64)
    norm = np.linalg.norm(r, axis=1)
    if (norm == 0).any():
        raise ValueError("zero vector")
    r = r / norm[:, None]
    c = r @ adm_k
    if (np.abs(c) <= MIN_ADMITTANCE * (np.abs(r) @ np.abs(adm_k))).any():
        raise ValueError("degenerate draw")
    r = r * (np.conj(c) / np.abs(c))[:, None]
    return r, np.abs(c)


def vectors(n_draws, n_orders, seed, adm_k):
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((n_draws, n_orders)) + 1j * rng.standard_normal((n_draws, n_orders))
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    return gauge(r, adm_k)[0]


def _cwt_psih_padded(x, psih_fn, scales, fs, padtype):
    """`gmw_order_ref.cwt_psih(..., derivative=True)` for the pad types the oracle's `padsignal` does not restate
    ('symmetric', 'replicate', 'wrap': tests/helpers/pad_ref.py), line for line."""
    x = np.asarray(x, dtype=np.float64)
    xp, n_up, n1, _ = pad_ref.padsignal(x, padtype)
    xh = np.fft.fft(xp)
    xi = u.xifn(1.0, n_up)
    Wx = np.zeros((len(scales), n_up), dtype=np.complex128)
    dWx = np.zeros_like(Wx)
    for i, a in enumerate(np.asarray(scales, dtype=np.float64)):
        psih = u.psih_at_scale(psih_fn, float(a), n_up)
        Wx[i] = np.fft.ifft(psih * xh)
        dWx[i] = np.fft.ifft((1j * xi * fs) * psih * xh)
    return Wx[:, n1:n1 + len(x)], dWx[:, n1:n1 + len(x)]


def planes(x, scales, gamma=3.0, beta=60.0, orders=(0, 1, 2), fs=1.0, padtype="reflect"):
    """(W, dW) [J, na, N]: the transform and its derivative for every order."""
    out = []
    for k in orders:
        fn = lambda w, k=k: g.gmw_l1_k(w, gamma, beta, k)                                 # noqa: E731
        out.append(g.cwt_psih(x, fn, scales, fs, True, padtype) if padtype in ("reflect", "zero")
                   else _cwt_psih_padded(x, fn, scales, fs, padtype))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def combine(P, r_m):
    """sum_j r_mj P_j, j ascending."""
    out = np.zeros(P.shape[1:], dtype=np.complex128)
    for j in range(P.shape[0]):
        out = out + r_m[j] * P[j]
    return out


def phase(Wm, dWm, gamma_t):
    """The draw's phase transform: +inf where |W| > gamma_t does not hold (algos.py:864)."""
    with np.errstate(all="ignore"):
        A, B, C, D = dWm.real, dWm.imag, Wm.real, Wm.imag
        w = np.abs((B * C - A * D) / ((C ** 2 + D ** 2) * 6.283185307179586))
    return np.where(np.abs(Wm) > gamma_t, w, np.inf)


def squeeze_planes(W, dW, r, c, adm0, f_asc, const, logscale, flipud, gamma_t, details=False):
    """Tx [na, N] from the planes W, dW [J, na, N] and GAUGED vectors r [M, J] with their c [M].  details: also the
    draws' W^(m) [M, na, N] and w [M, na, N]."""
    Tx = np.zeros(W.shape[1:], dtype=np.complex128)
    Wms, ws = [], []
    for m in range(r.shape[0]):
        Wm, dWm = combine(W, r[m]), combine(dW, r[m])
        Tx += sq.ssqueeze_fast(Wm, dWm, f_asc, const, logscale, flipud, gamma_t)
        if details:
            Wms.append(Wm)
            ws.append(phase(Wm, dWm, gamma_t))
    Tx *= adm0 / np.sum(c)
    return (Tx, np.stack(Wms), np.stack(ws)) if details else Tx


# ---- the noisy two-component signal of the concentration facts ----
def noisy_pair(N, noise_seed=None):
    """cos 2 pi (0.05 t + 0.05 t^2 / N) + cos(2 pi 0.30 t + 2 pi 8 sin(3 pi t / N)) (+ unit white noise) and the two
    instantaneous frequencies in cycles/sample."""
    t = np.arange(N, dtype=np.float64)
    x = np.cos(2 * np.pi * (0.05 * t + 0.05 * t * t / N)) + np.cos(2 * np.pi * 0.30 * t + 2 * np.pi * 8 * np.sin(3 * np.pi * t / N))
    if noise_seed is not None:
        x = x + np.random.default_rng(noise_seed).standard_normal(N)
    f1 = 0.05 + 0.1 * t / N
    f2 = 0.30 + 8 * (3 * np.pi / N) * np.cos(3 * np.pi * t / N)
    return x, f1, f2


def ridge_share(Tx, f1, f2, f_asc, flipud=True, half=2):
    """The share of |Tx|^2 within +-half rows of the two true instantaneous-frequency rows (log frequencies f_asc), over
    the columns N/8 .. 7N/8."""
    na, N = Tx.shape
    E = np.abs(Tx) ** 2
    cols = np.arange(N // 8, 7 * N // 8)
    mask = np.zeros((na, N), dtype=bool)
    params = sq.bin_params(f_asc, True)
    for f in (f1, f2):
        k = sq.bins(f, params, na - 1, flipud)
        for d in range(-half, half + 1):
            kk = k + d
            ok = (kk >= 0) & (kk < na)
            mask[kk[ok], np.arange(N)[ok]] = True
    return float(E[:, cols][mask[:, cols]].sum() / E[:, cols].sum())
