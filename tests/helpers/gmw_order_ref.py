"""NumPy fp64 restatement of upstream's higher-order GMW transforms (old/ssqueezepy): the order-k wavelet
(`_gmw.py:267-295` gmw_l1_k, `:366-395` _gmw_k_constants), `cwt_higher_order` (`_cwt.py:515-608`: one full transform per
order, THEN the mean of the outputs) and the `order > 0` branch of `ssq_cwt` (`_ssq_cwt.py:227-241`: Wx from the padded
transform, dWx by `trigdiff`, `utils/common.py:161-240`; ssq_freqs from the order-0 wavelet).

Test infrastructure only.  The padding, frequency grid, Nyquist halving, ssq frequencies and bin rules are those of
oracle/upstream_oracle.py, imported.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import upstream_oracle as u


def gmw_k_constants(gamma, beta, k):
    """_gmw.py:366-395, norm='bandpass'."""
    r = (2 * beta + 1) / gamma
    c = r - 1
    coeff = np.sqrt(np.exp(math.lgamma(r) + math.lgamma(k + 1) - math.lgamma(k + r)))
    L = np.zeros(k + 1)
    for m in range(k + 1):
        fact = np.exp(math.lgamma(k + c + 1) - math.lgamma(c + m + 1) - math.lgamma(k - m + 1))
        L[m] = (-1) ** m * fact / math.gamma(m + 1)
    return L * coeff * 2


def gmw_l1_k(w, gamma=3.0, beta=60.0, k=0):
    """_gmw.py:284-295 (_gmw_l1_k): C(w) exp(-beta ln wc + wc^gamma + beta ln w - w^gamma), 0 for w < 0."""
    w = np.array(w, dtype=np.float64, copy=True)
    wc = u.morsefreq(gamma, beta)
    kc = gmw_k_constants(gamma, beta, k)
    nonneg = w >= 0
    w = w * nonneg
    C = np.zeros_like(w)
    for m in range(len(kc)):
        C += kc[m] * (2 * w ** gamma) ** m
    with np.errstate(divide="ignore", invalid="ignore"):
        return C * np.exp(-beta * np.log(wc) + wc ** gamma + beta * np.log(w) - w ** gamma) * nonneg


def cwt_psih(x, psih_fn, scales, fs=1.0, derivative=False, padtype="reflect", rpadded=False):
    """_cwt.py:160-318 for any psih(w) (L1 norm): Wx [na, N] (or [na, n_up] with rpadded), and dWx."""
    x = np.asarray(x, dtype=np.float64)
    N = len(x)
    dt = 1.0 / fs
    xp, n_up, n1, _ = u.padsignal(x, padtype)
    xh = np.fft.fft(xp)
    xi = u.xifn(1.0, n_up)
    Wx = np.zeros((len(scales), n_up), dtype=np.complex128)
    dWx = np.zeros_like(Wx) if derivative else None
    for i, a in enumerate(np.asarray(scales, dtype=np.float64)):
        psih = u.psih_at_scale(psih_fn, float(a), n_up)
        Wx[i] = np.fft.ifft(psih * xh)
        if derivative:
            dWx[i] = np.fft.ifft((1j * xi / dt) * psih * xh)
    if not rpadded:
        Wx = Wx[:, n1:n1 + N]
        dWx = dWx[:, n1:n1 + N] if derivative else None
    return Wx, dWx


def cwt_higher_order(x, scales, gamma=3.0, beta=60.0, order=1, average=None, fs=1.0, derivative=False,
                     padtype="reflect", rpadded=False):
    """_cwt.py:515-608: one transform per order with its own wavelet, then the mean over the orders of the OUTPUTS
    (np.vstack([list]) stacks, the mean runs over the order axis), or a list; x may be [B, N]."""
    if isinstance(order, (list, range)):
        order = tuple(order)
    is_tuple = isinstance(order, tuple)
    orders = list(order) if is_tuple else [order]
    if len(orders) == 1 and average:
        average = False
    x = np.asarray(x, dtype=np.float64)

    def one(k):
        fn = lambda w: gmw_l1_k(w, gamma, beta, k)                                        # noqa: E731
        outs = [cwt_psih(xb, fn, scales, fs, derivative, padtype, rpadded) for xb in (x if x.ndim == 2 else [x])]
        W = np.stack([o[0] for o in outs]) if x.ndim == 2 else outs[0][0]
        dW = (np.stack([o[1] for o in outs]) if x.ndim == 2 else outs[0][1]) if derivative else None
        return W, dW

    res = [one(k) for k in orders]
    Wx, dWx = [r[0] for r in res], [r[1] for r in res]
    if average or (average is None and is_tuple):
        Wx = np.mean(np.vstack([Wx]), axis=0)
        dWx = np.mean(np.vstack([dWx]), axis=0) if derivative else None
    elif len(Wx) == 1:
        Wx, dWx = Wx[0], dWx[0]
    return (Wx, dWx) if derivative else Wx


def trigdiff(A, fs, N, n1):
    """utils/common.py:161-240 with rpadded=True: ifft(fft(A) * 1j * xi * fs), then unpadded."""
    xi = u.xifn(1, A.shape[-1])
    return np.fft.ifft(np.fft.fft(A, axis=-1) * 1j * xi * fs, axis=-1)[..., n1:n1 + N]


def ssq_cwt_order(x, scales, gamma=3.0, beta=60.0, order=1, fs=1.0, padtype="reflect", squeezing="sum",
                  maprange="peak", ssq_freqs=None, flipud=True):
    """_ssq_cwt.py:227-311 with `order > 0`: Wx of the (averaged) orders on the padded grid, dWx = trigdiff(Wx), then the
    restated synchrosqueezing of oracle/upstream_oracle.py:ssq_cwt with the ORDER-0 wavelet's ssq_freqs.
    -> Tx, Wx, out_freqs, scales, intermediates."""
    x = np.asarray(x, dtype=np.float64)
    N = len(x)
    dt = 1.0 / fs
    scales = np.asarray(scales, dtype=np.float64).reshape(-1)
    nv = u.infer_nv(scales)
    _, n1, _ = u.p2up(N)
    average = isinstance(order, (tuple, list, range))
    Wp = cwt_higher_order(x, scales, gamma, beta, order, average, fs=fs, padtype=padtype, rpadded=True)
    dWx = trigdiff(Wp, fs, N, n1)
    Wx = Wp[:, n1:n1 + N]
    gamma_t = 10 * u.EPS64
    scaletype = ssq_freqs if isinstance(ssq_freqs, str) else "log"
    freqs = u.cwt_ssq_freqs(scales, N, ("gmw", {"gamma": gamma, "beta": beta}), dt, maprange, scaletype)
    const = np.log(2) / nv
    na = len(scales)
    with np.errstate(all="ignore"):
        A, B, C, D = dWx.real, dWx.imag, Wx.real, Wx.imag
        w = np.abs((B * C - A * D) / ((C ** 2 + D ** 2) * 6.283185307179586))
    keep = np.abs(Wx) > gamma_t
    if scaletype == "log":
        k = u._bins_log(w, float(np.log2(freqs[0])), float(np.log2(freqs[1]) - np.log2(freqs[0])), na - 1)
    else:
        k = u._bins_lin(w, float(freqs[0]), float(freqs[1] - freqs[0]), na - 1)
    if flipud:
        k = na - 1 - k
    Wv = (np.ones(Wx.shape, dtype=Wx.dtype) / na) if squeezing == "lebesgue" else Wx
    Tx = np.zeros(Wx.shape, dtype=np.complex128)
    cols = np.arange(N)
    for i in range(na):
        m = keep[i]
        np.add.at(Tx, (k[i, m], cols[m]), Wv[i, m] * const)
    return Tx, Wx, freqs[::-1], scales, dict(dWx=dWx, w=np.where(keep, w, np.inf), k=np.where(keep, k, -1),
                                             const=const, freqs_ascending=freqs)
