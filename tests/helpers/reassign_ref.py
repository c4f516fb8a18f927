"""Numpy model of the reassigned spectrogram (`upstream.reassign_stft`).  No GPU, no library.

Per-sample units throughout, `fs` enters at the end.  With n = n_fft, F = n//2 + 1, u[j] = j - n//2, the window tables g,
g1, tg of `sst2_ref` and V, V1, Vt the STFTs of x with them (frame m centred on sample m hop):
    w   = fs |k/n - Im(V1/V) / (2 pi)|          (`sst2_ref`'s first-order w1)         in the real dtype
    tau = clamp(Re(Vt/V), -n/2, n/2) / fs       (`tsst_ref`'s order-1 tau)            in the real dtype
    a bin is kept where |V| > gamma; w and tau are +inf where it is not
    k'  = `sst2_ref`'s bin rule on w, on np.linspace(0, fs/2, F), no flipud
    m'  = clip(m + rint(tau / (hop/fs)), 0, n_frames - 1)                              (`tsst_ref.targets`)
    Rx[k', m'] += |V[k, m]|^2
Two switches exist so that a test's tolerance can come from the model's disagreement with itself: `arith` = 'fft' or
'dft' and `dtype` = complex128 or complex64 (ALL arithmetic in that precision), as in `sst2_ref` and `tsst_ref`."""
from __future__ import annotations

import numpy as np

from .sst2_ref import NP_PAD, _stft, window_tables
from .tsst_ref import targets


def bins(w, fs, F):
    """`sst2_ref`'s bin rule on a reported map `w`, in w's own dtype -> k' int64; meaningless where w is inf."""
    rdt = w.dtype.type
    Sfs = np.linspace(0, .5 * fs, F)
    f0, dw = rdt(Sfs[0]), rdt(Sfs[1] - Sfs[0])
    with np.errstate(all="ignore"):
        v = np.maximum((w - f0) / dw, rdt(0))
        kk = np.minimum(np.rint(v), F - 1)
    return np.where(np.isnan(kk), 0, kk).astype(np.int64)


def energy(S, acc=np.float64):
    """|S|^2 from the real and imaginary parts, in `acc`."""
    return S.real.astype(acc) ** 2 + S.imag.astype(acc) ** 2


def scatter(E, kk, tgt, keep, acc=np.float64):
    """Rx of the energies E [F, n_frames] under the targets (kk, tgt), kept bins only, summed in `acc` (np.longdouble: a
    reference whose own summation error is out of the way) -> (Rx in acc, the number of contributions of every cell)."""
    k, m = np.nonzero(keep)
    Rx = np.zeros(E.shape, dtype=acc)
    np.add.at(Rx, (kk[k, m], tgt[k, m]), E[k, m].astype(acc))
    cnt = np.zeros(E.shape, dtype=np.int64)
    np.add.at(cnt, (kk[k, m], tgt[k, m]), 1)
    return Rx, cnt


def reassign_ref(x, window, n_fft, hop_len=1, fs=1.0, padtype="reflect", modulated=True, gamma=None, arith="fft",
                 dtype=np.complex128, details=False, tables=None, squeeze=True):
    """-> (V, w, tau, kk, tgt, Rx): V [F, n_frames] in `dtype`; w, tau real (+inf where a bin is not kept); kk, tgt int64
    target row and frame (-1 where not kept); Rx real, in the real dtype of `dtype` (None with squeeze=False).  tables:
    (g, g1, g2, tg, tg1) float64 to use instead of this module's own (a comparison with the library takes the library's:
    `sst2_ref.sst2_ref`); g2 and tg1 are not read.  details=True appends a dict with re_w1 (per sample, before |.| and
    fs), offset (samples, clamped) and keep."""
    cdt = np.dtype(dtype).type
    rdt = np.float32 if cdt == np.complex64 else np.float64
    x = np.asarray(x, dtype=np.float64)
    N, n, hop = len(x), int(n_fft), int(hop_len)
    F, nfr = n // 2 + 1, (N - 1) // hop + 1
    if gamma is None:
        gamma = 10 * float(np.finfo(rdt).eps)
    gamma = rdt(gamma)
    xp = np.pad(x, [n // 2, n - 1 - n // 2], mode=NP_PAD[padtype]).astype(rdt)
    frames = xp[np.arange(n)[:, None] + hop * np.arange(nfr)[None, :]]
    g, g1, _, tg, _ = window_tables(window, n) if tables is None else tables
    V, V1, Vt = (_stft(frames, t, modulated, arith, cdt) for t in (g, g1, tg))
    half = rdt(n / 2)
    eta = (np.arange(F, dtype=rdt) / rdt(n))[:, None]
    with np.errstate(all="ignore"):
        re_w1 = (eta - (V1 / V) / cdt(2j * np.pi)).real.astype(rdt)
        off = np.clip((Vt / V).real, -half, half).astype(rdt)
        keep = np.abs(V) > gamma
        w = np.where(keep, (float(fs) * np.abs(re_w1.astype(np.float64))).astype(rdt), rdt(np.inf)).astype(rdt)
        tau = np.where(keep, (off.astype(np.float64) / float(fs)).astype(rdt), rdt(np.inf)).astype(rdt)
    kk = bins(w, fs, F)
    tgt, _ = targets(tau, hop, fs)
    Rx = scatter(energy(V, rdt), kk, tgt, keep, rdt)[0] if squeeze else None
    out = (V, w, tau, np.where(keep, kk, -1), np.where(keep, tgt, -1), Rx)
    if details:
        out += (dict(re_w1=re_w1, offset=off, keep=keep),)
    return out
