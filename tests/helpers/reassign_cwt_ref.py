"""Numpy model of the reassigned scalogram (`upstream.reassign_cwt`).  No GPU, no library.

Per-sample units throughout, `dt` enters at the end.  With P, n1, n2, xh, xi_k, T0, T1 and gamma exactly those of
`cwt_sst2_ref`, in float64 for either call dtype:
    W = F^-1[xh T0]     W1 = F^-1[xh i xi T0]     Wt = F^-1[xh (-i) T1]             columns n1 .. n1 + N - 1
    w   = |Im(W1/W)| / (2 pi dt)                 (`cwt_sst2_ref`'s first-order branch)   rounded once to `rdt`
    tau = clamp(Re(Wt/W), -N, N) dt              (seconds)                               rounded once to `rdt`
    kept: not (|W| < gamma); w and tau are +inf where a bin is not kept
    k'  = `upstream.ssqueeze`'s bin rule on the reported w, in its dtype, then flipped with `flipud`
    m'  = clip(j + rint(tau / dt), 0, N - 1) in the call's dtype (`tsst_ref.targets`' arithmetic)
    Rx[k', m'] += |Wx[i, j]|^2                   of the REPORTED Wx (W rounded to the call's complex dtype), in float64
`arith` = 'fft' or 'dft' as in `cwt_sst2_ref`, so that a test's tolerance can come from the model's disagreement with
itself."""
from __future__ import annotations

import numpy as np

from .cwt_sst2_ref import NP_PAD, _forward, _inverse, bin_positions, p2up, tables
from .reassign_ref import energy, scatter  # noqa: F401  (re-exported: the tests scatter a call's own maps with them)


def time_targets(tau, dt):
    """The time rule on a reported map `tau`, in tau's own dtype -> m' int64; meaningless where tau is inf."""
    rdt = tau.dtype.type
    N = tau.shape[-1]
    with np.errstate(all="ignore"):
        v = tau / rdt(dt)
        r = np.where(np.isfinite(v), np.rint(v), 0).astype(np.int64)
    return np.clip(np.arange(N, dtype=np.int64) + r, 0, N - 1)


def freq_targets(w, f_asc, kind, f_idx, flipud):
    """The bin rule on a reported map `w`, in w's own dtype -> k' int64; meaningless where w is inf."""
    rdt = w.dtype.type
    f = np.asarray(f_asc, dtype=np.float64)
    omax = len(f) - 1
    with np.errstate(all="ignore"):
        if kind == "linear":
            v = np.maximum((w - rdt(f[0])) / rdt(f[1] - f[0]), rdt(0))
            b = np.rint(v)
        else:
            wl = np.log2(w)
            vmin, dv = rdt(np.log2(f[0])), np.log2(f[1]) - np.log2(f[0])
            if kind == "log-piecewise":
                dv = max(dv, 2.220446049250313e-16)
                vmin1 = rdt(np.log2(f[f_idx - 1]))
                dv1 = rdt(max(np.log2(f[f_idx]) - np.log2(f[f_idx - 1]), 2.220446049250313e-16))
                b = np.where(wl > vmin1, np.rint((wl - vmin1) / dv1) + rdt(f_idx - 1),
                             np.rint(np.maximum((wl - vmin) / rdt(dv), rdt(0))))
            else:
                b = np.rint(np.maximum((wl - vmin) / rdt(dv), rdt(0)))
    b = np.where(b >= omax, omax, b)
    k = np.where(np.isnan(b), 0, b).astype(np.int64)
    return omax - k if flipud else k


def reassign_cwt_ref(x, wavelet, scales, f_asc, kind="log", f_idx=None, dt=1.0, padtype="reflect", gamma=None,
                     flipud=False, arith="fft", tabs=None, rdt=np.float64, squeeze=True, details=False):
    """-> (W, w, tau, kk, mm, Rx): W [na, N] complex128 (unrounded); w, tau in `rdt` (+inf where a bin is not kept); kk, mm
    int64 targets (-1 where not kept); Rx in `rdt` (None with squeeze=False).  wavelet: ('gmw', gamma, beta) or
    ('morlet', mu).  tabs: (T0, T1) [na, P] to use instead of `cwt_sst2_ref.tables`' own.  gamma default: 10 eps of
    `rdt`.  details=True appends a dict with im1 (Im(W1/W) per sample), offset (samples, clamped) and keep."""
    rdt = np.dtype(rdt).type
    cdt = np.complex64 if rdt == np.float32 else np.complex128
    x = np.asarray(x, dtype=np.float64)
    scales = np.asarray(scales, dtype=np.float64).reshape(-1)
    N, na = len(x), len(scales)
    P, n1, n2 = p2up(N)
    if gamma is None:
        gamma = 10 * float(np.finfo(rdt).eps)
    K = P // 2 + 1
    xp = np.pad(x, [n1, n2], mode=NP_PAD[padtype])
    xh = _forward(xp, arith)
    T0, T1 = tables(wavelet, scales, P) if tabs is None else tabs
    T0, T1 = np.asarray(T0)[:, :K], np.asarray(T1)[:, :K]
    xi = 2 * np.pi * np.arange(K) / P
    maps = _inverse(np.concatenate([xh * T0, xh * (1j * xi) * T0, xh * (-1j) * T1], axis=0), P, n1, N, arith)
    W, W1, Wt = (maps[i * na:(i + 1) * na] for i in range(3))
    with np.errstate(all="ignore"):
        im1 = (W1 / W).imag
        off = np.clip((Wt / W).real, -float(N), float(N))
        keep = ~(np.abs(W) < gamma)
        w = np.where(keep, np.abs(im1) / (2 * np.pi * dt), np.inf).astype(rdt)
        tau = np.where(keep, off * dt, np.inf).astype(rdt)
        keep &= ~np.isinf(w)                                 # (a frequency that overflows the dtype is not a target)
        tau = np.where(keep, tau, rdt(np.inf))
    kk = freq_targets(w, f_asc, kind, f_idx, flipud)
    mm = time_targets(tau, dt)
    Rx = scatter(energy(W.astype(cdt)), kk, mm, keep)[0].astype(rdt) if squeeze else None
    out = (W, w, tau, np.where(keep, kk, -1), np.where(keep, mm, -1), Rx)
    if details:
        out += (dict(im1=im1, offset=off, keep=keep),)
    return out


def ridge_cells(na, N, rows_cols, reach=1):
    """Boolean [na, N] mask of the cells within +-`reach` (in both directions) of the listed (row, column) pairs."""
    mask = np.zeros((na, N), dtype=bool)
    r, c = (np.asarray(a, dtype=np.int64) for a in rows_cols)
    for dr in range(-reach, reach + 1):
        for dc in range(-reach, reach + 1):
            rr, cc = r + dr, c + dc
            ok = (rr >= 0) & (rr < na) & (cc >= 0) & (cc < N)
            mask[rr[ok], cc[ok]] = True
    return mask
