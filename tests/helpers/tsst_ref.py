"""Numpy model of the time-reassigned synchrosqueezed STFT (`upstream.tssq_stft`).  No GPU, no library.

Per-sample units throughout, `fs` enters at the end.  With n = n_fft, F = n//2 + 1, u[j] = j - n//2 and the five window
tables and STFTs V, V1, V2, Vt, Vt1 of `sst2_ref` (frame m centred on sample m hop):
    d1 = Re(Vt / V)                        D = Vt V1 - Vt1 V          num = V2 V - V1^2
    d2 = Re(Vt / V + V1 D / (V num))       the time at which the locally fitted linear chirp crosses frequency k/n
    offset = d2 where order = 2, |num| > gamma^2, d2 is finite and |d2| <= n/2, else d1; clamped to [-n/2, n/2]
    tau    = offset / fs in the real dtype, +inf where |V| <= gamma
    r = rint(tau / (hop / fs)) (0 where not finite)        m' = clip(m + r, 0, n_frames - 1)
    Tx[k, m'] += V[k, m] exp(-2 pi i ((k (m - m') hop) mod n) / n)       in ascending source frame m
Two switches exist so that a test's tolerance can come from the model's disagreement with itself: `arith` = 'fft' or
'dft' and `dtype` = complex128 or complex64 (ALL arithmetic in that precision), as in `sst2_ref`."""
from __future__ import annotations

import numpy as np

from .sst2_ref import NP_PAD, _stft, window_tables


def rotation(k, m, m_to, hop, n, cdt=np.complex128):
    """exp(-2 pi i ((k (m - m_to) hop) mod n) / n): re-references a coefficient's phase from frame m's centre to m_to's."""
    idx = (np.asarray(k, dtype=np.int64) * (np.asarray(m, dtype=np.int64) - np.asarray(m_to, dtype=np.int64)) * hop) % n
    return np.exp(-2j * np.pi * idx / n).astype(cdt)


def targets(tau, hop, fs, cols=None, nfr=None):
    """The target rule on a reported map `tau`, in tau's own dtype -> (m' int64, v); meaningless where tau is inf.
    cols, nfr: the frames the columns of `tau` stand for, of how many (default: all of them)."""
    rdt = tau.dtype.type
    nfr = tau.shape[-1] if nfr is None else nfr
    cols = np.arange(nfr, dtype=np.int64) if cols is None else np.asarray(cols, dtype=np.int64)
    with np.errstate(all="ignore"):
        v = tau / rdt(hop / fs)
        r = np.where(np.isfinite(v), np.rint(v), 0).astype(np.int64)
    return np.clip(cols + r, 0, nfr - 1), v


def scatter(S, tgt, keep, hop, n, acc=np.complex128):
    """Tx of coefficients S [F, n_frames] under targets `tgt`, kept bins only, every cell in ascending source frame.
    acc: complex64 / complex128 (product and sum in that precision), or np.longdouble: the complex128 products summed
    in extended precision, rounded once to complex128 (a reference whose own summation error is out of the way)."""
    F, nfr = S.shape
    kk, mm = np.nonzero(keep)                                 # row-major: ascending source frame inside every row
    to = tgt[kk, mm]
    if acc is np.longdouble:
        z = S[kk, mm].astype(np.complex128) * rotation(kk, mm, to, hop, n)
        re, im = np.zeros((F, nfr), dtype=np.longdouble), np.zeros((F, nfr), dtype=np.longdouble)
        np.add.at(re, (kk, to), z.real.astype(np.longdouble))
        np.add.at(im, (kk, to), z.imag.astype(np.longdouble))
        return re.astype(np.float64) + 1j * im.astype(np.float64)
    cdt = np.dtype(acc).type
    Tx = np.zeros((F, nfr), dtype=cdt)
    np.add.at(Tx, (kk, to), (S[kk, mm].astype(cdt) * rotation(kk, mm, to, hop, n, cdt)).astype(cdt))
    return Tx


def tsst_ref(x, window, n_fft, hop_len=1, fs=1.0, padtype="reflect", modulated=True, order=2, gamma=None, arith="fft",
             dtype=np.complex128, details=False, tables=None, squeeze=True, cols=None):
    """-> (V, tau, tgt, Tx): V [F, n_frames] in `dtype`; tau real, seconds (+inf where a bin is not kept); tgt int64
    target frame (-1 where not kept); Tx in `dtype`.  tables: (g, g1, g2, tg, tg1) float64 to use instead of this
    module's own (a comparison with the library takes the library's: `sst2_ref.sst2_ref`).  details=True appends a dict
    with d1, d2, offset (samples, clamped), num, use2 and keep.  squeeze=False leaves the scatter out (Tx is None);
    cols (with squeeze=False): the frames to compute, for an arithmetic too slow to run on all of them."""
    if order not in (1, 2):
        raise ValueError(order)
    cdt = np.dtype(dtype).type
    rdt = np.float32 if cdt == np.complex64 else np.float64
    x = np.asarray(x, dtype=np.float64)
    N, n, hop = len(x), int(n_fft), int(hop_len)
    F, nfr = n // 2 + 1, (N - 1) // hop + 1
    if gamma is None:
        gamma = 10 * float(np.finfo(rdt).eps)
    gamma = rdt(gamma)
    xp = np.pad(x, [n // 2, n - 1 - n // 2], mode=NP_PAD[padtype]).astype(rdt)
    assert cols is None or not squeeze
    frames = xp[np.arange(n)[:, None] + hop * (np.arange(nfr) if cols is None else np.asarray(cols))[None, :]]
    g, g1, g2, tg, tg1 = window_tables(window, n) if tables is None else tables
    half = rdt(n / 2)
    with np.errstate(all="ignore"):
        if order == 1:
            V, Vt = (_stft(frames, t, modulated, arith, cdt) for t in (g, tg))
            d1 = (Vt / V).real
            d2, num, use2 = d1, np.zeros_like(V), np.zeros(V.shape, dtype=bool)
        else:
            V, V1, V2, Vt, Vt1 = (_stft(frames, t, modulated, arith, cdt) for t in (g, g1, g2, tg, tg1))
            d1 = (Vt / V).real
            D = Vt * V1 - Vt1 * V
            num = V2 * V - V1 * V1
            d2 = (Vt / V + V1 * D / (V * num)).real
            use2 = (np.abs(num) > gamma * gamma) & np.isfinite(d2) & (np.abs(d2) <= half)
        off = np.clip(np.where(use2, d2, d1), -half, half).astype(rdt)
        keep = np.abs(V) > gamma
        tau = np.where(keep, (off.astype(np.float64) / float(fs)).astype(rdt), rdt(np.inf)).astype(rdt)
    tgt, _ = targets(tau, hop, fs, cols, nfr)
    Tx = scatter(V, tgt, keep, hop, n, cdt) if squeeze else None
    out = (V, tau, np.where(keep, tgt, -1), Tx)
    if details:
        out += (dict(d1=d1, d2=d2, offset=off, num=num, use2=use2, keep=keep),)
    return out


def impulses(N, at, height=1.0):
    x = np.zeros(N)
    x[list(at)] = height
    return x
