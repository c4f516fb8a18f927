"""Numpy model of the synchroextracting and transient-extracting CWT (`upstream.set_cwt`, `upstream.tet_cwt`).
No GPU, no library.  Built ON the models of the transforms whose maps it reads: `cwt_sst2_ref.cwt_sst2_ref(details=True)`
for the frequency map (its `w1` is the first-order frequency) and `tssq_cwt_ref.tssq_cwt_ref(squeeze=False)` for the
group-delay map, with their `arith` / `tabs` switches.  A cell is live unless |W| < gamma (the CWT family's rule).

    set (axis 0): w = `cwt_sst2_ref`'s w2 (order 2) or its w1 on every cell (order 1), rounded once to the real dtype `rdt`,
                  +inf where the cell is not live;  e = `row_edges`: +inf, sqrt(nu[i-1] nu[i]) / dt, 0, float64, each
                  rounded once to `rdt`;  keep where live and e[i+1] <= w < e[i], compared in `rdt`
    tet (axis 1): tau = `tssq_cwt_ref`'s, +inf where the cell is not live;  r = rint(tau / dt) in `rdt`, BEFORE any clip
                  to [0, N - 1];  keep where live and r == 0
    Te = where(keep, W rounded to the complex dtype of `rdt`, +0)
The rules are also exposed on their own (`keep_freq`, `keep_time`, `extract`): a test rebuilds `keep` from the map a call
reports, in the call's dtype, and holds `Te` to it bit for bit.  `maps_in` restates both maps in the arithmetic of one
complex dtype: the parents' models have no complex64 switch, and a float32 map's tolerance is the model's complex64-
against-complex128 disagreement."""
from __future__ import annotations

import numpy as np

from . import cwt_sst2_ref as c2
from . import tssq_cwt_ref as tc


def row_edges(wavelet, scales, dt=1.0):
    """e [na + 1] float64, Hz: +inf, the log midpoints of the rows' frequencies (`tssq_cwt_ref.row_freqs`, which must be
    strictly decreasing), 0.  wavelet: ('gmw', gamma, beta) or ('morlet', mu)."""
    nu = tc.row_freqs(wavelet, scales)
    if len(nu) < 2 or not (np.diff(nu) < 0).all():
        raise ValueError("the rows' frequencies must be strictly decreasing")
    return np.concatenate([[np.inf], np.sqrt(nu[:-1] * nu[1:]) / dt, [0.0]])


def keep_freq(w, edges):
    """SET's keep rule on a reported frequency map `w` [..., na, N] under the edges e [na + 1] (float64, rounded here to w's
    dtype): live (w is not +inf) and e[i+1] <= w < e[i] in w's dtype.  A NaN fails both comparisons."""
    e = np.asarray(edges, dtype=np.float64).astype(w.dtype)
    with np.errstate(invalid="ignore"):
        return ~np.isposinf(w) & (e[1:, None] <= w) & (w < e[:-1, None])


def keep_time(tau, dt):
    """TET's keep rule on a reported offset map `tau`: live (tau is not +inf) and rint(tau / dt) == 0 in tau's dtype."""
    rdt = tau.dtype.type
    with np.errstate(all="ignore"):
        r = np.rint(tau / rdt(dt))
    return ~np.isposinf(tau) & (r == 0)


def extract(W, keep):
    """where(keep, W, +0 + 0i) in W's dtype."""
    return np.where(keep, W, W.dtype.type(0))


def _dtypes(rdt):
    rdt = np.dtype(rdt).type
    return rdt, (np.complex64 if rdt == np.float32 else np.complex128)


def maps_in(x, wavelet, scales, cdt, dt=1.0, padtype="reflect", order=2, gamma=None, tabs=None):
    """(W, w, tau) with EVERY step in the arithmetic of the complex dtype `cdt`, from the rounding of the signal on: the
    forward FFT, the tables, the five product spectra, the inverse FFTs and both operators, written out as the parents
    write them.  In complex128 this is the parents' models bit for bit; in complex64 it is what a test takes the
    float32 tolerance of a map from (the model's complex64-against-complex128 disagreement), nothing else reads it."""
    cdt = np.dtype(cdt).type
    rdt = np.float32 if cdt == np.complex64 else np.float64
    x = np.asarray(x, dtype=np.float64).astype(rdt)
    scales = np.asarray(scales, dtype=np.float64).reshape(-1)
    N, na = len(x), len(scales)
    P, n1, n2 = c2.p2up(N)
    K = P // 2 + 1
    if gamma is None:
        gamma = 10 * float(np.finfo(rdt).eps)
    nu = tc.row_freqs(wavelet, scales).astype(rdt)
    xh = np.fft.fft(np.pad(x, [n1, n2], mode=c2.NP_PAD[padtype]))[:K].astype(cdt)
    T0, T1 = c2.tables(wavelet, scales, P) if tabs is None else tabs
    T0, T1 = np.asarray(T0)[:, :K].astype(rdt), np.asarray(T1)[:, :K].astype(rdt)
    xi = (2 * np.pi * np.arange(K) / P).astype(rdt)
    full = np.zeros((5 * na, P), dtype=cdt)
    full[:, :K] = np.concatenate([xh * T0, xh * (1j * xi) * T0, xh * (-xi * xi) * T0, xh * (-1j) * T1, xh * xi * T1], axis=0)
    maps = np.fft.ifft(full, axis=1)[:, n1:n1 + N].astype(cdt)
    W, W1, W2, Wt, Wt1 = (maps[i * na:(i + 1) * na] for i in range(5))
    with np.errstate(all="ignore"):
        live = ~(np.abs(W) < gamma)
        D = W * W + Wt1 * W - Wt * W1
        num = W2 * W - W1 * W1
        om1 = W1 / W
        om2 = om1 - (num / D) * Wt / W
        use2 = (np.abs(D) > gamma * gamma) & np.isfinite(om2.imag) if order == 2 else np.zeros(W.shape, dtype=bool)
        w = np.where(live, np.abs(np.where(use2, om2.imag, om1.imag)) / rdt(2 * np.pi * dt), np.inf).astype(rdt)
        d1 = (Wt / W).real
        d2 = d1 - ((D / num) * (rdt(2 * np.pi) * nu[:, None] + 1j * W1 / W)).imag
        use2 = (np.abs(num) > gamma * gamma) & np.isfinite(d2) & (np.abs(d2) <= N) if order == 2 else np.zeros(W.shape, dtype=bool)
        off = np.where(use2, d2, d1)
        off = np.where(np.isnan(off), off, np.clip(off, -rdt(N), rdt(N)))
        tau = np.where(live, off * rdt(dt), np.inf).astype(rdt)
    return W, w, tau


def sst2_parent(x, wavelet, scales, dt=1.0, padtype="reflect", gamma=None, arith="fft", tabs=None):
    """`cwt_sst2_ref(..., details=True)` as `set_cwt_ref` calls it (its bins and its scatter are not read); gamma default:
    10 eps of float64."""
    f_asc = c2.log_freqs(len(x), len(np.reshape(scales, -1)), dt)
    return c2.cwt_sst2_ref(x, wavelet, scales, f_asc, "log", dt=dt, padtype=padtype, gamma=gamma, arith=arith, tabs=tabs,
                           details=True)


def set_cwt_ref(x, wavelet, scales, dt=1.0, padtype="reflect", order=2, gamma=None, arith="fft", tabs=None,
                rdt=np.float64, parent=None):
    """-> (Te, W, w, keep): the synchroextracting CWT of the model.  W complex128 (unrounded); w in `rdt` (+inf where a
    cell is not live); Te in the complex dtype of `rdt`.  gamma default: 10 eps of `rdt`.  parent: what
    `cwt_sst2_ref(..., details=True)` returned for these arguments, where the caller holds it (both orders read it)."""
    if order not in (1, 2):
        raise ValueError(order)
    rdt, cdt = _dtypes(rdt)
    if gamma is None:
        gamma = 10 * float(np.finfo(rdt).eps)
    scales = np.asarray(scales, dtype=np.float64).reshape(-1)
    if parent is None:
        parent = sst2_parent(x, wavelet, scales, dt, padtype, gamma, arith, tabs)
    W, w2, _, _, d = parent
    with np.errstate(all="ignore"):
        w = (w2 if order == 2 else np.where(np.abs(W) < gamma, np.inf, d["w1"])).astype(rdt)
    keep = keep_freq(w, row_edges(wavelet, scales, dt))
    return extract(W.astype(cdt), keep), W, w, keep


def tet_cwt_ref(x, wavelet, scales, dt=1.0, padtype="reflect", order=2, gamma=None, arith="fft", tabs=None,
                rdt=np.float64):
    """-> (Te, W, tau, keep): the transient-extracting CWT of the model.  tau in `rdt` (+inf where a cell is not live)."""
    rdt, cdt = _dtypes(rdt)
    W, tau, _, _ = tc.tssq_cwt_ref(x, wavelet, scales, dt=dt, padtype=padtype, order=order, gamma=gamma, arith=arith,
                                   tabs=tabs, rdt=rdt, squeeze=False)
    keep = keep_time(tau, dt)
    return extract(W.astype(cdt), keep), W, tau, keep
