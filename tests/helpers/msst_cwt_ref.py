"""Numpy model of the multisynchrosqueezed CWT (`upstream.mssq_cwt`) on top of tests/helpers/cwt_sst2_ref.py.
No GPU, no library.

Per column, with na rows (scales ascending), w[i] the one-step frequency of row i (order 2: `cwt_sst2_ref`'s w2; order 1:
its first-order frequency on every element; inf where |W| < gamma), b[i] the one-step bin of w[i] (unflipped, -1 where w is
infinite) and rho[beta] the row nearest in log2 frequency to bin beta (`row_of_bin`):
    r1[k] = k (kept k);    r(i+1)[k] = rho[b[ri[k]]] if b[rho[b[ri[k]]]] >= 0, else ri[k]             (i = 1 .. n_iter - 1)
    w_n[k] = w[r_n[k]], inf where k is not kept;    Tx = the rows-ascending scatter of W row_const under the bins of w_n
(flipped last, with `flipud`): a coefficient lands on b[r_n[k]] with its own row weight."""
from __future__ import annotations

import numpy as np

from tests.helpers import cwt_sst2_ref as m


def row_freqs(wavelet, scales):
    """nu [na], cycles/sample: the peak frequency of every row, wc / (2 pi scale); wavelet ('gmw', gamma, beta) or
    ('morlet', mu)."""
    wc = m.gmw_wc(float(wavelet[1]), float(wavelet[2])) if wavelet[0] == "gmw" else float(wavelet[1])
    return wc / (2 * np.pi * np.asarray(scales, dtype=np.float64).reshape(-1))


def row_of_bin(nu, f_asc):
    """rho [len(f_asc)] int64: the row i minimising |log2 nu_i - log2 f_asc[beta]|, the lowest i on a tie; a bin with
    f_asc[beta] <= 0 takes the row of the lowest nu.  float64."""
    nu, f = np.asarray(nu, dtype=np.float64), np.asarray(f_asc, dtype=np.float64)
    lnu = np.log2(nu)
    out = np.empty(len(f), dtype=np.int64)
    for beta, fb in enumerate(f):
        out[beta] = np.argmin(np.abs(lnu - np.log2(fb))) if fb > 0 else np.argmin(nu)     # (argmin: the first of equals)
    return out


def walk_rows(b, rho, n_iter):
    """The walk by the definition.  b: integer [..., na, n] one-step bins, -1: not kept; rho [na] -> r_n, b's shape, int64,
    -1 where not kept."""
    b = np.asarray(b).astype(np.int64)
    rho = np.asarray(rho).astype(np.int64)
    na, n = b.shape[-2:]
    cols = np.arange(n)
    lead = np.ix_(*[np.arange(s) for s in b.shape[:-2]]) if b.ndim > 2 else ()
    lead = tuple(a[..., None, None] for a in lead)
    kept = b >= 0
    r = np.broadcast_to(np.arange(na)[:, None], b.shape).copy()
    for _ in range(int(n_iter) - 1):
        nxt = rho[np.maximum(b[lead + (r, cols)], 0)]            # rho[b[r]]: r is kept wherever the result is used
        ok = kept & (b[lead + (nxt, cols)] >= 0)
        r = np.where(ok, nxt, r)
    return np.where(kept, r, -1)


def gather(w, rows):
    """w_n = w[r_n] along axis -2, inf where r_n < 0."""
    w = np.asarray(w)
    g = np.take_along_axis(w, np.maximum(rows, 0), axis=-2)
    return np.where(rows >= 0, g, np.inf).astype(w.dtype)


def one_step_bins(w, f_asc, kind, f_idx=None):
    """`upstream.ssqueeze`'s rule on w in float64, unflipped -> (bins int64, -1 where w is infinite; v: the positions)."""
    b, v = m.bin_positions(np.asarray(w, dtype=np.float64), f_asc, kind, f_idx)
    return np.where(np.isinf(w), -1, b), v


def scatter(W, bins, row_const=None, squeezing="sum"):
    """The rows-ascending scatter of `cwt_sst2_ref`: Tx[bins[i, j], j] += W[i, j] row_const[i] (1 / na for 'lebesgue')
    wherever bins[i, j] >= 0, rows i ascending, complex128."""
    na, N = W.shape
    rc = np.ones(na) if row_const is None else np.asarray(row_const, dtype=np.float64)
    add = (np.full((na, N), 1.0 / na) if squeezing == "lebesgue" else W.astype(np.complex128)) * rc[:, None]
    Tx = np.zeros((na, N), dtype=np.complex128)
    cols = np.arange(N)
    for i in range(na):
        k = bins[i] >= 0
        Tx[bins[i, k], cols[k]] += add[i, k]
    return Tx


def mssq_cwt_ref(x, wavelet, scales, f_asc, kind="log", f_idx=None, row_const=None, dt=1.0, padtype="reflect",
                 squeezing="sum", gamma=None, flipud=False, order=2, n_iter=4, arith="fft", tabs=None):
    """-> (W, w, b, rows, w_n, Tx): W [na, N] complex128; w the one-step frequency (inf where not kept); b its bins
    (unflipped, -1 where not kept); rows r_n (-1 where not kept); w_n = w[r_n]; Tx complex128 (flipped with `flipud`)."""
    W, w2, _, _, det = m.cwt_sst2_ref(x, wavelet, scales, f_asc, kind, f_idx, row_const, dt=dt, padtype=padtype,
                                      squeezing=squeezing, gamma=gamma, flipud=False, arith=arith, tabs=tabs, details=True)
    if order == 2:
        w = w2
    elif order == 1:
        w = np.where(np.isinf(w2), np.inf, det["w1"])
    else:
        raise ValueError(order)
    na = len(W)
    b, _ = one_step_bins(w, f_asc, kind, f_idx)
    rho = row_of_bin(row_freqs(wavelet, scales) / dt, f_asc)
    rows = walk_rows(b, rho, n_iter)
    w_n = gather(w, rows)
    final, _ = one_step_bins(w_n, f_asc, kind, f_idx)            # = b[r_n]
    if flipud:
        final = np.where(final >= 0, na - 1 - final, -1)
    return W, w, b, rows, w_n, scatter(W, final, row_const, squeezing)


def top_cell_share(Tx, margin=128):
    """DESIGN 4.17's measure: the share of each column's |Tx|^2 in the column's largest cell, over columns
    margin .. N - margin."""
    P = np.abs(Tx[:, margin:Tx.shape[1] - margin]) ** 2
    return float(P.max(0).sum() / P.sum())


# ------------------------------------------------------------------------------- the model signal of DESIGN 4.20's table
FM_WAVELET = ("gmw", 3.0, 60.0)
FM_NV, FM_NA, FM_N = 32, 127, 1024


def fm_case(grid="peak", noise=0.0, seed=0):
    """-> (x, scales, f_asc, row_const): the sinusoidal FM 0.2 + 0.1 sin(2 pi 3 t / N) cycles/sample, N = 1024, under
    GMW(3, 60) on 127 log scales at nv = 32 whose rows run from 0.45 down to 0.03 cycles/sample; 'peak' frequencies: the
    log grid between the last and the first row's frequency (the rows', reversed); 'maximal': `log_freqs(N, na)`."""
    from tests.helpers import msst_ref
    x, _ = msst_ref.fm_signal(FM_N, f0=0.2, depth=0.1, cycles=3)
    if noise:
        x = x + noise * np.random.default_rng(seed).standard_normal(FM_N)
    scales = m.gmw_wc(*FM_WAVELET[1:]) / (2 * np.pi * 0.45) * 2.0 ** (np.arange(FM_NA) / FM_NV)
    nu = row_freqs(FM_WAVELET, scales)
    if grid == "peak":
        f_asc = nu[-1] * np.power(nu[0] / nu[-1], np.arange(FM_NA) / (FM_NA - 1))
    else:
        f_asc = m.log_freqs(FM_N, FM_NA)
    return x, scales, f_asc, np.full(FM_NA, np.log(2) / FM_NV)
