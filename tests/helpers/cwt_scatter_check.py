"""Per-cell checks of `_rs.ssq_cwt` against its own debug planes and the fp64 oracle (tests/test_gpu_cwt_tiles.py and
the scatter line of tests/test_gpu_cwt.py).

Every bound below is derived from the code or taken from where it is already established; none is a measured number.

**Scatter (`assert_scatter_cells`).**  Cell (k, j) of Tx receives the terms Wx[i, j] (Lebesgue: float32(1 / na)) of the
rows i with dbg k[i, j] == k.  However the kernels split those n terms between run accumulators, read-modify-writes and
launches, each real sum is n - 1 additions of T numbers (0 + v is exact), so by the recursive-summation bound
|Tx - S| <= (n - 1) u / (1 - (n - 1) u) * sum|term| with u = 2^-24 (fp32) or 2^-53 (fp64); the tests use
n * 2 u * sum|term| (a factor below 2 of slack), per real and per imaginary part, with sum|term| of that part.
n == 0: exactly zero (a stray write, an incomplete clear); n == 1: the term itself, bit for bit up to the sign of a
zero (a first flush is 0 + v, and 0 + (-0) is +0).  A cell that is not a number fails like any other (`~(err <= bound)`).
The reference sums S and sum|term| are accumulated one precision above T -- float64 for fp32 results, long double
(x87 extended, u = 2^-64) for fp64 results -- so their own rounding, at most (n - 1) u_S sum|term|, is below 2^-11 of
the bound and the slack stated above is what the kernel gets.

**w from Wx, dWx (`C_W`).**  `reassign_bin` (csrc/cwt_bin.h), fp32 branch, with W = C + iD, dW = A + iB, u = 2^-24 and
hardware reciprocals good to 1 ulp = 2 u:
    sc = rcp(mx)                     -- its error is common to cs, ds and den and CANCELS in the quotient below
    cs = C sc, ds = D sc             -- 1 rounding each
    num = B cs - A ds                -- 2 products + 1 difference (or an fma: fewer); with cs / ds: 3 roundings per term,
                                        relative to |B C| + |A D| <= |dW| |W| (Cauchy-Schwarz): 3 u |dW| |W| sc
    den = C cs + D ds                -- all terms >= 0: 1 (cs / ds) + 1 (product) + 1 (sum) = 3 u relative
    den * two_pi                     -- the constant (float)(2 pi): 1, the product: 1     -> 5 u
    rcp(.)                           -- 1 ulp = 2 u                                        -> 7 u
    num * rcp                        -- 1                                                  -> 8 u on w itself
so |w - w_exact| <= 8 u w + 3 u |dW| / (2 pi |W|) <= 11 u |dW| / (2 pi |W|) to first order (w <= |dW| / (2 pi |W|));
C_W = 12 covers the second-order terms.  Products that underflow (flushed or denormal: at most 2^-126 each) add
3 * 2^-126 / (2 pi |W|).  The fp64 branch divides in IEEE arithmetic: den 2, times two_pi 2, division 1, numerator 2
relative to |dW| |W|: 7 u, C_W64 = 8 with u = 2^-53.

**Keep mask (`C_KEEP`).**  fp32: small = !(mx * sqrt(cs^2 + ds^2) >= gamma): cs carries 2 u (rcp) + 1, its square 7 u,
the sum 8 u, the square root half of that + 2 u (1 ulp) = 6 u, the product 7 u: elements with | |Wx| - gamma | <=
8 u gamma = 4 ulp(fp32) are exempt, counted, and capped at 1e-5 of the elements.  fp64 (hypot, < 1 ulp): 4 * 2^-53.

**Bins.**  Exactly `_check_ssq_cwt`'s rule (profiles/r03_bin_parity.json): o.cwt_bins on the kernel's own w, mismatches
only within 1e-5 (fp32) / 1e-6 (fp64) bins of a rounding boundary, at a rate <= 1e-5 / 1e-4.

**Wx, dWx.**  Every row against o.cwt in fp64, <= 2e-5 of that row's maximum (the bound of the existing tiled tests).
"""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import ssq_oracle as o
from ssqueeze_rs_amd import _rs

C_W = {np.dtype(np.float32): 12.0 * 2.0 ** -24, np.dtype(np.float64): 8.0 * 2.0 ** -53}
C_KEEP = {np.dtype(np.float32): 8.0 * 2.0 ** -24, np.dtype(np.float64): 4.0 * 2.0 ** -53}
SUM_EPS = {np.dtype(np.float32): 2.0 ** -23, np.dtype(np.float64): 2.0 ** -52}
TIE_TOL = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-6}
MISMATCH_RATE = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-4}
EXEMPT_CAP = 1e-5
ROW_TOL = 2e-5


def assert_scatter_cells(Tx, Wx, k, lebesgue, real_dtype):
    """Tx [na, N] against the re-accumulation of Wx [na, N] with the kernel's own bins k [na, N] (-1: dropped), cell by
    cell.  Returns the worst err / bound over the cells with n >= 2, per row [na]: a cell counts for the LAST row that
    added to it (the kernel that finished its sum)."""
    na, N = Tx.shape
    eps = SUM_EPS[np.dtype(real_dtype)]
    acc_t = np.float64 if np.dtype(real_dtype) == np.float32 else np.longdouble    # one precision above the kernel's
    assert np.finfo(acc_t).eps <= eps * 2.0 ** -10
    S = np.zeros((2, na * N), dtype=acc_t)
    A = np.zeros((2, na * N), dtype=acc_t)
    n = np.zeros(na * N, dtype=np.int32)
    last = np.full(na * N, -1, dtype=np.int16)
    cols = np.arange(N, dtype=np.int64)
    leb = acc_t(np.asarray(1.0 / na, dtype=real_dtype))
    for i in range(na):
        m = k[i] >= 0
        idx = k[i][m] * N + cols[m]                      # one term per column of a row: no index repeats
        if lebesgue:
            S[0][idx] += leb
            A[0][idx] += leb
        else:
            re = Wx[i].real[m].astype(acc_t)
            im = Wx[i].imag[m].astype(acc_t)
            S[0][idx] += re
            S[1][idx] += im
            A[0][idx] += np.abs(re)
            A[1][idx] += np.abs(im)
        n[idx] += 1
        last[idx] = i
    worst = np.zeros(na * N)
    nf = np.where(n >= 2, n, 0).astype(acc_t) * acc_t(eps)        # n <= 1: no rounding at all
    for part, T in ((0, Tx.real), (1, Tx.imag)):
        err = np.abs(T.reshape(-1).astype(acc_t) - S[part])
        bound = nf * A[part]
        bad = ~(err <= bound)                            # (not `err > bound`: a NaN cell must fail)
        if bad.any():
            c = int(np.flatnonzero(bad)[0])
            raise AssertionError(
                f"Tx[{c // N}, {c % N}] ({'re' if part == 0 else 'im'}) = {T.reshape(-1)[c]!r}, its {int(n[c])} terms sum "
                f"to {S[part][c]!r} (bound {bound[c]:.3e}); {int(bad.sum())} cells in all, "
                f"{int((bad & (n == 0)).sum())} with no term, {int((bad & (n == 1)).sum())} with one")
        with np.errstate(all="ignore"):
            r = np.where(bound > 0, err / bound, 0.0).astype(np.float64)
        np.maximum(worst, r, out=worst)
    sel = np.flatnonzero(worst > 0.0)
    worst, last = worst[sel], last[sel]
    return np.array([worst[last == i].max(initial=0.0) for i in range(na)])


def assert_bins_follow_w(k, w, freqs, flipud, real_dtype):
    """`_check_ssq_cwt`'s bin rule on the kernel's own w.  Returns the mismatch rate."""
    dt = np.dtype(real_dtype)
    na = freqs.shape[0]
    w_g = w.astype(np.float64)
    b, valid, is_log = o.cwt_bins(w_g, freqs)
    k_model = np.where(valid, (na - 1 - b) if flipud else b, -1)
    mism = k_model != k
    if not mism.any():
        return 0.0
    with np.errstate(all="ignore"):
        if is_log:
            lmin = np.log2(freqs[0])
            lstep = (np.log2(freqs[-1]) - lmin) / (na - 1)
            v = (np.log2(w_g[mism]) - lmin) / lstep
        else:
            lstep = (freqs[-1] - freqs[0]) / (na - 1)
            v = (w_g[mism] - freqs[0]) / lstep
    tie = np.abs(np.abs(v - np.trunc(v)) - 0.5) < TIE_TOL[dt]
    assert tie.all(), f"{int((~tie).sum())} bins differ from the rule away from a rounding boundary"
    rate = float(mism.mean())
    assert rate <= MISMATCH_RATE[dt], rate
    return rate


def assert_w_follows_wx(w, Wx, dWx, gamma, real_dtype):
    """Keep mask and phase transform of the kernel's own Wx / dWx.  Returns (share of exempt elements, worst
    err / bound per row [na])."""
    dt = np.dtype(real_dtype)
    g = float(np.asarray(gamma, dtype=dt))
    W = Wx.astype(np.complex128)
    absW = np.abs(W)
    small = absW < g
    near = np.abs(absW - g) <= C_KEEP[dt] * g
    exempt = float(near.mean())
    assert exempt <= EXEMPT_CAP, exempt
    isinf = np.isposinf(w)
    bad = (isinf != small) & ~near
    assert not bad.any(), f"{int(bad.sum())} elements with w == +inf on the wrong side of |Wx| < gamma, first at " \
                          f"{tuple(np.argwhere(bad)[0])}"
    keep = ~small & ~isinf
    dW = dWx.astype(np.complex128)
    with np.errstate(all="ignore"):
        lim = np.abs(dW) / (2.0 * math.pi * absW)
        w_x = np.abs((dW * np.conj(W)).imag) / (2.0 * math.pi * absW * absW)
        err = np.abs(w.astype(np.float64) - w_x)
        bound = C_W[dt] * lim + (3.0 * 2.0 ** -126 / (2.0 * math.pi * absW) if dt == np.float32 else 0.0)
        ratio = np.where(keep, err / bound, 0.0)
        ratio = np.where(keep & (err == 0.0), 0.0, ratio)
    nan = keep & ~np.isfinite(ratio)
    assert not nan.any(), f"{int(nan.sum())} kept elements whose w is not finite or has a zero bound, first at {tuple(np.argwhere(nan)[0])}"
    rows = ratio.max(axis=1)
    assert rows.max() <= 1.0, f"w off its bound: worst err / bound per row {np.round(rows, 3)}"
    return exempt, rows


def assert_rows_follow_oracle(Wx, dWx, Wx_o, dWx_o, tol=ROW_TOL):
    """Every row of Wx / dWx within `tol` of that row's maximum of the oracle.  Returns the worst ratio per row
    (err / (tol * row max)) of both planes [2, na]."""
    out = np.zeros((2, Wx.shape[0]))
    for p, (a, b) in enumerate(((Wx, Wx_o), (dWx, dWx_o))):
        for i in range(a.shape[0]):
            rm = np.abs(b[i]).max()
            e = np.abs(a[i] - b[i]).max()
            out[p, i] = e / (tol * rm) if rm > 0 else (0.0 if e == 0 else np.inf)
    assert out.max() <= 1.0, f"rows off the oracle by more than {tol} of their maximum: Wx {np.round(out[0], 2)}, " \
                             f"dWx {np.round(out[1], 2)}"
    return out


def oracle_cwt_rows(x, wavelet, scales, fs=None, padtype="reflect", threads=8):
    """(Wx, dWx) of o.cwt in fp64, the rows computed a few at a time on `threads` threads: each row of o.cwt depends on
    its own scale alone, so the result is o.cwt's bit for bit (NumPy's transforms and exp run outside the interpreter
    lock), in a third of the time at 50 rows of 2^20 points."""
    x64 = np.asarray(x, dtype=np.float64)
    scales = np.asarray(scales, dtype=np.float64)

    def rows(idx):
        Wx, _, dWx = o.cwt(x64, wavelet, scales=scales[idx], fs=fs, derivative=True, padtype=padtype)
        return Wx, dWx

    chunks = [c for c in np.array_split(np.arange(len(scales)), max(1, (len(scales) + 4) // 5)) if len(c)]
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(rows, chunks))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def check_ssq_cwt_cells(x, oracle=None, **kw):
    """`_rs.ssq_cwt(x, _debug=True, **kw)` through every check of this module.  `oracle`: (Wx, dWx) of o.cwt for the
    same x / wavelet / scales / fs / padtype if the caller shares one among several calls.  Returns the measured
    figures (dict)."""
    Tx, f, dbg = _rs.ssq_cwt(x, _debug=True, **kw)
    na, N = Tx.shape
    real = x.dtype
    assert dbg["k"].shape == (na, N) and dbg["k"].max() < na and dbg["k"].min() >= -1
    gamma = kw.get("gamma")
    gamma = 10.0 * 2.2204460492503131e-16 if gamma is None else gamma           # ssq_cwt.rs:438-441
    scatter = assert_scatter_cells(Tx, dbg["Wx"], dbg["k"], kw.get("squeezing") == "lebesgue", real)
    rate = assert_bins_follow_w(dbg["k"], dbg["w"], f, kw.get("flipud", True), real)
    exempt, w_rows = assert_w_follows_wx(dbg["w"], dbg["Wx"], dbg["dWx"], gamma, real)
    if oracle is None:
        Wx_o, dWx_o = oracle_cwt_rows(x, kw.get("wavelet", "gmw"), dbg["scales"], kw.get("fs"),
                                      kw.get("padtype", "reflect"))
    else:
        Wx_o, dWx_o = oracle
    rows = assert_rows_follow_oracle(dbg["Wx"], dbg["dWx"], Wx_o, dWx_o)
    return dict(Tx=Tx, f=f, k=dbg["k"], scatter_rows=scatter, bin_mismatch=rate, gamma_exempt=exempt, w_rows=w_rows,
                wx_rows=rows[0], dwx_rows=rows[1])
