"""GPU tests of ConceFT, the multitaper synchrosqueezed CWT `upstream.conceft_cwt` (csrc/cwt_conceft.hip),
against the numpy model tests/helpers/conceft_ref.py.

The planes are `cwt_higher_order`'s (held bitwise), so the squeeze is checked on the call's OWN planes: the model forms
the draws from them in fp64.  Bins compare outside ties (a fractional bin within 1e-9 of a half in fp64, the project's
width; in fp32 within the rounding of the bin position itself) and on strong coefficients (|W^(m)| >= 1e-2 of the draw's
maximum); sums compare within M na eps sum|terms| of the cell, the bound of any order of the additions."""
import ctypes as C
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.helpers import conceft_ref as cr
from tests.helpers import cwt_sst2_ref as m2

pytestmark = pytest.mark.gpu

FS = 2.0
GMW = ("gmw", {"gamma": 3.0, "beta": 60.0})
S0 = m2.gmw_wc(3.0, 60.0) / np.pi                  # the scale whose peak sits at Nyquist


def _log(count, nv):
    return S0 * 2.0 ** (np.arange(count) / nv)


@functools.lru_cache(maxsize=None)
def _piecewise():
    return np.ascontiguousarray(up.process_scales("log-piecewise", 777, GMW, nv=8), dtype=np.float64).reshape(-1)


# (N, scales, J, M, padtype, extra keywords)
CASES = [
    (300, lambda: _log(37, 8), 3, 5, "reflect", dict()),
    (40, lambda: _log(20, 4), 2, 1, "zero", dict(flipud=False)),
    (1000, lambda: np.linspace(2, 60, 50), 4, 8, "symmetric", dict(maprange="maximal")),
    (777, _piecewise, 3, 7, "wrap", dict()),
    (2500, lambda: _log(12, 2), 2, 33, "replicate", dict()),
]
IDS = ["300-log37-J3-M5-reflect", "40-log20-J2-M1-zero", "1000-linear50-J4-M8-symmetric", "777-piecewise-J3-M7-wrap",
       "2500-log12-J2-M33-replicate"]
RDTS = [np.float64, np.float32]
RIDS = ["f64", "f32"]


def two_chirps(N, seed=0):
    """Two crossing linear chirps (0.1 -> 0.4 and 0.4 -> 0.1 cycles/sample) plus 1e-3 seeded noise."""
    a, _ = m2.chirp(N, 0.1, 0.4)
    b, _ = m2.chirp(N, 0.4, 0.1)
    return a + b + 1e-3 * np.random.default_rng(seed).standard_normal(N)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _eps(rdt):
    return float(np.finfo(rdt).eps)


def adm(J):
    return np.array([up.gmw_adm_ssq(3.0, 60.0, k) for k in range(J)])


@functools.lru_cache(maxsize=None)
def case_vectors(i):
    """The gauged unit vectors of case i and their c_m."""
    _, _, J, M, _, _ = CASES[i]
    r = up.conceft_vectors(M, J, 100 + i, adm(J))
    r, c = cr.gauge(r, adm(J))
    r.setflags(write=False)
    return r, c


def grids(i):
    """(scales, row_const, f_asc, kind, f_idx) of case i, as `conceft_cwt` derives them."""
    N, sc, J, M, pad, kw = CASES[i]
    code, p0, p1 = up._wavelet(GMW)
    return up._cwt_freq_grid(sc(), None, None, kw.get("maprange", "peak"), N, code, p0, p1, 1 / FS)


@functools.lru_cache(maxsize=None)
def gpu(i, rdt):
    """(Tx, ssq_freqs, scales, Wx [J, na, N], w [M, na, N]) of case i."""
    N, sc, J, M, pad, kw = CASES[i]
    out = up.conceft_cwt(two_chirps(N, i).astype(rdt), GMW, scales=sc(), orders=J, vectors=case_vectors(i)[0], fs=FS,
                         padtype=pad, get_Wx=True, get_w=True, **kw)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def planes(i, rdt):
    """(W, dW) [J, na, N] of case i from `cwt_higher_order(..., derivative=True)`: the call's own planes."""
    N, sc, J, M, pad, kw = CASES[i]
    W, _, dW = up.cwt_higher_order(two_chirps(N, i).astype(rdt), GMW, order=range(J), average=False, derivative=True,
                                   scales=sc(), fs=FS, padtype=pad)
    return np.stack(W), np.stack(dW)


@functools.lru_cache(maxsize=None)
def model(i, rdt):
    """The fp64 model on the call's own planes -> (Tx, W^(m) [M, na, N], w [M, na, N])."""
    N, sc, J, M, pad, kw = CASES[i]
    s, rc, f, kind, f_idx = grids(i)
    r, c = case_vectors(i)
    W, dW = planes(i, rdt)
    out = cr.squeeze_planes(W.astype(np.complex128), dW.astype(np.complex128), r, c, adm(J)[0], f, rc, kind != "linear",
                            kw.get("flipud", True), 10 * _eps(rdt), details=True)
    for a in out:
        a.setflags(write=False)
    return out


def bins_of(w, i, rdt=np.float64):
    """(rows after the flip, v: the positions that were rounded, tie: positions too close to a half to call) of
    frequencies w on case i's grid.  fp64: the project's tie width 1e-9; fp32: the rounding of v itself, v = (log2 w -
    vmin) / dv formed in fp32 from a log2 of 1 ulp: 4 eps32 (|log2 w| + |vmin|) / dv (linear: w and f0)."""
    N, sc, J, M, pad, kw = CASES[i]
    s, rc, f, kind, f_idx = grids(i)
    with np.errstate(all="ignore"):
        k, v = m2.bin_positions(np.asarray(w, dtype=np.float64), f, kind, f_idx)
        width = 1e-9
        if rdt == np.float32:
            mag = np.abs(w) + abs(f[0]) if kind == "linear" else np.abs(np.log2(w)) + abs(np.log2(f[0]))
            dv = f[1] - f[0] if kind == "linear" else np.log2(f[1]) - np.log2(f[0])
            if kind == "log-piecewise":
                dv = min(dv, np.log2(f[f_idx]) - np.log2(f[f_idx - 1]))
            width = np.maximum(4 * _eps(np.float32) * mag / dv, 1e-9)
        tie = np.abs(v - np.floor(v) - 0.5) < width
    if kw.get("flipud", True):
        k = len(f) - 1 - k
    return k, v, tie


def scaled_weights(i, rdt):
    """The row weights as the kernel holds them: row_const C_0 / sum c_m rounded once to the call's dtype."""
    _, _, J, _, _, _ = CASES[i]
    rc = grids(i)[1]
    return (rc * (adm(J)[0] / case_vectors(i)[1].sum())).astype(rdt).astype(np.float64)


def rebuild(w, Wm, weights, i, rdt):
    """Tx from the bins of `w` [M, na, N] and the draws Wm [M, na, N] -> (Tx, S: sum |terms| of every cell, loose: cells a
    tie could move a term into or out of, n_tie)."""
    M, na, N = w.shape
    Tx = np.zeros((na, N), dtype=np.complex128)
    S = np.zeros((na, N))
    loose = np.zeros((na, N), dtype=bool)
    cols = np.arange(N)
    n_tie = 0
    for m in range(M):
        k, _, tie = bins_of(w[m], i, rdt)
        keep = np.isfinite(w[m]) | np.isnan(w[m])
        for r in range(na):
            q = keep[r]
            t = Wm[m, r, q] * weights[r]
            np.add.at(Tx, (k[r, q], cols[q]), t)
            np.add.at(S, (k[r, q], cols[q]), np.abs(t))
            z = q & tie[r]
            n_tie += int(z.sum())
            for d in (-1, 0, 1):
                loose[np.clip(k[r, z] + d, 0, na - 1), cols[z]] = True
    return Tx, S, loose, n_tie


@pytest.mark.parametrize("rdt", RDTS, ids=RIDS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_planes_are_cwt_higher_orders(i, rdt):
    """The get_Wx planes are bitwise those of `cwt_higher_order(average=False)`, with or without its derivative."""
    N, sc, J, M, pad, kw = CASES[i]
    Tx, ssq_freqs, scales, Wx, w = gpu(i, rdt)
    s, rc, f, kind, f_idx = grids(i)
    cdt = np.complex64 if rdt == np.float32 else np.complex128
    assert Tx.shape == (len(s), N) and Wx.shape == (J, len(s), N) and w.shape == (M, len(s), N)
    assert Tx.dtype == Wx.dtype == cdt and w.dtype == ssq_freqs.dtype == scales.dtype == rdt
    assert np.array_equal(scales, s.astype(rdt)) and np.array_equal(ssq_freqs, f[::-1].astype(rdt))
    ref = up.cwt_higher_order(two_chirps(N, i).astype(rdt), GMW, order=range(J), average=False, scales=sc(), fs=FS,
                              padtype=pad)[0]
    assert np.array_equal(Wx, np.stack(ref))
    assert np.array_equal(Wx, planes(i, rdt)[0])


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_bins_float64(i):
    """Every draw's w against the model on the call's own planes: the infinities agree, no strong non-tie coefficient
    lands in another bin, ties are at most 1e-3 of the strong coefficients."""
    Tx, _, _, Wx, w = gpu(i, np.float64)
    _, Wm, wm = model(i, np.float64)
    assert np.array_equal(np.isinf(w), np.isinf(wm))
    strong = np.abs(Wm) >= 1e-2 * np.abs(Wm).max(axis=(1, 2), keepdims=True)
    kg, _, _ = bins_of(w, i)
    km, _, tie = bins_of(wm, i)
    fin = np.isfinite(wm)
    nbad = int(((kg != km) & strong & fin & ~tie).sum())
    ntie = int((tie & strong & fin).sum())
    err = np.abs(w - wm)[strong & fin].max()
    print("w err on strong %.3g; bins differ %d, ties %d of %d strong" % (err, nbad, ntie, strong.sum()))
    assert nbad == 0
    assert ntie <= 1e-3 * strong.sum()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_w_float32(i):
    """float32 w on strong coefficients within the forward error of the two combinations and the quotient,
    (J + 4) eps32 (sum_j |r_j||dW_j| |W| + |dW| sum_j |r_j||W_j|) / (2 pi |W|^2) + 1 ulp, of the fp64 model on the widened
    float32 planes.  Measured on an MI355X: the worst ratio 0.14 .. 0.21 over the five cases."""
    N, sc, J, M, pad, kw = CASES[i]
    _, _, _, Wx, w = gpu(i, np.float32)
    _, Wm, wm = model(i, np.float32)
    r, _ = case_vectors(i)
    W, dW = (a.astype(np.complex128) for a in planes(i, np.float32))
    worst = 0.0
    for m in range(M):
        strong = np.abs(Wm[m]) >= 1e-2 * np.abs(Wm[m]).max()
        assert np.isfinite(w[m][strong]).all()
        dWm = cr.combine(dW, r[m])
        sW = sum(abs(r[m, j]) * np.abs(W[j]) for j in range(J))
        sdW = sum(abs(r[m, j]) * np.abs(dW[j]) for j in range(J))
        a = np.abs(Wm[m])
        bound = (J + 4) * _eps(np.float32) * (sdW * a + np.abs(dWm) * sW) / (2 * np.pi * a * a)
        bound = bound + np.spacing(wm[m].astype(np.float32)).astype(np.float64)
        with np.errstate(invalid="ignore"):                     # (inf - inf off the strong coefficients)
            ratio = (np.abs(w[m].astype(np.float64) - wm[m]) / bound)[strong]
        worst = max(worst, float(ratio.max()))
    print("worst |w - w_model| / bound: %.3g" % worst)
    assert worst <= 1.0


@pytest.mark.parametrize("rdt", RDTS, ids=RIDS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_tx_from_the_calls_own_w(i, rdt):
    """Tx rebuilt in numpy from the bins of the returned w, the model's W^(m) on the call's planes and the scale: every
    cell within M na eps sum|terms of that cell|; the cells next to a tie are left out, and ties are at most 1e-3 of the
    kept coefficients."""
    N, sc, J, M, pad, kw = CASES[i]
    Tx, _, _, Wx, w = gpu(i, rdt)
    _, Wm, _ = model(i, rdt)
    ref, S, loose, n_tie = rebuild(w, Wm, scaled_weights(i, rdt), i, rdt)
    na = Tx.shape[0]
    tol = M * na * _eps(rdt) * S
    err = np.abs(Tx.astype(np.complex128) - ref)
    ok = ~loose
    print("worst cell: %.3g of its tolerance; %d ties of %d kept" % ((err[ok] / np.maximum(tol[ok], 1e-300)).max(), n_tie,
                                                                       np.isfinite(w).sum()))
    assert (err[ok] <= tol[ok]).all()
    assert Tx.any()
    assert n_tie <= 1e-3 * np.isfinite(w).sum()


@pytest.mark.parametrize("rdt", RDTS, ids=RIDS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_column_sums(i, rdt):
    """sum_k Tx[k, n] = (C_0 / sum c_m) sum_m sum_j r_mj sum_i row_const[i] W_j[i, n], within M na eps sum|terms| plus
    M na gamma (the coefficients the gamma test drops)."""
    N, sc, J, M, pad, kw = CASES[i]
    Tx, _, _, Wx, w = gpu(i, rdt)
    r, c = case_vectors(i)
    rc = grids(i)[1]
    na = Tx.shape[0]
    scale = adm(J)[0] / c.sum()
    U = (Wx.astype(np.complex128) * rc[None, :, None]).sum(1)                     # [J, N]
    want = scale * (r.sum(0)[:, None] * U).sum(0)
    terms = sum(np.abs(cr.combine(Wx.astype(np.complex128), r[m])) for m in range(M)) * (rc * scale)[:, None]
    tol = M * na * _eps(rdt) * terms.sum(0) + M * na * 10 * _eps(rdt)
    err = np.abs(Tx.astype(np.complex128).sum(0) - want)
    print("worst column: %.3g of its tolerance" % (err / tol).max())
    assert (err <= tol).all()


@pytest.mark.parametrize("rdt", RDTS, ids=RIDS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_degenerate_draw_is_ssqueeze(i, rdt):
    """vectors = [[1, 0, ...]] against `upstream.ssqueeze(W_0, dWx=dW_0)` on the call's planes: the bins of the call's w
    are those of `phase_cwt(W_0, dW_0)` outside ties (the two kernels may contract the phase's products differently: the
    last place of w), cells within na eps sum|terms| (next to a tie: left out)."""
    N, sc, J, M, pad, kw = CASES[i]
    e0 = np.zeros((1, J))
    e0[0, 0] = 1
    Tx, _, _, w = up.conceft_cwt(two_chirps(N, i).astype(rdt), GMW, scales=sc(), orders=J, vectors=e0, fs=FS, padtype=pad,
                                 get_w=True, **kw)
    W, dW = planes(i, rdt)
    ref, _ = up.ssqueeze(W[0], dWx=dW[0], scales=sc(), wavelet=GMW, maprange=kw.get("maprange", "peak"),
                         flipud=kw.get("flipud", True), fs=FS)
    wp = up.phase_cwt(W[0], dW[0], gamma=10 * _eps(rdt))
    both = np.isfinite(w[0]) & np.isfinite(wp)
    assert (np.isfinite(w[0]) != np.isfinite(wp)).sum() <= 1e-3 * w[0].size      # (|W| == gamma exactly: > against >=)
    k1, _, tie = bins_of(w[0], i, rdt)
    k2, _, _ = bins_of(wp, i, rdt)
    assert not ((k1 != k2) & both & ~tie).any()
    rcT = grids(i)[1].astype(rdt).astype(np.float64)
    _, S, loose, n_tie = rebuild(w.astype(np.float64), W[:1].astype(np.complex128), rcT, i, rdt)
    err = np.abs(Tx.astype(np.complex128) - ref.astype(np.complex128))
    tol = Tx.shape[0] * _eps(rdt) * S
    ok = ~loose
    print("w differing at all: %d; cells differing at all: %d; worst %.3g of its tolerance; %d ties"
          % ((w[0][both] != wp[both]).sum(), (err > 0).sum(), (err[ok] / np.maximum(tol[ok], 1e-300)).max(), n_tie))
    assert (err[ok] <= tol[ok]).all()
    assert n_tie <= 1e-3 * both.sum()


@pytest.mark.parametrize("rdt", RDTS, ids=RIDS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_gauge(i, rdt):
    """The vectors times arbitrary unit phases give the same Tx: the gauge takes the phases out again (to rounding)."""
    N, sc, J, M, pad, kw = CASES[i]
    Tx, _, _, Wx, w = gpu(i, rdt)
    r, _ = case_vectors(i)
    ph = np.exp(2j * np.pi * np.random.default_rng(7 + i).random(M))
    Tx2, _, _, w2 = up.conceft_cwt(two_chirps(N, i).astype(rdt), GMW, scales=sc(), orders=J, vectors=r * ph[:, None], fs=FS,
                                   padtype=pad, get_w=True, **kw)
    _, S, loose, _ = rebuild(w, model(i, rdt)[1], scaled_weights(i, rdt), i, rdt)
    moved = int(((bins_of(w2, i)[0] != bins_of(w, i)[0]) & np.isfinite(w) & np.isfinite(w2)).sum())
    err = np.abs(Tx2.astype(np.complex128) - Tx.astype(np.complex128))
    tol = M * Tx.shape[0] * _eps(rdt) * S
    ok = ~loose
    print("cells differing at all: %d; coefficients in another bin: %d; worst %.3g of its tolerance"
          % ((err > 0).sum(), moved, (err[ok] / np.maximum(tol[ok], 1e-300)).max()))
    assert (err[ok] <= tol[ok]).all()


@pytest.mark.parametrize("rdt", RDTS, ids=RIDS)
def test_batch_equals_single_calls(rdt):
    X = np.stack([two_chirps(300, sd) for sd in (11, 12, 13)]).astype(rdt)
    kw = dict(scales=_log(37, 8), orders=3, vectors=case_vectors(0)[0], fs=FS, get_Wx=True, get_w=True)
    B = up.conceft_cwt(X, GMW, **kw)
    assert B[0].shape == (3, 37, 300) and B[3].shape == (3, 3, 37, 300) and B[4].shape == (3, 5, 37, 300)
    for b in range(3):
        one = up.conceft_cwt(X[b], GMW, **kw)
        for k in (0, 3, 4):
            assert np.array_equal(B[k][b], one[k]), (b, k)


@pytest.mark.parametrize("rdt", RDTS, ids=RIDS)
def test_workspace_size_does_not_change_a_bit(rdt):
    """`ssq_conceft_cwt_exec` with the least workspace (one signal per slice) and the preferred one (the batch in one)."""
    lib = _lib.load()
    B, N, na, J = 3, 300, 37, 3
    code = _lib.SSQ_F32 if rdt == np.float32 else _lib.SSQ_F64
    X = np.stack([two_chirps(N, sd) for sd in (11, 12, 13)]).astype(rdt)
    sc = _log(na, 8)
    wcode, p0, p1 = up._wavelet(GMW)
    s, rc, f, kind, f_idx = up._cwt_freq_grid(sc, None, None, "peak", N, wcode, p0, p1, 1 / FS)
    r, c = up._conceft_gauge(case_vectors(0)[0], adm(J))            # what `conceft_cwt` hands the library
    polys = np.ascontiguousarray(up.gmw_order_coefficients(p0, p1, range(J), average=False))
    mn = C.c_int64(0)
    pref = int(lib.ssq_conceft_cwt_workspace_bytes(code, B, N, na, J, C.byref(mn)))
    assert 0 < mn.value < pref == 3 * mn.value
    cdt = np.complex64 if rdt == np.float32 else np.complex128
    M = r.shape[0]
    shapes = [((B, na, N), cdt), ((B, J, na, N), cdt), ((B, M, na, N), rdt)]
    sizes = [int(np.prod(sh)) * np.dtype(dt).itemsize for sh, dt in shapes]       # Tx, Wx, w
    res = []
    for ws in (mn.value, pref):
        bufs = [C.c_void_p() for _ in range(5)]
        try:
            for d, n in zip(bufs, (X.nbytes, ws, *sizes)):
                _lib.check(lib.ssq_dev_malloc(C.byref(d), n))
            _lib.check(lib.ssq_memcpy_h2d(bufs[0], _vp(X), X.nbytes, None))
            ms = C.c_float(-1.0)
            _lib.check(lib.ssq_conceft_cwt_exec(code, bufs[0], B, N, p0, p1, _vp(polys), polys.shape[1], J, _vp(r), M,
                                                float(adm(J)[0] / c.sum()), _vp(s), na, 1 / FS, _vp(rc), _vp(f),
                                                up.FREQS[kind], f_idx or 0, 0, -1.0, up.VARIANT_FLIPUD, bufs[2], bufs[3], bufs[4],
                                                bufs[1], ws, None, C.byref(ms)))
            assert ms.value > 0
            got = [np.empty(sh, dtype=dt) for sh, dt in shapes]
            for a, d in zip(got, bufs[2:]):
                _lib.check(lib.ssq_memcpy_d2h(_vp(a), d, a.nbytes, None))
            _lib.check(lib.ssq_device_sync())
            res.append(got)
        finally:
            for d in bufs:
                if d:
                    lib.ssq_dev_free(d)
    # every output of the device door, the optional ones included, is the host call's bit for bit at either workspace
    ref = up.conceft_cwt(X, GMW, scales=sc, orders=J, vectors=case_vectors(0)[0], fs=FS, get_Wx=True, get_w=True)
    for got in res:
        for k, a in zip((0, 3, 4), got):
            assert np.array_equal(a, ref[k]), k
    # bad arguments are refused before any launch
    assert lib.ssq_conceft_cwt_exec(code, None, B, N, p0, p1, _vp(polys), polys.shape[1], J, _vp(r), r.shape[0], 1.0, _vp(s),
                                    na, 1 / FS, _vp(rc), _vp(f), up.FREQS[kind], f_idx or 0, 0, -1.0, 0, None, None, None, None,
                                    0, None, None) != 0


# ---- the two-component signal of DESIGN 4.18: N = 2048, fs = 1, 96 log scales at nv 16, J = 3, M = 16 ----
NC = 2048
SCALES_C = S0 * 2.0 ** (np.arange(96) / 16)


def test_inversion_float64():
    """`issq_cwt` of the ConceFT Tx of the noise-free signal, on the columns N/8 .. 7N/8.  With x_a the positive-frequency
    half of the signal from its FFT (x = 2 Re x_a: an analytic wavelet sees this half, so sum_i row_const[i] W[i] ~ C x_a
    and issq_cwt's 2 / C_0 restores x) and U_j = sum_i row_const[i] W_j[i],
    |issq_cwt(Tx) - x| <= (2 / sum c_m) sum_m sum_j |r_mj| |U_j - C_kj x_a| plus the rounding of the column sums (the
    triangle inequality of the definition: a wrong C_k, gauge or scale breaks it).
    Measured on an MI355X (M = 20, vector seed 0): relative L2 error 4.52e-5 beside 1.07e-4 for `ssq_cwt` order 0; the
    worst column at 0.288 of its bound."""
    N, J, M = NC, 3, 20
    x, _, _ = cr.noisy_pair(N)
    r = up.conceft_vectors(M, J, 0, adm(J))
    r, c = cr.gauge(r, adm(J))
    Tx, f, s, Wx = up.conceft_cwt(x, GMW, scales=SCALES_C, orders=J, vectors=r, get_Wx=True)
    xr = up.issq_cwt(Tx, GMW)
    wcode, p0, p1 = up._wavelet(GMW)
    rc = up._cwt_freq_grid(SCALES_C, None, None, "peak", N, wcode, p0, p1, 1.0)[1]
    X = np.fft.fft(x)
    X[N // 2 + 1:] = 0
    X[0] *= 0.5
    X[N // 2] *= 0.5
    xa = np.fft.ifft(X)
    assert np.abs(2 * xa.real - x).max() <= 1e-13
    U = (Wx * rc[None, :, None]).sum(1)                                           # [J, N]
    D = np.abs(U - adm(J)[:, None] * xa[None, :])
    bound = (2 / c.sum()) * (np.abs(r).sum(0)[:, None] * D).sum(0)
    na = len(SCALES_C)
    terms = sum(np.abs(cr.combine(Wx, r[m])) for m in range(M)) * rc[:, None]
    bound = bound + (2 / c.sum()) * (M * na * _eps(np.float64) * terms.sum(0) + M * na * 10 * _eps(np.float64))
    cols = slice(N // 8, 7 * N // 8)
    err = np.abs(xr - x)
    T0 = up.ssq_cwt(x, GMW, scales=SCALES_C)[0]
    e0 = np.abs(up.issq_cwt(T0, GMW) - x)
    rel = lambda e: float(np.linalg.norm(e[cols]) / np.linalg.norm(x[cols]))       # noqa: E731
    print("relative L2 error: ConceFT %.3g, ssq_cwt order 0 %.3g; worst column %.3g of its bound"
          % (rel(err), rel(e0), (err[cols] / bound[cols]).max()))
    assert (err[cols] <= bound[cols]).all()


@pytest.mark.parametrize("vseed", [3, 11])
@pytest.mark.parametrize("nseed", range(4))
def test_concentration(nseed, vseed):
    """Unit white noise on the two components: the share of |Tx|^2 within +-2 rows of the two true ridges, columns N/8 ..
    7N/8, is at least `ssq_cwt`'s plus 0.02 (the model's gaps: 0.039 .. 0.060, tests/test_conceft_ref.py; an MI355X gives
    the model's shares to the four digits printed: 0.7563 .. 0.7803 against 0.7172 .. 0.7303)."""
    x, f1, f2 = cr.noisy_pair(NC, nseed)
    Tx, f, s = up.conceft_cwt(x, GMW, scales=SCALES_C, orders=3, n_draws=16, seed=vseed)
    T0 = up.ssq_cwt(x, GMW, scales=SCALES_C)[0]
    f_asc = f[::-1].astype(np.float64)
    sc, s0 = cr.ridge_share(Tx, f1, f2, f_asc), cr.ridge_share(T0, f1, f2, f_asc)
    print("ridge share: ConceFT %.4f, ssq_cwt %.4f" % (sc, s0))
    assert sc >= s0 + 0.02


@pytest.mark.parametrize("rdt", RDTS, ids=RIDS)
def test_degenerate_inputs(rdt):
    sc = _log(20, 4)
    kw = dict(scales=sc, orders=2, n_draws=3, seed=1, get_w=True)
    Tx, _, _, w = up.conceft_cwt(np.zeros(200, dtype=rdt), GMW, **kw)
    assert not Tx.any() and np.isinf(w).all()
    Tx, _, _, w = up.conceft_cwt(np.ones(200, dtype=rdt), GMW, **kw)
    assert np.isfinite(Tx.view(rdt)).all()
    Tx, _, _, w = up.conceft_cwt((1e30 * two_chirps(200, 3)).astype(rdt), GMW, **kw)
    assert np.isfinite(Tx.view(rdt)).all() and Tx.any()        # (float32: the phase overflows to NaN, which is row 0)
