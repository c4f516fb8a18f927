"""GPU tests of ConceFT on the STFT, `upstream.conceft_stft` (csrc/stft_conceft.hip), against the numpy
model tests/helpers/conceft_stft_ref.py, by the rules of tests/test_gpu_conceft.py.

The planes are checked against `ssq_stft2`'s Sx and the fp64 model; the squeeze is checked on the call's OWN planes: the
model forms the draws from them in fp64.  Bins compare outside ties (a fractional bin within 1e-9 of a half in fp64, the
project's width; in fp32 within the forward error of w itself) and on strong coefficients (|S| >= 1e-2 of the draw's
maximum); sums compare within M F eps sum|terms| of the cell, the bound of any order of the additions."""
import ctypes as C
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.helpers import conceft_ref as cr
from tests.helpers import conceft_stft_ref as cs
from tests.helpers import sst2_ref as s2

pytestmark = pytest.mark.gpu

FS = 2.0
# (N, n_fft, hop, J, M, padtype, extra keywords)
CASES = [
    (300, 16, 1, 2, 1, "zero", dict()),
    (777, 64, 3, 3, 5, "wrap", dict(flipud=True)),
    (1000, 256, 1, 4, 8, "symmetric", dict()),
    (1500, 1024, 7, 3, 9, "reflect", dict(modulated=False)),
    (3000, 2048, 16, 8, 33, "replicate", dict()),
    (5000, 4096, 16, 2, 3, "reflect", dict()),
]
IDS = ["300-16-1-J2-M1-zero", "777-64-3-J3-M5-wrap-flipud", "1000-256-1-J4-M8-symmetric", "1500-1024-7-J3-M9-reflect-unmod",
       "3000-2048-16-J8-M33-replicate", "5000-4096-16-J2-M3-reflect"]
RDTS = [np.float64, np.float32]
RIDS = ["f64", "f32"]


def two_chirps(N, seed=0):
    """Two crossing linear chirps (0.1 -> 0.4 and 0.4 -> 0.1 cycles/sample) plus 1e-3 seeded noise."""
    a, _ = s2.chirp(N, 0.1, 0.4)
    b, _ = s2.chirp(N, 0.4, 0.1)
    return a + b + 1e-3 * np.random.default_rng(seed).standard_normal(N)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _eps(rdt):
    return float(np.finfo(rdt).eps)


def _cdt(rdt):
    return np.complex64 if rdt == np.float32 else np.complex128


@functools.lru_cache(maxsize=None)
def tapers(i):
    N, n, hop, J, M, pad, kw = CASES[i]
    h = up.hermite_windows(n, J)
    h.setflags(write=False)
    return h


def adm(i):
    return tapers(i)[:, CASES[i][1] // 2]


@functools.lru_cache(maxsize=None)
def case_vectors(i):
    """The gauged unit vectors of case i and their c_m."""
    N, n, hop, J, M, pad, kw = CASES[i]
    r, c = cr.gauge(cs.draws(M, J, 100 + i), adm(i))
    r.setflags(write=False)
    return r, c


def call_kw(i):
    N, n, hop, J, M, pad, kw = CASES[i]
    return dict(n_fft=n, hop_len=hop, fs=FS, padtype=pad, **kw)


@functools.lru_cache(maxsize=None)
def gpu(i, rdt):
    """(Tx, ssq_freqs, Sfs, Sx [J, F, nfr], dSx, w [M, F, nfr]) of case i."""
    N = CASES[i][0]
    out = up.conceft_stft(two_chirps(N, i).astype(rdt), tapers(i), vectors=case_vectors(i)[0], get_planes=True, get_w=True,
                          **call_kw(i))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model(i, rdt):
    """The fp64 model on the call's own planes -> (Tx, S [M, F, nfr], w [M, F, nfr])."""
    N, n, hop, J, M, pad, kw = CASES[i]
    r, c = case_vectors(i)
    _, _, _, Sx, dSx, _ = gpu(i, rdt)
    out = cs.squeeze_planes(Sx.astype(np.complex128), dSx.astype(np.complex128), r, c, adm(i)[0], n, FS,
                            kw.get("flipud", False), 10 * _eps(rdt), details=True)
    for a in out:
        a.setflags(write=False)
    return out


def w_bound32(i, m):
    """The forward error of draw m's float32 w on the call's planes: the two combinations and the quotient,
    fs (J + 4) eps32 (sum_j |r_j||dS_j| |S| + |dS| sum_j |r_j||S_j|) / (2 pi |S|^2)."""
    N, n, hop, J, M, pad, kw = CASES[i]
    r, _ = case_vectors(i)
    _, _, _, Sx, dSx, _ = gpu(i, np.float32)
    V, V1 = Sx.astype(np.complex128), dSx.astype(np.complex128)
    S, dS = cr.combine(V, r[m]), cr.combine(V1, r[m])
    sS = sum(abs(r[m, j]) * np.abs(V[j]) for j in range(J))
    sdS = sum(abs(r[m, j]) * np.abs(V1[j]) for j in range(J))
    a = np.abs(S)
    with np.errstate(all="ignore"):
        return FS * (J + 4) * _eps(np.float32) * (sdS * a + np.abs(dS) * sS) / (2 * np.pi * a * a)


def bins_of(w, i, rdt=np.float64, wbound=None):
    """(rows after the flip, tie: positions too close to a half to call) of frequencies w on case i's grid.  fp64: the
    project's tie width 1e-9; fp32: the rounding of the position v = w / dw formed in fp32, 4 eps32 v, plus the forward
    error `wbound` of w where one is given."""
    N, n, hop, J, M, pad, kw = CASES[i]
    F = n // 2 + 1
    dw = 0.5 * FS / (F - 1)
    k, v = cs.bin_positions(w, F, FS)
    with np.errstate(all="ignore"):
        width = 1e-9
        if rdt == np.float32:
            width = np.maximum(4 * _eps(np.float32) * v, 1e-9)
            if wbound is not None:
                width = width + np.nan_to_num(wbound, nan=np.inf) / dw
        tie = ~(np.abs(v - np.floor(v) - 0.5) >= width)
    if kw.get("flipud", False):
        k = F - 1 - k
    return k, tie


def fac_of(i, rdt):
    """The factor as the kernel holds it: dw h_0[c] / sum c_m rounded once to the call's dtype."""
    n = CASES[i][1]
    dw = np.linspace(0, .5 * FS, n // 2 + 1)[1]
    return float(rdt(dw * (adm(i)[0] / case_vectors(i)[1].sum())))


def rebuild(w, S, fac, i, rdt, wbound=None):
    """Tx from the bins of `w` [M, F, nfr] and the draws S [M, F, nfr] -> (Tx, A: sum |terms| of every cell, loose: cells a
    tie could move a term into or out of, n_tie)."""
    M, F, nfr = w.shape
    Tx = np.zeros((F, nfr), dtype=np.complex128)
    A = np.zeros((F, nfr))
    loose = np.zeros((F, nfr), dtype=bool)
    cols = np.broadcast_to(np.arange(nfr), (F, nfr))
    n_tie = 0
    for m in range(M):
        k, tie = bins_of(w[m], i, rdt, None if wbound is None else wbound(m))
        keep = ~np.isinf(w[m])
        t = S[m][keep] * fac
        np.add.at(Tx, (k[keep], cols[keep]), t)
        np.add.at(A, (k[keep], cols[keep]), np.abs(t))
        z = keep & tie
        n_tie += int(z.sum())
        for d in (-1, 0, 1):
            loose[np.clip(k[z] + d, 0, F - 1), cols[z]] = True
    return Tx, A, loose, n_tie


@pytest.mark.parametrize("rdt", RDTS, ids=RIDS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_planes(i, rdt):
    """Sx[j] against `ssq_stft2(x, tapers[j])`'s Sx within 8 log2(n_fft) eps max|Sx[j]| (the same pass structure, rounded
    twice at the most), and Sx[j], dSx[j] against the fp64 model within the project's STFT tolerances, 1e-11 / 2e-6 of the
    plane's maximum.  Measured on an MI355X: bitwise equal to `ssq_stft2`'s Sx in every case and dtype; against the model
    4.6e-16 (n_fft 16) .. 8.7e-14 (n_fft 4096) of the maximum in float64, 4.9e-8 .. 5.4e-8 in float32."""
    N, n, hop, J, M, pad, kw = CASES[i]
    Tx, ssq_freqs, Sfs, Sx, dSx, w = gpu(i, rdt)
    F, nfr = n // 2 + 1, (N - 1) // hop + 1
    assert Tx.shape == (F, nfr) and Sx.shape == dSx.shape == (J, F, nfr) and w.shape == (M, F, nfr)
    assert Tx.dtype == Sx.dtype == dSx.dtype == _cdt(rdt) and w.dtype == ssq_freqs.dtype == Sfs.dtype == rdt
    lin = np.linspace(0, .5 * FS, F)
    assert np.array_equal(Sfs, lin.astype(rdt))
    assert np.array_equal(ssq_freqs, (lin[::-1] if kw.get("flipud") else lin).astype(rdt))
    x = two_chirps(N, i).astype(rdt)
    V, V1 = cs.planes(x.astype(np.float64), tapers(i), n, hop, pad, kw.get("modulated", True))
    rel = 1e-11 if rdt == np.float64 else 2e-6
    bitwise, worst = True, 0.0
    for j in range(J):
        ref = up.ssq_stft2(x, tapers(i)[j], n_fft=n, hop_len=hop, fs=FS, padtype=pad, modulated=kw.get("modulated", True))[1]
        bitwise &= bool(np.array_equal(ref, Sx[j]))
        assert np.abs(Sx[j] - ref).max() <= 8 * np.log2(n) * _eps(rdt) * np.abs(ref).max()
        for P, R in ((Sx[j], V[j]), (dSx[j], V1[j])):
            e = np.abs(P - R).max() / np.abs(R).max()
            worst = max(worst, float(e))
            assert e <= rel
    print("Sx bitwise ssq_stft2's: %s; planes against the model: %.3g of the maximum" % (bitwise, worst))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_bins_float64(i):
    """Every draw's w against the model on the call's own planes: the infinities agree, no strong non-tie coefficient
    lands in another bin, ties are at most 1e-3 of the strong coefficients.  Measured on an MI355X: w within 1.1e-16 ..
    1.1e-14 on strong coefficients, no bin differs and no tie among 2664 .. 2.5 M strong coefficients."""
    w = gpu(i, np.float64)[5]
    _, S, wm = model(i, np.float64)
    assert np.array_equal(np.isinf(w), np.isinf(wm))
    strong = np.abs(S) >= 1e-2 * np.abs(S).max(axis=(1, 2), keepdims=True)
    kg, _ = bins_of(w, i)
    km, tie = bins_of(wm, i)
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
    fs (J + 4) eps32 (sum_j |r_j||dS_j| |S| + |dS| sum_j |r_j||S_j|) / (2 pi |S|^2) + 1 ulp, of the fp64 model on the
    widened float32 planes (k / n_fft and the product with fs = 2 are exact).  Measured on an MI355X: the worst ratio
    0.38 .. 0.50 over the six cases."""
    N, n, hop, J, M, pad, kw = CASES[i]
    w = gpu(i, np.float32)[5]
    _, S, wm = model(i, np.float32)
    worst = 0.0
    for m in range(M):
        strong = np.abs(S[m]) >= 1e-2 * np.abs(S[m]).max()
        assert np.isfinite(w[m][strong]).all()
        bound = w_bound32(i, m) + np.spacing(wm[m].astype(np.float32)).astype(np.float64)
        with np.errstate(invalid="ignore"):                     # (inf - inf off the strong coefficients)
            ratio = (np.abs(w[m].astype(np.float64) - wm[m]) / bound)[strong]
        worst = max(worst, float(ratio.max()))
    print("worst |w - w_model| / bound: %.3g" % worst)
    assert worst <= 1.0


@pytest.mark.parametrize("rdt", RDTS, ids=RIDS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_tx_from_the_calls_own_w(i, rdt):
    """Tx rebuilt in numpy from the bins of the returned w, the model's S on the call's planes and the factor: every cell
    within M F eps sum|terms of that cell|; the cells next to a tie are left out, and ties are at most 1e-3 of the kept
    coefficients.  Measured on an MI355X: the worst cell at 0.0012 .. 0.51 of its tolerance (the closest: 300 x 16, M 1,
    float64); no tie in float64, at most 3082 among 6.4 M kept coefficients in float32."""
    N, n, hop, J, M, pad, kw = CASES[i]
    Tx, w = gpu(i, rdt)[0], gpu(i, rdt)[5]
    _, S, _ = model(i, rdt)
    ref, A, loose, n_tie = rebuild(w, S, fac_of(i, rdt), i, rdt)
    F = Tx.shape[0]
    tol = M * F * _eps(rdt) * A
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
    """sum_k Tx[k, t] = fac sum_m sum_j r_mj sum_k V_j[k, t], within M F eps sum|terms| plus M F gamma (the coefficients
    the gamma test drops).  Measured on an MI355X: the worst column at 1.5e-7 .. 0.049 of its tolerance."""
    N, n, hop, J, M, pad, kw = CASES[i]
    Tx, Sx = gpu(i, rdt)[0], gpu(i, rdt)[3].astype(np.complex128)
    r, c = case_vectors(i)
    F = Tx.shape[0]
    fac = fac_of(i, rdt)
    want = fac * (r.sum(0)[:, None] * Sx.sum(1)).sum(0)
    terms = sum(np.abs(cr.combine(Sx, r[m])) for m in range(M)) * fac
    tol = M * F * _eps(rdt) * terms.sum(0) + M * F * 10 * _eps(rdt)
    err = np.abs(Tx.astype(np.complex128).sum(0) - want)
    print("worst column: %.3g of its tolerance" % (err / tol).max())
    assert (err <= tol).all()


@pytest.mark.parametrize("rdt", RDTS, ids=RIDS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_e0_draw_is_the_first_order_squeeze(i, rdt):
    """vectors = [[1, 0, ...]] against `mssq_stft(x, tapers[0], order=1, n_iter=1)`: the factor is exactly dw; the bins of
    the call's w are those of mssq_stft's w outside ties (float64: the same expression on the same planes; float32:
    mssq_stft forms w in fp64 before it rounds, this kernel in fp32 from the rounded planes, so a tie is as wide as that
    forward error), cells within F eps sum|terms| (next to a tie: left out).  Measured on an MI355X: Sx[0] bitwise
    mssq_stft's Sx; n_fft 16 and 64 in float64: Tx bitwise too; elsewhere the summed runs differ from the row-by-row sum
    in 31 .. 3950 cells, the worst at 0.041 of its tolerance; at most 50 strong ties (float32, n_fft 4096)."""
    N, n, hop, J, M, pad, kw = CASES[i]
    e0 = np.zeros((1, J))
    e0[0, 0] = 1
    x = two_chirps(N, i).astype(rdt)
    Tx, _, _, Sx, dSx, w = up.conceft_stft(x, tapers(i), vectors=e0, get_planes=True, get_w=True, **call_kw(i))
    ref, Sr, _, _, wr = up.mssq_stft(x, tapers(i)[0], order=1, n_iter=1, get_w=True, **call_kw(i))
    assert (np.isinf(w[0]) != np.isinf(wr)).sum() <= 1e-3 * wr.size      # (float32: |V| against gamma before / after rounding)
    both = np.isfinite(w[0]) & np.isfinite(wr)
    wb = None
    if rdt == np.float32:
        V, V1 = Sx[0].astype(np.complex128), dSx[0].astype(np.complex128)
        a = np.abs(V)
        with np.errstate(all="ignore"):
            wb = FS * (1 + 4) * _eps(np.float32) * 2 * np.abs(V1) / (2 * np.pi * a)
            wb = wb + np.spacing(np.abs(wr))
    k1, tie = bins_of(w[0], i, rdt, wb)
    k2, _ = bins_of(wr, i, rdt)
    assert not ((k1 != k2) & both & ~tie).any()
    dw = float(rdt(np.linspace(0, .5 * FS, n // 2 + 1)[1]))
    _, A, loose, n_tie = rebuild(w.astype(np.float64), Sx[:1].astype(np.complex128), dw, i, rdt,
                                 None if wb is None else (lambda m: wb))
    err = np.abs(Tx.astype(np.complex128) - ref.astype(np.complex128))
    tol = Tx.shape[0] * _eps(rdt) * A
    ok = ~loose
    strong = (np.abs(Sx[0]) >= 1e-2 * np.abs(Sx[0]).max()) & both
    print("Sx bitwise: %s; w differing at all: %d; cells differing at all: %d; worst %.3g of its tolerance; %d strong ties"
          % (np.array_equal(Sx[0], Sr), (w[0][both] != wr[both]).sum(), (err > 0).sum(),
             (err[ok] / np.maximum(tol[ok], 1e-300)).max(), (tie & strong).sum()))
    assert (err[ok] <= tol[ok]).all()
    assert (tie & strong).sum() <= 1e-3 * strong.sum()


@pytest.mark.parametrize("rdt", RDTS, ids=RIDS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_gauge(i, rdt):
    """The vectors times arbitrary unit phases give the same Tx: the gauge takes the phases out again (to rounding).
    Measured on an MI355X: no coefficient in another bin, cells within 0.15 of the tolerance in float64; float32:
    bit-identical (the vectors rounded to float32 are the same)."""
    N, n, hop, J, M, pad, kw = CASES[i]
    Tx, w = gpu(i, rdt)[0], gpu(i, rdt)[5]
    r, _ = case_vectors(i)
    ph = np.exp(2j * np.pi * np.random.default_rng(7 + i).random(M))
    Tx2, _, _, w2 = up.conceft_stft(two_chirps(N, i).astype(rdt), tapers(i), vectors=r * ph[:, None], get_w=True, **call_kw(i))
    # float32: the turned vectors round the combinations differently, so both w carry their forward error: a tie is that wide
    wbound = (lambda m: 2 * w_bound32(i, m)) if rdt == np.float32 else None
    _, A, loose, _ = rebuild(w, model(i, rdt)[1], fac_of(i, rdt), i, rdt, wbound)
    moved = int(((bins_of(w2, i)[0] != bins_of(w, i)[0]) & np.isfinite(w) & np.isfinite(w2)).sum())
    err = np.abs(Tx2.astype(np.complex128) - Tx.astype(np.complex128))
    tol = M * Tx.shape[0] * _eps(rdt) * A
    ok = ~loose
    print("cells differing at all: %d; coefficients in another bin: %d; worst %.3g of its tolerance"
          % ((err > 0).sum(), moved, (err[ok] / np.maximum(tol[ok], 1e-300)).max()))
    assert (err[ok] <= tol[ok]).all()


@pytest.mark.parametrize("rdt", RDTS, ids=RIDS)
def test_batch_equals_single_calls(rdt):
    X = np.stack([two_chirps(777, sd) for sd in (11, 12, 13)]).astype(rdt)
    kw = dict(vectors=case_vectors(1)[0], get_planes=True, get_w=True, **call_kw(1))
    B = up.conceft_stft(X, tapers(1), **kw)
    assert B[0].shape == (3, 33, 259) and B[3].shape == B[4].shape == (3, 3, 33, 259) and B[5].shape == (3, 5, 33, 259)
    for b in range(3):
        one = up.conceft_stft(X[b], tapers(1), **kw)
        for k in (0, 3, 4, 5):
            assert np.array_equal(B[k][b], one[k]), (b, k)


@pytest.mark.parametrize("rdt", RDTS, ids=RIDS)
def test_workspace_size_does_not_change_a_bit(rdt):
    """`ssq_conceft_stft_exec` with the least workspace (one store tile of one signal per slice: 63 slices a signal here)
    and the preferred one (the batch in one slice), and an in-between one that holds one signal and a part."""
    lib = _lib.load()
    i = 2
    N, n, hop, J, M, pad, kw = CASES[i]
    B, F, nfr = 3, n // 2 + 1, (N - 1) // hop + 1
    code = _lib.SSQ_F32 if rdt == np.float32 else _lib.SSQ_F64
    X = np.stack([two_chirps(N, sd) for sd in (11, 12, 13)]).astype(rdt)
    wins = np.ascontiguousarray(tapers(i))
    r, c = up._conceft_gauge(case_vectors(i)[0], adm(i))            # what `conceft_stft` hands the library
    scale = float(adm(i)[0] / c.sum())
    mn = C.c_int64(0)
    pref = int(lib.ssq_conceft_stft_workspace_bytes(code, B, N, n, hop, J, C.byref(mn)))
    csz = np.dtype(_cdt(rdt)).itemsize
    wid = 8 * N if rdt == np.float32 else 0
    assert mn.value == wid + 2 * J * F * 16 * csz and pref == 3 * (wid + 2 * J * F * nfr * csz)
    M = r.shape[0]
    shapes = [((B, F, nfr), _cdt(rdt)), ((B, J, F, nfr), _cdt(rdt)), ((B, J, F, nfr), _cdt(rdt)), ((B, M, F, nfr), rdt)]
    sizes = [int(np.prod(sh)) * np.dtype(dt).itemsize for sh, dt in shapes]       # Tx, Sx, dSx, w
    res = []
    for ws in (mn.value, pref, pref // 2):
        bufs = [C.c_void_p() for _ in range(6)]
        try:
            for d, nbytes in zip(bufs, (X.nbytes, ws, *sizes)):
                _lib.check(lib.ssq_dev_malloc(C.byref(d), nbytes))
            _lib.check(lib.ssq_memcpy_h2d(bufs[0], _vp(X), X.nbytes, None))
            ms = (C.c_float * 2)(-1.0, -1.0)
            _lib.check(lib.ssq_conceft_stft_exec(code, bufs[0], B, N, _vp(wins), J, n, hop, FS, up.PAD_MODES[pad], _vp(r),
                                                 M, scale, -1.0, up._variant(True), bufs[2], bufs[3], bufs[4], bufs[5],
                                                 bufs[1], ws, None, ms))
            assert ms[0] > 0 and ms[1] > 0
            got = [np.empty(sh, dtype=dt) for sh, dt in shapes]
            for a, d in zip(got, bufs[2:]):
                _lib.check(lib.ssq_memcpy_d2h(_vp(a), d, a.nbytes, None))
            _lib.check(lib.ssq_device_sync())
            res.append(got)
        finally:
            for d in bufs:
                if d:
                    lib.ssq_dev_free(d)
    # every output of the device door, the optional ones included, is the host call's bit for bit at every workspace
    ref = up.conceft_stft(X, tapers(i), vectors=case_vectors(i)[0], get_planes=True, get_w=True, **call_kw(i))
    for got in res:
        for k, a in zip((0, 3, 4, 5), got):
            assert np.array_equal(a, ref[k]), k
    # bad arguments are refused before any launch
    assert lib.ssq_conceft_stft_exec(code, None, B, N, _vp(wins), J, n, hop, FS, 0, _vp(r), r.shape[0], scale, -1.0, 0, None,
                                     None, None, None, None, 0, None, None) != 0


@pytest.mark.parametrize("rdt", RDTS, ids=RIDS)
def test_past_the_grid_limit(rdt):
    """65537 signals of N = 16, n_fft = 16, hop = 16 (one frame each): two launches of the plane kernel and a squeeze
    grid that strides over the signals; every signal repeats the 7-signal base batch's result."""
    base = np.stack([two_chirps(16, 40 + b) for b in range(7)]).astype(rdt)
    h = up.hermite_windows(16, 2)
    kw = dict(n_fft=16, hop_len=16, fs=FS, n_draws=3, seed=2, get_w=True)
    Tb, _, _, wb = up.conceft_stft(base, h, **kw)
    assert Tb.shape == (7, 9, 1) and Tb.any()
    idx = np.arange(65537) % 7
    T, _, _, w = up.conceft_stft(np.ascontiguousarray(base[idx]), h, **kw)
    assert np.array_equal(T, Tb[idx]) and np.array_equal(w, wb[idx])


# ---- the two-component signal of DESIGN 4.19: N = 2048, fs = 1, n_fft = 256, the default Hermite tapers, J = 3 ----
NC, NFC = 2048, 256


def test_inversion_float64():
    """`issq_stft(Tx, window=tapers[0])` of the ConceFT Tx of the noise-free signal, on the columns N/8 .. 7N/8.  With
    x_a the positive-frequency half of the signal from its FFT (x = 2 Re x_a) and U_j = dw sum_k V_j[k] from the call's
    own planes, |issq_stft(Tx) - x| <= (2 / sum c_m) sum_m sum_j |r_mj| |U_j - h_j[c] x_a| plus the rounding of the column
    sums (the triangle inequality of the definition: a wrong h_j[c], gauge or scale breaks it).
    Measured on an MI355X (M = 20, vector seed 0): relative L2 error 7.15e-10 beside 3.33e-11 for `ssq_stft` with taper
    0; the worst column at 8.7e-6 of its bound (the bound is led by M F gamma, the allowance for dropped coefficients)."""
    N, n, J, M = NC, NFC, 3, 20
    x, _, _ = cr.noisy_pair(N)
    h = up.hermite_windows(n, J)
    a = h[:, n // 2]
    r, c = cr.gauge(cs.draws(M, J, 0), a)
    Tx, f, Sfs, Sx, dSx = up.conceft_stft(x, n_fft=n, n_tapers=J, vectors=r, get_planes=True)
    assert np.array_equal(Tx, up.conceft_stft(x, h, n_fft=n, vectors=r)[0])             # (the default tapers)
    xr = up.issq_stft(Tx, window=h[0])
    X = np.fft.fft(x)
    X[N // 2 + 1:] = 0
    X[0] *= 0.5
    X[N // 2] *= 0.5
    xa = np.fft.ifft(X)
    assert np.abs(2 * xa.real - x).max() <= 1e-13
    F = n // 2 + 1
    dw = float(Sfs[1] - Sfs[0])
    U = Sx.sum(1) * dw                                                            # [J, N]
    D = np.abs(U - a[:, None] * xa[None, :])
    bound = (2 / c.sum()) * (np.abs(r).sum(0)[:, None] * D).sum(0)
    terms = sum(np.abs(cr.combine(Sx, r[m])) for m in range(M)) * dw
    bound = bound + (2 / c.sum()) * (M * F * _eps(np.float64) * terms.sum(0) + M * F * 10 * _eps(np.float64))
    cols = slice(N // 8, 7 * N // 8)
    err = np.abs(xr - x)
    T0 = up.ssq_stft(x, h[0], n_fft=n)[0]
    e0 = np.abs(up.issq_stft(T0, window=h[0]) - x)
    rel = lambda e: float(np.linalg.norm(e[cols]) / np.linalg.norm(x[cols]))       # noqa: E731
    print("relative L2 error: ConceFT %.3g, ssq_stft with taper 0 %.3g; worst column %.3g of its bound"
          % (rel(err), rel(e0), (err[cols] / bound[cols]).max()))
    assert (err[cols] <= bound[cols]).all()


@pytest.mark.parametrize("vseed", [3, 11])
@pytest.mark.parametrize("nseed", range(4))
def test_concentration(nseed, vseed):
    """Unit white noise on the two components: the share of |Tx|^2 within +-2 rows of the two true ridges, columns N/8 ..
    7N/8, is at least `ssq_stft(x, tapers[0])`'s plus 0.02 (the model's gaps: 0.039 .. 0.052,
    tests/test_conceft_stft_ref.py; an MI355X gives the model's shares to the four digits printed: 0.7233 .. 0.7582
    against 0.6841 .. 0.7125)."""
    x, f1, f2 = cr.noisy_pair(NC, nseed)
    h = up.hermite_windows(NFC, 3)
    Tx = up.conceft_stft(x, h, n_fft=NFC, n_draws=16, seed=vseed)[0]
    T0 = up.ssq_stft(x, h[0], n_fft=NFC)[0]
    sc, s0 = cs.ridge_share(Tx, f1, f2), cs.ridge_share(T0, f1, f2)
    print("ridge share: ConceFT %.4f, ssq_stft %.4f" % (sc, s0))
    assert sc >= s0 + 0.02


@pytest.mark.parametrize("rdt", RDTS, ids=RIDS)
def test_degenerate_inputs(rdt):
    kw = dict(n_fft=64, n_tapers=2, n_draws=3, seed=1, get_w=True)
    Tx, _, _, w = up.conceft_stft(np.zeros(200, dtype=rdt), **kw)
    assert not Tx.any() and np.isinf(w).all()
    Tx, _, _, w = up.conceft_stft(np.ones(200, dtype=rdt), **kw)
    assert np.isfinite(Tx.view(rdt)).all()
    Tx, _, _, w = up.conceft_stft((1e30 * two_chirps(200, 3)).astype(rdt), **kw)
    assert np.isfinite(Tx.view(rdt)).all() and Tx.any()        # (float32: |S|^2 overflows, w is NaN, which is row 0)
