"""GPU tests of the second-order synchrosqueezed CWT, `upstream.ssq_cwt2` (csrc/cwt_sst2.hip), against the
numpy model tests/helpers/cwt_sst2_ref.py.

The model runs on the library's own fp64 wavelet tables (`ssq_ssq_cwt2_tables`, held to numpy's by
tests/test_cwt_sst2_surface.py).  Tolerances come from the model's disagreement with itself, never from the kernel: Wx
and the fp64 frequencies may differ from the model by 10 x the difference between the model's FFT and DFT-matrix
arithmetics on the same input (the kernels are a third rounding order: radix-4 Stockham passes, FMA contraction).  The
frequency and bin comparisons run on the bins with |W| >= 1e-2 max|W|: on weaker ones the operator is a quotient of two
small numbers and the model's own arithmetics land in different bins."""
import ctypes as C
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.helpers import cwt_sst2_ref as m

pytestmark = pytest.mark.gpu

FS = 2.0
GMW, MORLET = ("gmw", {"gamma": 3.0, "beta": 60.0}), ("morlet", {"mu": 13.4})
S0 = {"gmw": m.gmw_wc(3.0, 60.0) / np.pi, "morlet": 13.4 / np.pi}      # the scale whose peak sits at Nyquist


def _log(wavelet, count, nv):
    return S0[wavelet[0]] * 2.0 ** (np.arange(count) / nv)


@functools.lru_cache(maxsize=None)
def _piecewise():
    return np.ascontiguousarray(up.process_scales("log-piecewise", 777, MORLET, nv=8), dtype=np.float64).reshape(-1)


# (N, scales, wavelet, padtype, extra keywords)
CASES = [
    (300, lambda: _log(GMW, 37, 8), GMW, "reflect", dict()),
    (40, lambda: _log(MORLET, 20, 4), MORLET, "zero", dict(flipud=False)),
    (1000, lambda: np.linspace(2, 60, 50), GMW, "symmetric", dict(squeezing="lebesgue", maprange="maximal")),
    (777, _piecewise, MORLET, "wrap", dict(maprange="peak")),
    (2500, lambda: _log(GMW, 12, 2), GMW, "replicate", dict()),
]
IDS = ["300-log37-gmw-reflect", "40-log20-morlet-zero", "1000-linear50-gmw-symmetric", "777-piecewise-morlet-wrap",
       "2500-log12-gmw-replicate"]


def two_chirps(N, seed=0):
    """Two crossing linear chirps (0.1 -> 0.4 and 0.4 -> 0.1 cycles/sample) plus 1e-3 seeded noise."""
    a, _ = m.chirp(N, 0.1, 0.4)
    b, _ = m.chirp(N, 0.4, 0.1)
    return a + b + 1e-3 * np.random.default_rng(seed).standard_normal(N)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def lib_tables(wavelet, scales, P):
    """(T0, T1) [na, P] as the library evaluates them on the host (`ssq_ssq_cwt2_tables`)."""
    code, p0, p1 = up._wavelet(wavelet)
    T0, T1 = np.zeros((len(scales), P)), np.zeros((len(scales), P))
    for i, a in enumerate(scales):
        _lib.check(_lib.load().ssq_ssq_cwt2_tables(code, p0, p1, float(a), P, _vp(T0[i]), _vp(T1[i])))
    return T0, T1


def grids(i):
    """(scales, row_const, f_asc, kind, f_idx) of case i: the grids `ssq_cwt2` derives (upstream's Python, shared with
    `ssq_cwt`)."""
    N, sc, wavelet, pad, kw = CASES[i]
    code, p0, p1 = up._wavelet(wavelet)
    return up._cwt_freq_grid(sc(), None, None, kw.get("maprange", "peak"), N, code, p0, p1, 1 / FS)


@functools.lru_cache(maxsize=None)
def model(i, arith="fft", f32=False):
    """The model on case i, on the library's tables; f32: on the float32-rounded input with float32's default gamma."""
    N, sc, wavelet, pad, kw = CASES[i]
    s, rc, f, kind, f_idx = grids(i)
    x = two_chirps(N, i)
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    mw = (wavelet[0], *up._wavelet(wavelet)[1:])
    out = m.cwt_sst2_ref(x, mw, s, f, kind, f_idx, rc, dt=1 / FS, padtype=pad, squeezing=kw.get("squeezing", "sum"),
                         gamma=10 * float(np.finfo(np.float32 if f32 else np.float64).eps), arith=arith,
                         tabs=lib_tables(wavelet, s, m.p2up(N)[0]), details=True)
    for a in out[:4]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gpu(i, rdt):
    N, sc, wavelet, pad, kw = CASES[i]
    out = up.ssq_cwt2(two_chirps(N, i).astype(rdt), wavelet, scales=sc(), fs=FS, padtype=pad, get_w=True, **kw)
    for a in out:
        a.setflags(write=False)
    return out


def strong(W):
    return np.abs(W) >= 1e-2 * np.abs(W).max()


def fp64_bounds(i):
    """(Wx bound relative to max|W|, w2 bound on the strong bins): 10 x the model's 'fft'-against-'dft' disagreement."""
    W, w2m = model(i)[:2]
    Wd, w2d = model(i, "dft")[:2]
    big = strong(W)
    return 10 * np.abs(W - Wd).max() / np.abs(W).max(), 10 * np.abs(w2m - w2d)[big].max()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_parity_float64(i):
    """Wx, w2 and the bins against the model.  Measured on an MI355X: Wx 2.7e-16 ... 6.5e-16 of its maximum against bounds
    of 5.6e-15 ... 1.3e-14; the w2 error on strong bins 3.5e-13 ... 1.9e-10 against bounds of 3.8e-12 ... 1.1e-9 (closest:
    1000-linear50, 1.9e-10 against 9.0e-10); no bin differs and no strong bin is a tie."""
    N, sc, wavelet, pad, kw = CASES[i]
    s, rc, f, kind, f_idx = grids(i)
    W, w2m, binm, _, d = model(i)
    tolW, tolw = fp64_bounds(i)
    Tx, Wx, ssq_freqs, scales, w2 = gpu(i, np.float64)
    assert Tx.shape == Wx.shape == w2.shape == W.shape == (len(s), N)
    assert Tx.dtype == Wx.dtype == np.complex128 and w2.dtype == ssq_freqs.dtype == scales.dtype == np.float64
    assert np.array_equal(scales, s) and np.array_equal(ssq_freqs, f[::-1])
    eW = np.abs(Wx - W).max() / np.abs(W).max()
    big = strong(W)
    ew = np.abs(w2 - w2m)[big].max()
    kk, _ = m.bin_positions(w2, f, kind, f_idx)
    tie = np.abs(d["v"] - np.floor(d["v"]) - 0.5) < 1e-9
    nbad = int(((kk != binm) & big & ~tie).sum())
    ntie = int((tie & big).sum())
    print("Wx %.3g (tol %.3g)  w2 err %.3g (tol %.3g, %d strong bins)  bins differ %d, ties %d"
          % (eW, tolW, ew, tolw, big.sum(), nbad, ntie))
    assert eW <= tolW
    assert np.array_equal(np.isinf(w2), np.isinf(w2m))
    assert ew <= tolw
    assert nbad == 0
    assert ntie <= 1e-3 * big.sum()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_parity_float32(i):
    """float32 in, complex64 / float32 out; the kernels compute in fp64 and round once on store: w2 is within the fp64
    bound plus one float32 ulp of the model on the float32-rounded input.  Measured on an MI355X: Wx within 5.1e-8 of its
    maximum, w2 within 0.50 of that bound in every case (the one rounding on store)."""
    W, w2m = model(i, "fft", True)[:2]
    _, tolw = fp64_bounds(i)
    Tx, Wx, ssq_freqs, scales, w2 = gpu(i, np.float32)
    assert Tx.dtype == Wx.dtype == np.complex64 and w2.dtype == ssq_freqs.dtype == scales.dtype == np.float32
    big = strong(W)
    assert np.isfinite(w2[big]).all()
    err = np.abs(w2.astype(np.float64)[big] - w2m[big])
    ulp = np.spacing(w2m[big].astype(np.float32)).astype(np.float64)
    eW = np.abs(Wx - W).max() / np.abs(W).max()
    print("Wx %.3g  w2 err %.3g, worst %.3g of (fp64 bound %.3g + 1 ulp)" % (eW, err.max(), (err / (tolw + ulp)).max(), tolw))
    assert eW <= 2 * float(np.finfo(np.float32).eps)
    assert (err <= tolw + ulp).all()


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_tx_is_ssqueeze_of_the_calls_own_outputs(i, rdt):
    N, sc, wavelet, pad, kw = CASES[i]
    Tx, Wx, _, _, w2 = gpu(i, rdt)
    ref, _ = up.ssqueeze(Wx, w2, scales=sc(), wavelet=wavelet, maprange=kw.get("maprange", "peak"), ssq_freqs=None,
                         squeezing=kw.get("squeezing", "sum"), flipud=kw.get("flipud", True), fs=FS)
    assert ref.dtype == Tx.dtype and np.array_equal(Tx, ref)


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_row_sums(i, rdt):
    """The column sums of Tx are the row-weighted column sums of the call's own kept Wx, to na eps sum|terms|: what
    `issq_cwt` sums, so it inverts a second-order Tx like a first-order one."""
    N, sc, wavelet, pad, kw = CASES[i]
    s, rc, f, kind, f_idx = grids(i)
    Tx, Wx, _, _, w2 = gpu(i, rdt)
    na = len(s)
    rcT = rc.astype(rdt).astype(np.float64)[:, None]
    terms = (np.full(Wx.shape, 1.0 / na) if kw.get("squeezing") == "lebesgue" else Wx.astype(np.complex128)) * rcT
    terms = np.where(np.isinf(w2), 0, terms)
    err = np.abs(Tx.astype(np.complex128).sum(0) - terms.sum(0))
    tol = na * float(np.finfo(rdt).eps) * np.abs(terms).sum(0)
    print("worst column: %.3g of its tolerance" % (err / np.maximum(tol, 1e-300)).max())
    assert (err <= tol).all()


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
def test_batch_equals_single_calls(rdt):
    X = np.stack([two_chirps(300, sd) for sd in (11, 12, 13)]).astype(rdt)
    kw = dict(scales=_log(GMW, 37, 8), fs=FS, get_w=True)
    B = up.ssq_cwt2(X, GMW, **kw)
    assert B[0].shape == B[1].shape == B[4].shape == (3, 37, 300)
    for b in range(3):
        one = up.ssq_cwt2(X[b], GMW, **kw)
        for k in (0, 1, 4):
            assert np.array_equal(B[k][b], one[k]), (b, k)


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
def test_chunking_does_not_change_a_row(rdt):
    """`work_limit_bytes` for 16 rows per chunk: the 2 x 37 rows go as 16 + 16 + 16 + 16 + 10, one chunk across the two
    signals, the last one partial."""
    lib = _lib.load()
    B, N, na = 2, 300, 37
    code = _lib.SSQ_F32 if rdt == np.float32 else _lib.SSQ_F64
    X = np.stack([two_chirps(N, sd) for sd in (21, 22)]).astype(rdt)
    sc = _log(GMW, na, 8)
    wcode, p0, p1 = up._wavelet(GMW)
    s, rc, f, kind, f_idx = up._cwt_freq_grid(sc, None, None, "peak", N, wcode, p0, p1, 1 / FS)
    mn = C.c_int64(0)
    assert lib.ssq_ssq_cwt2_workspace_bytes(code, B, N, na, C.byref(mn)) > 0
    P = m.p2up(N)[0]
    limit = mn.value + 15 * 160 * P
    res = []
    for lim in (0, limit, mn.value):
        Tx, Wx = (np.empty((B, na, N), dtype=np.complex64 if rdt == np.float32 else np.complex128) for _ in range(2))
        w2 = np.empty((B, na, N), dtype=rdt)
        _lib.check(lib.ssq_ssq_cwt2_host(code, _vp(X), B, N, wcode, p0, p1, _vp(s), na, 1 / FS, _vp(rc), _vp(f), up.FREQS[kind],
                                         f_idx or 0, 0, 0, -1.0, up.VARIANT_FLIPUD, lim, _vp(Tx), _vp(Wx), _vp(w2)))
        res.append((Tx, Wx, w2))
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert np.array_equal(a, b)
    ref = up.ssq_cwt2(X, GMW, scales=sc, fs=FS, get_w=True)
    assert np.array_equal(res[0][0], ref[0]) and np.array_equal(res[0][2], ref[4])


def test_concentrates_a_chirp_where_first_order_smears_it():
    """The chirp of DESIGN 4.12's table (0.02 -> 0.45 cycles/sample, N = 512, GMW(3, 60), scales s0 2^(k/32), k < 180,
    'maximal' log frequencies): the share of |Tx|^2 on the chirp's own bin over columns N/5 .. 4N/5."""
    N = 512
    x, fi = m.chirp(N, 0.02, 0.45)
    sc = _log(GMW, 180, 32)
    f = m.log_freqs(N, len(sc))
    own, _ = m.bin_positions(fi, f, "log")
    c = np.arange(N // 5, 4 * N // 5)

    def share(Tx):
        E = np.abs(Tx) ** 2
        return E[own[c], c].sum() / E[:, c].sum()
    kw = dict(scales=sc, maprange="maximal", flipud=False)
    out2 = up.ssq_cwt2(x, GMW, **kw)
    assert np.allclose(out2[2][::-1], f, rtol=1e-14)
    s2, s1 = share(out2[0]), share(up.ssq_cwt(x, GMW, **kw)[0])
    print("own-bin share: second order %.4f, first order %.4f" % (s2, s1))
    assert s2 >= 0.99
    assert s1 <= 0.9


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
def test_degenerate_inputs(rdt):
    sc = _log(GMW, 20, 4)
    Tx, Wx, _, _, w2 = up.ssq_cwt2(np.zeros(200, dtype=rdt), GMW, scales=sc, get_w=True)
    assert not Tx.any() and not Wx.any() and np.isinf(w2).all()
    x = two_chirps(200, 3).astype(rdt)
    Tx, Wx, _, _, w2 = up.ssq_cwt2(x, GMW, scales=sc, gamma=1e6, get_w=True)
    assert np.abs(Wx).max() < 1e6 and not Tx.any() and np.isinf(w2).all()
    Tx, Wx, _, _, w2 = up.ssq_cwt2(x, GMW, scales=sc, get_w=True)
    assert np.isfinite(Tx.view(rdt)).all() and Tx.any() and not np.isnan(w2).any()
