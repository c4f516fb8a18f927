"""GPU tests of the local maximum synchrosqueezed CWT, `upstream.lmssq_cwt`, and of `upstream.lmsst_rows`
(csrc/cwt_lmsst.hip), against the numpy model tests/helpers/lmsst_ref.py.

The window maximum is integer work on the call's own `Wx`: it is compared with `np.array_equal`.  `Wx` is held bitwise to
`ssq_cwt2`'s, `w` to the rows' own frequencies, and `Tx` bitwise to the GPU's own `upstream.ssqueeze` of the call's `Wx`
under the call's `w`."""
import ctypes as C
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests import test_gpu_cwt_sst2 as c2
from tests.helpers import lmsst_ref as r
from tests.helpers import msst_cwt_ref as mr

pytestmark = pytest.mark.gpu

FS = c2.FS
GMW = c2.GMW


@functools.lru_cache(maxsize=None)
def _piecewise():
    return np.ascontiguousarray(up.process_scales("log-piecewise", 1024, GMW), dtype=np.float64).reshape(-1)


# (N, scales): 48 log scales at 16 to the octave; a log-piecewise grid from `process_scales`; two rows
CASES = [(700, lambda: c2._log(GMW, 48, 16)), (1024, _piecewise), (300, lambda: c2._log(GMW, 2, 1))]
IDS = ["700-log48", "1024-piecewise", "300-two-rows"]
DTYPES = pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
EACH = pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
EVERY = pytest.mark.parametrize("which", ("one", "default", "top"))


def delta_of(i, which):
    s = CASES[i][1]()
    return {"one": 1, "default": up.lmssq_cwt_default_delta(GMW, s), "top": len(s) - 1}[which]


@functools.lru_cache(maxsize=None)
def gpu(i, rdt, which):
    N, sc = CASES[i]
    out = up.lmssq_cwt(c2.two_chirps(N, i).astype(rdt), GMW, scales=sc(), fs=FS, delta=delta_of(i, which), get_w=True,
                       get_rows=True)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def second_order(i, rdt):
    N, sc = CASES[i]
    out = up.ssq_cwt2(c2.two_chirps(N, i).astype(rdt), GMW, scales=sc(), fs=FS)
    for a in out:
        a.setflags(write=False)
    return out


@DTYPES
@EACH
def test_wx_is_ssq_cwt2s_bit_for_bit(i, rdt):
    Tx, Wx, f, sc, w, rows = gpu(i, rdt, "default")
    Tx2, Wx2, f2, sc2 = second_order(i, rdt)
    assert Wx.dtype == Wx2.dtype and np.array_equal(Wx.view(rdt), Wx2.view(rdt))
    assert np.array_equal(f, f2) and np.array_equal(sc, sc2) and Tx.dtype == Tx2.dtype and Tx.shape == Tx2.shape


@DTYPES
@EVERY
@EACH
def test_rows_are_the_model_on_the_calls_own_wx(i, rdt, which):
    N, scf = CASES[i]
    na = len(scf())
    Tx, Wx, f, sc, w, rows = gpu(i, rdt, which)
    assert Tx.shape == Wx.shape == w.shape == rows.shape == (na, N)
    assert Tx.dtype == Wx.dtype == (np.complex64 if rdt == np.float32 else np.complex128)
    assert w.dtype == f.dtype == sc.dtype == rdt and rows.dtype == np.int32
    gamma = 10 * float(np.finfo(rdt).eps)
    ref = r.cwt_rows(Wx, delta_of(i, which), gamma)
    kept = rows >= 0
    assert np.array_equal(rows[kept], ref[kept]) and rows.max() < na
    # the keep rule runs on the fp64 coefficient: it agrees with |Wx| < gamma except within 1e-6 relative of gamma
    mag = np.abs(Wx.astype(np.complex128))
    clear = np.abs(mag - gamma) > 1e-6 * gamma
    assert np.array_equal(kept[clear], ~(mag < gamma)[clear])
    print("delta %d: %d of %d cells kept, %d left their row" % (delta_of(i, which), kept.sum(), kept.size,
                                                                (rows != np.arange(na)[:, None])[kept].sum()))
    if which == "top":                                            # the window is the column: its first largest row
        assert np.array_equal(rows[kept], np.broadcast_to(r.energy(Wx).argmax(0), rows.shape)[kept])


@DTYPES
@EVERY
@EACH
def test_w_is_the_frequency_of_the_row(i, rdt, which):
    N, scf = CASES[i]
    Tx, Wx, f, sc, w, rows = gpu(i, rdt, which)
    nu_hz = (up.tssq_cwt_row_freqs(GMW, scf()) * FS).astype(rdt)                # rounded once to the call's dtype
    assert np.array_equal(np.isinf(w), rows == -1) and not np.isnan(w).any()
    kept = rows >= 0
    assert np.array_equal(w[kept], nu_hz[rows[kept]])
    assert (w[~kept] == np.inf).all()


@DTYPES
@EVERY
@EACH
def test_tx_is_ssqueeze_of_the_calls_own_outputs(i, rdt, which):
    N, scf = CASES[i]
    Tx, Wx, _, _, w, rows = gpu(i, rdt, which)
    ref, _ = up.ssqueeze(Wx, w, scales=scf(), wavelet=GMW, maprange="peak", ssq_freqs=None, squeezing="sum", flipud=True, fs=FS)
    assert ref.dtype == Tx.dtype and np.array_equal(Tx, ref)
    if i < 2:
        assert not np.array_equal(Tx, second_order(i, rdt)[0])


@DTYPES
@EVERY
def test_on_a_peak_log_grid_the_bin_is_the_reversed_row(rdt, which):
    """Case 0: log scales and a 'peak' log grid; `ssqueeze`'s bin rule on the reported w (the model of the bins:
    msst_cwt_ref.one_step_bins) puts a coefficient on bin na - 1 - rows, so under `flipud` on row `rows` of Tx."""
    N, scf = CASES[0]
    na = len(scf())
    Tx, Wx, f, sc, w, rows = gpu(0, rdt, which)
    s, rc, f_asc, kind, f_idx = up._cwt_freq_grid(scf(), None, None, "peak", N, *up._wavelet(GMW), 1 / FS)
    assert kind == "log"
    bins, _ = mr.one_step_bins(w.astype(np.float64), f_asc, kind, f_idx)
    kept = rows >= 0
    assert np.array_equal(bins[kept], (na - 1 - rows)[kept])
    empty = np.ones((na, N), dtype=bool)
    empty[rows[kept], np.broadcast_to(np.arange(N), rows.shape)[kept]] = False
    assert not Tx[empty].any()                                    # rows of Tx that no coefficient names stay zero


@DTYPES
def test_batch_equals_single_calls_and_is_deterministic(rdt):
    X = np.stack([c2.two_chirps(300, sd) for sd in (11, 12, 13)]).astype(rdt)
    kw = dict(scales=c2._log(GMW, 37, 8), fs=FS, get_w=True, get_rows=True)
    B = up.lmssq_cwt(X, GMW, **kw)
    assert B[0].shape == B[4].shape == B[5].shape == (3, 37, 300)
    for b in range(3):
        one = up.lmssq_cwt(X[b], GMW, **kw)
        for k in (0, 1, 4, 5):
            assert np.array_equal(B[k][b], one[k]), (b, k)
    again = up.lmssq_cwt(X, GMW, **kw)
    for k in (0, 1, 4, 5):
        assert np.array_equal(B[k], again[k]), k


def test_inverts_like_the_second_order_transform():
    N, scf = CASES[0]
    x = c2.two_chirps(N, 0)
    Txl = gpu(0, np.float64, "default")[0]
    Tx2 = second_order(0, np.float64)[0]
    xl, x2 = up.issq_cwt(Txl, GMW), up.issq_cwt(Tx2, GMW)
    print("inverse difference %.3g of max|x|" % (np.abs(xl - x2).max() / np.abs(x).max()))
    assert not np.array_equal(Txl, Tx2)
    assert np.abs(xl - x2).max() <= 1e-9 * np.abs(x).max()


@DTYPES
def test_row_chunks_do_not_change_a_bit(rdt):
    """The host door under a `work_limit_bytes` that leaves room for 5 rows a chunk (chunks end inside a signal) against
    the preferred workspace, every row in one chunk."""
    lib = _lib.load()
    N, scf = CASES[0]
    s = scf()
    na = len(s)
    X = np.stack([c2.two_chirps(N, sd) for sd in (3, 4)]).astype(rdt)
    whole = up.lmssq_cwt(X, GMW, scales=s, fs=FS, get_w=True, get_rows=True)
    code = _lib.SSQ_F32 if rdt == np.float32 else _lib.SSQ_F64
    wcode, p0, p1 = up._wavelet(GMW)
    _, rc, f_asc, kind, f_idx = up._cwt_freq_grid(s, None, None, "peak", N, wcode, p0, p1, 1 / FS)
    nu_hz = np.ascontiguousarray(up.tssq_cwt_row_freqs(GMW, s) * FS)
    mn = C.c_int64(0)
    pref = lib.ssq_lmssq_cwt_workspace_bytes(code, 2, N, na, C.byref(mn))
    P = up.p2up(N)[0]
    limit = 16 * P * (2 + 2 * 5)
    assert mn.value < limit < pref
    cdt = whole[0].dtype
    Tx, Wx = np.empty((2, na, N), cdt), np.empty((2, na, N), cdt)
    w, rows = np.empty((2, na, N), rdt), np.empty((2, na, N), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                                  # noqa: E731
    _lib.check(lib.ssq_lmssq_cwt_host(code, vp(X), 2, N, wcode, p0, p1, vp(s), na, 1 / FS, vp(rc), vp(f_asc), up.FREQS[kind],
                                      f_idx or 0, 0, 0, -1.0, up.VARIANT_FLIPUD, limit,
                                      up.lmssq_cwt_default_delta(GMW, s), vp(nu_hz), vp(Tx), vp(Wx), vp(w), vp(rows)))
    for k, (a, b) in enumerate(zip((Tx, Wx, w, rows), (whole[0], whole[1], whole[4], whole[5]))):
        assert np.array_equal(a, b), k


@DTYPES
def test_degenerate_inputs(rdt):
    sc = c2._log(GMW, 20, 4)
    kw = dict(scales=sc, get_w=True, get_rows=True)
    Tx, Wx, _, _, w, rows = up.lmssq_cwt(np.zeros(200, dtype=rdt), GMW, **kw)
    assert not Tx.any() and not Wx.any() and np.isinf(w).all() and (rows == -1).all()
    x = c2.two_chirps(200, 3).astype(rdt)
    Tx, Wx, _, _, w, rows = up.lmssq_cwt(x, GMW, gamma=1e6, **kw)
    assert np.abs(Wx).max() < 1e6 and not Tx.any() and np.isinf(w).all() and (rows == -1).all()
    na = len(sc)
    f_asc = 0.5 * 2.0 ** ((np.arange(na) - (na - 1)) / 4)       # (given: the 'peak' frequencies of a 4-point grid coincide)
    for xs in (np.full(200, 3.0, dtype=rdt), np.array([1.0, -1.0], dtype=rdt)):    # a constant; N = 2
        Tx, Wx, f, _, w, rows = up.lmssq_cwt(xs, GMW, ssq_freqs=f_asc, **kw)
        assert Tx.shape == rows.shape == (na, len(xs)) and np.isfinite(Tx.view(rdt)).all()
        assert np.array_equal(f, f_asc[::-1].astype(rdt))
        assert np.array_equal(np.isinf(w), rows == -1) and rows.max() < na
        kept = rows >= 0
        assert np.array_equal(rows[kept], r.cwt_rows(Wx, up.lmssq_cwt_default_delta(GMW, sc))[kept])
        ref, _ = up.ssqueeze(Wx, w, scales=sc, ssq_freqs=f_asc, flipud=True)
        assert np.array_equal(Tx, ref, equal_nan=True)


# --------------------------------------------------------------------------------------------- the plane kernel alone
def _maps(R, n, B, rdt):
    rng = np.random.default_rng(R * 1000 + n)
    rnd = rng.random((B, R, n)).astype(rdt)
    ties = (np.round(rng.random((B, R, n)) * 3) / 3).astype(rdt)                  # many exact ties: the lowest row wins
    plateau = np.zeros((B, R, n), dtype=rdt)
    plateau[:, R // 3:R // 3 + 4] = 5                                             # equal values on up to four rows
    first = rnd.copy()
    first[:, 0] = 7                                                               # the maximum on the first row
    last = rnd.copy()
    last[:, -1] = 7                                                               # and on the last
    return dict(random=rnd, ties=ties, plateau=plateau, first=first, last=last, zeros=np.zeros((B, R, n), dtype=rdt))


@DTYPES
@pytest.mark.parametrize("R,n,B", [(2, 257, 1), (9, 257, 3), (9, 1, 1), (2049, 20, 2)],
                         ids=["2x257", "9x257x3", "9x1", "2049x20x2"])
def test_lmsst_rows_follows_the_definition(R, n, B, rdt):
    """n = 257: one past the edge of a workgroup's 256 columns."""
    for name, A in _maps(R, n, B, rdt).items():
        for delta in sorted({1, min(R - 1, 3), min(R - 1, 256)}):
            got = up.lmsst_rows(A, delta)
            assert got.dtype == np.int32 and got.shape == A.shape
            ref = r.rows_of(A, delta)
            assert np.array_equal(got, ref), (name, delta, int((got != ref).sum()))
    A2 = _maps(R, n, B, rdt)["ties"][0]                                           # a 2-D map
    assert np.array_equal(up.lmsst_rows(A2, 1), r.rows_of(A2, 1))
    assert np.array_equal(r.rows_of(A2[:, :3], 1), r.rows_brute(A2[:, :3], 1))    # (the model itself)
