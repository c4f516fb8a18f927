"""GPU tests of the multisynchrosqueezed CWT, `upstream.mssq_cwt` and `upstream.mssq_cwt_walk` (csrc/cwt_msst.hip, DESIGN
4.20), against the numpy model tests/helpers/msst_cwt_ref.py.

The walk is integer work: it is compared with `np.array_equal`, on frequency maps built by hand (through `mssq_cwt_walk`,
the same kernel) and on the transform's own one-step bins.  The one-step bins are held to the model's rule on the `w` the
call reports, away from rounding ties (the margin is derived in `tie_margin`).  `Tx` is held bitwise to the GPU's own
`upstream.ssqueeze` of the call's `Wx` under w_n = w[rows].  Frequencies of order 1 may differ from the model by 10 x the
difference between the model's FFT and DFT-matrix arithmetics, on the bins with |W| >= 1e-2 max|W| and with the model on the
library's own wavelet tables, as tests/test_gpu_cwt_sst2.py does it."""
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import upstream as up
from tests import test_gpu_cwt_sst2 as c2
from tests.helpers import msst_cwt_ref as r

pytestmark = pytest.mark.gpu

FS = c2.FS
N_ITER = 4
CASES, IDS = c2.CASES[:4], c2.IDS[:4]            # the four grids: log, log unflipped, linear 'maximal' lebesgue, log-piecewise
DTYPES = pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
EACH = pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
ORDERS = pytest.mark.parametrize("order", [2, 1], ids=["o2", "o1"])


# ---------------------------------------------------------------------------------------------- the walk kernel alone
def _freqs(kind, na):
    if kind == "linear":
        return np.linspace(0.0, 0.5, na)
    if kind == "log":                                             # 16 voices, or 8 octaves in all where that is finer
        return 0.5 * 2.0 ** ((np.arange(na) - (na - 1)) * min(1 / 16, 8 / (na - 1)))
    h = na // 2                                                   # 'log-piecewise': 4 voices, then 8, up to 0.5
    lo = np.concatenate([np.arange(h) / 4, (h - 1) / 4 + np.arange(1, na - h + 1) / 8])
    return 0.5 * 2.0 ** (lo - lo[-1])


def walk_shapes():
    """(na, n, B, grid): the smallest column; a tile tail; three tiles and a tail with a batch; the first narrower tile;
    the largest na."""
    return [(9, 1, 1, "log"), (9, 37, 1, "linear"), (33, 3 * up.mssq_cwt_tile_cols(33) + 5, 3, "log-piecewise"),
            (257, up.mssq_cwt_tile_cols(257) + 7, 1, "log-piecewise"), (2049, 20, 2, "log")]


def _w_of(bins, f, rdt):
    """w = f[target] exactly (every position an integer, away from any rounding tie), inf for holes."""
    return np.where(bins >= 0, f.astype(rdt)[np.maximum(bins, 0)], rdt(np.inf)).astype(rdt)


def _cases(na, n, B):
    """-> [(name, rho, bins [B, na, n], {n_iter: closed-form rows or None})]: row maps g under the reversal (the bin of row
    k is na - 1 - g[k]), then seeded random bins under the reversal, a permutation and a many-to-one table."""
    k = np.arange(na)
    rev = na - 1 - k

    def full(col):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(col)[None, :, None], (B, na, n))).astype(np.int64)

    def under_rev(g):
        return full(np.where(np.asarray(g) >= 0, na - 1 - np.asarray(g), -1))
    shift = np.minimum(k + 1, na - 1)
    pair = k ^ 1
    pair[pair >= na] = na - 1                                     # an odd na leaves its last row on itself
    hole = shift.copy()
    hole[5] = -1
    hole_ans = np.where(k < 5, 4, np.minimum(k + 63, na - 1))     # rows below the hole stop on row 4, which points at it
    hole_ans[5] = -1
    rng = np.random.default_rng(na * 1000 + n)

    def rnd():
        b = rng.integers(0, na, size=(B, na, n))
        b[rng.random((B, na, n)) < 1 / 3] = -1
        return b
    perm = rng.permutation(na)
    many = np.minimum((k // 3) * 3 + 1, na - 1)[::-1].copy()      # three bins to a row, descending
    return [
        ("identity", rev, under_rev(k), {i: full(k) for i in (1, 2, 7, 64)}),
        ("none", rev, full(np.full(na, -1)), {i: full(np.full(na, -1)) for i in (1, 5, 64)}),
        ("shift", rev, under_rev(shift), {i: full(np.minimum(k + i - 1, na - 1)) for i in (1, 2, 7, 64)}),
        ("pairs", rev, under_rev(pair), {i: full(k if i % 2 else pair) for i in (1, 2, 7, 64)}),
        ("hole", rev, under_rev(hole), {1: full(np.where(hole >= 0, k, -1)), 64: full(hole_ans), 3: None}),
        ("random", rev, rnd(), {i: None for i in (1, 2, 5, 64)}),
        ("permutation", perm, rnd(), {i: None for i in (2, 5, 64)}),
        ("many-to-one", many, rnd(), {i: None for i in (2, 5, 64)}),
    ]


@DTYPES
@pytest.mark.parametrize("shape", range(5), ids=["9x1", "9x37-linear", "33xtiles+5x3-piecewise", "257xtile+7-piecewise",
                                                 "2049x20x2"])
def test_walk_kernel_follows_the_definition(shape, rdt):
    na, n, B, grid = walk_shapes()[shape]
    f = _freqs(grid, na)
    with np.errstate(divide="ignore", invalid="ignore"):
        _, kind, f_idx = up._freq_type(f, None, None, None)
    assert kind == grid
    for name, rho, bins, answers in _cases(na, n, B):
        w = _w_of(bins, f, rdt)
        b_model, _ = r.one_step_bins(w, f, kind, f_idx)
        assert np.array_equal(b_model, bins), ("the model's bins of the built w", name)
        for n_iter, closed in answers.items():
            ref = r.walk_rows(bins, rho, n_iter)
            if closed is not None:
                assert np.array_equal(ref, closed), ("the model itself", name, n_iter)
            rows, got_bins, w_n = up.mssq_cwt_walk(w, f, rho, n_iter)
            assert rows.dtype == got_bins.dtype == np.int32 and w_n.dtype == rdt and rows.shape == w_n.shape == w.shape
            assert np.array_equal(got_bins, bins), (name, n_iter, int((got_bins != bins).sum()))
            assert np.array_equal(rows, ref), (name, n_iter, int((rows != ref).sum()))
            assert np.array_equal(w_n, r.gather(w, ref)), (name, n_iter)
    name, rho, bins, _ = _cases(na, n, B)[5]
    w2d = _w_of(bins[0], f, rdt)                                                  # a 2-D map
    rows, got_bins, w_n = up.mssq_cwt_walk(w2d, f, rho, 5)
    assert np.array_equal(rows, r.walk_rows(bins[0], rho, 5)) and np.array_equal(got_bins, bins[0])


def test_walk_puts_nan_in_bin_zero():
    """NaN is kept and lands in bin 0, as `ssqueeze` has it; rho[0] is then its row."""
    na, n = 9, 3
    f = _freqs("log", na)
    w = np.full((na, n), np.inf)
    w[2, 1] = np.nan
    w[4, 1] = f[3]
    rho = na - 1 - np.arange(na)                                  # bin 0 -> row 8 (no map): the NaN row stays; bin 3 -> row 5
    rows, bins, w_n = up.mssq_cwt_walk(w, f, rho, 3)
    assert bins[2, 1] == 0 and bins[4, 1] == 3 and (np.delete(bins.ravel(), [2 * n + 1, 4 * n + 1]) == -1).all()
    assert rows[2, 1] == 2 and rows[4, 1] == 4 and np.isnan(w_n[2, 1]) and w_n[4, 1] == f[3]
    rho[0] = 4                                                    # bin 0 -> row 4, which maps: the NaN row moves there
    rows, bins, w_n = up.mssq_cwt_walk(w, f, rho, 2)
    assert rows[2, 1] == 4 and w_n[2, 1] == f[3]


def test_walk_past_the_grid_dimension_limit():
    """65537 signals go in two launches (grid.y holds 65535): the last two are walked like the first."""
    B, na, n = 65537, 3, 2
    f = _freqs("log", na)
    rng = np.random.default_rng(7)
    bins = rng.integers(-1, na, size=(B, na, n))
    rho = np.array([1, 2, 0])
    w = _w_of(bins, f, np.float32)
    rows, got_bins, w_n = up.mssq_cwt_walk(w, f, rho, 5)
    ref = r.walk_rows(bins, rho, 5)
    assert np.array_equal(got_bins, bins) and np.array_equal(rows, ref) and np.array_equal(w_n, r.gather(w, ref))
    assert (ref[65535:] != np.arange(na)[:, None]).any()                         # (the tail does move)


# ------------------------------------------------------------------------------------------------------ the transform
def _call(i, rdt, order, n_iter, **more):
    N, sc, wavelet, pad, kw = CASES[i]
    return up.mssq_cwt(c2.two_chirps(N, i).astype(rdt), wavelet, scales=sc(), fs=FS, padtype=pad, order=order, n_iter=n_iter,
                       **{**kw, **more})


@functools.lru_cache(maxsize=None)
def gpu(i, rdt, order=2, n_iter=N_ITER):
    out = _call(i, rdt, order, n_iter, get_w=True, get_rows=True, get_bins=True)
    for a in out:
        a.setflags(write=False)
    return out


def rho_of(i):
    N, sc, wavelet, pad, kw = CASES[i]
    s, rc, f, kind, f_idx = c2.grids(i)
    rho = up.mssq_cwt_row_of_bin(wavelet, s, f, FS)
    mw = (wavelet[0], *up._wavelet(wavelet)[1:])
    assert np.array_equal(rho, r.row_of_bin(r.row_freqs(mw, s) * FS, f))
    return rho


def tie_margin(w, f, kind, f_idx, rdt):
    """How far from a half-integer the rounded position must lie for the bin to be decided.  The kernel forms, in the
    call's dtype with eps = its machine epsilon, v = (L(w) - v0) / dv with L = log2 (identity on 'linear' grids) and v0, dv
    rounded from float64.  Errors: L(w) by at most 2 ulp (2 eps |L|), v0 by eps/2 |v0|, the difference by eps/2 (|L| + |v0|),
    the quotient and dv's rounding by eps |v| together: |dv| in all <= eps ((2.5 |L| + |v0|) / dv + |v|).  The margin is
    4 eps ((|L| + |v0|) / dv + |v|) with the larger |v0| and the smaller dv of the two segments on 'log-piecewise' grids."""
    eps = float(np.finfo(rdt).eps)
    w = w.astype(np.float64)
    with np.errstate(all="ignore"):
        if kind == "linear":
            L, v0, dv = np.abs(w), abs(f[0]), f[1] - f[0]
        else:
            L, v0, dv = np.abs(np.log2(w)), abs(np.log2(f[0])), np.log2(f[1]) - np.log2(f[0])
            if kind == "log-piecewise":
                v0 = max(v0, abs(np.log2(f[f_idx - 1])))
                dv = min(dv, np.log2(f[f_idx]) - np.log2(f[f_idx - 1]))
        _, v = r.one_step_bins(w, f, kind, f_idx)
        return 4 * eps * ((L + v0) / dv + np.abs(v)), v


@DTYPES
@EACH
def test_one_step_of_order_two_is_ssq_cwt2(i, rdt):
    Tx, Wx, f, sc, w, rows, bins = gpu(i, rdt, 2, 1)
    Tx2, Wx2, f2, sc2, w2 = c2.gpu(i, rdt)
    assert Tx.dtype == Tx2.dtype and w.dtype == w2.dtype and rows.dtype == bins.dtype == np.int32
    assert np.array_equal(Tx.view(rdt), Tx2.view(rdt)) and np.array_equal(Wx.view(rdt), Wx2.view(rdt))
    assert np.array_equal(w, w2) and np.array_equal(f, f2) and np.array_equal(sc, sc2)
    na = len(sc)
    assert np.array_equal(rows, np.where(np.isinf(w), -1, np.arange(na)[:, None]))
    N, scf, wavelet, pad, kw = CASES[i]                                          # the launch is skipped: the same bits
    plain = up.mssq_cwt(c2.two_chirps(N, i).astype(rdt), wavelet, scales=scf(), fs=FS, padtype=pad, n_iter=1, **kw)
    assert len(plain) == 4 and np.array_equal(plain[0].view(rdt), Tx2.view(rdt))


@ORDERS
@DTYPES
@EACH
def test_rows_are_the_walk_of_the_calls_own_bins(i, rdt, order):
    N = CASES[i][0]
    s, rc, f, kind, f_idx = c2.grids(i)
    Tx, Wx, fr, sc, w, rows, bins = gpu(i, rdt, order)
    assert Tx.shape == Wx.shape == w.shape == rows.shape == bins.shape == (len(s), N)
    assert Tx.dtype == Wx.dtype == (np.complex64 if rdt == np.float32 else np.complex128)
    assert w.dtype == fr.dtype == sc.dtype == rdt and np.array_equal(fr, f[::-1].astype(rdt))
    assert np.array_equal(np.isinf(w), bins == -1) and bins.max() < len(s)
    ref = r.walk_rows(bins, rho_of(i), N_ITER)
    print("%d of %d kept coefficients left their row" % ((ref != np.arange(len(s))[:, None])[bins >= 0].sum(), (bins >= 0).sum()))
    assert np.array_equal(rows, ref)


@ORDERS
@DTYPES
@EACH
def test_bins_follow_the_rule_on_the_calls_own_w(i, rdt, order):
    """Away from rounding ties (`tie_margin`) the kernel's one-step bins are the model's rule on the reported w; at most 1 %
    of the kept elements may lie that near a tie."""
    s, rc, f, kind, f_idx = c2.grids(i)
    w, bins = gpu(i, rdt, order)[4], gpu(i, rdt, order)[6]
    kept = ~np.isinf(w)
    ref, _ = r.one_step_bins(w.astype(np.float64), f, kind, f_idx)
    margin, v = tie_margin(w, f, kind, f_idx, rdt)
    with np.errstate(invalid="ignore"):
        near = kept & ~(np.abs(v - np.floor(v) - 0.5) > margin)                   # (NaN positions count as near)
    share = near.sum() / max(kept.sum(), 1)
    print("%d of %d kept elements near a tie (%.3g), %d of them differ; largest margin %.3g"
          % (near.sum(), kept.sum(), share, (bins != ref)[near].sum(), np.nanmax(np.where(kept, margin, 0))))
    assert np.array_equal(bins[~near], ref[~near])
    assert share <= 0.01


@ORDERS
@DTYPES
@EACH
def test_tx_is_ssqueeze_of_the_gathered_w(i, rdt, order):
    N, sc, wavelet, pad, kw = CASES[i]
    Tx, Wx, _, _, w, rows, bins = gpu(i, rdt, order)
    w_n = r.gather(w, rows)
    assert w_n.dtype == w.dtype
    ref, _ = up.ssqueeze(Wx, w_n, scales=sc(), wavelet=wavelet, maprange=kw.get("maprange", "peak"), ssq_freqs=None,
                         squeezing=kw.get("squeezing", "sum"), flipud=kw.get("flipud", True), fs=FS)
    assert ref.dtype == Tx.dtype and np.array_equal(Tx, ref)
    if order == 2:
        assert not np.array_equal(Tx, c2.gpu(i, rdt)[0])                         # (the walk moved something)


@EACH
def test_order_one_reports_the_first_order_frequency(i):
    W, _, _, _, d = c2.model(i)
    dd = c2.model(i, "dft")[4]
    big = c2.strong(W)
    tol = 10 * np.abs(d["w1"] - dd["w1"])[big].max()
    w = gpu(i, np.float64, 1)[4]
    ew = np.abs(w - d["w1"])[big].max()
    print("w err %.3g (tol %.3g, %d strong bins)" % (ew, tol, big.sum()))
    assert np.array_equal(np.isinf(w), np.isinf(c2.model(i)[1]))
    assert ew <= tol
    assert not np.array_equal(w, gpu(i, np.float64, 2)[4])                       # (the two orders are different maps)


@DTYPES
def test_batch_equals_single_calls_and_is_deterministic(rdt):
    X = np.stack([c2.two_chirps(300, sd) for sd in (11, 12, 13)]).astype(rdt)
    kw = dict(scales=c2._log(c2.GMW, 37, 8), fs=FS, n_iter=N_ITER, get_w=True, get_rows=True, get_bins=True)
    B = up.mssq_cwt(X, c2.GMW, **kw)
    assert B[0].shape == B[4].shape == B[5].shape == B[6].shape == (3, 37, 300)
    for b in range(3):
        one = up.mssq_cwt(X[b], c2.GMW, **kw)
        for k in (0, 1, 4, 5, 6):
            assert np.array_equal(B[k][b], one[k], equal_nan=True), (b, k)
    again = up.mssq_cwt(X, c2.GMW, **kw)
    for k in (0, 1, 4, 5, 6):
        assert np.array_equal(B[k], again[k], equal_nan=True), k


@DTYPES
@pytest.mark.parametrize("i", [0, 3], ids=[IDS[0], IDS[3]])
def test_flipud_mirrors_tx_and_nothing_else(i, rdt):
    up_ = _call(i, rdt, 2, N_ITER, flipud=True, get_w=True, get_rows=True, get_bins=True)
    dn = _call(i, rdt, 2, N_ITER, flipud=False, get_w=True, get_rows=True, get_bins=True)
    assert np.array_equal(up_[0][::-1], dn[0]) and np.array_equal(up_[2], dn[2])      # (ssq_freqs are returned descending)
    for k in (1, 3, 4, 5, 6):
        assert np.array_equal(up_[k], dn[k]), k


@pytest.mark.parametrize("grid", ["peak", "maximal"])
def test_concentrates_an_fm_signal_as_the_model_says(grid):
    """The sinusoidal FM of DESIGN 4.20's table at order 2, n_iter 4: the top-cell share at the model's digits (0.9980 on
    the 'peak' grid, 0.9970 on the 'maximal' one), above `ssq_cwt2`'s."""
    x, scales, f_asc, rc = r.fm_case(grid)
    s_model = r.top_cell_share(r.mssq_cwt_ref(x, r.FM_WAVELET, scales, f_asc, "log", None, rc, order=2, n_iter=4)[5])
    kw = dict(scales=scales, ssq_freqs=f_asc, flipud=False)
    Tx = up.mssq_cwt(x, c2.GMW, order=2, n_iter=4, **kw)[0]
    s4, s1 = r.top_cell_share(Tx), r.top_cell_share(up.ssq_cwt2(x, c2.GMW, **kw)[0])
    print("top-cell share: n_iter 4 %.6f (model %.6f), ssq_cwt2 %.6f" % (s4, s_model, s1))
    assert "%.4f" % s4 == "%.4f" % s_model
    assert s4 > s1


def test_inverts_like_the_second_order_transform():
    N = 300
    x = c2.two_chirps(N, 5)
    kw = dict(scales=c2._log(c2.GMW, 37, 8))
    Txm = up.mssq_cwt(x, c2.GMW, n_iter=N_ITER, **kw)[0]
    Tx2 = up.ssq_cwt2(x, c2.GMW, **kw)[0]
    xm, x2 = up.issq_cwt(Txm, c2.GMW), up.issq_cwt(Tx2, c2.GMW)
    print("inverse difference %.3g of max|x|" % (np.abs(xm - x2).max() / np.abs(x).max()))
    assert not np.array_equal(Txm, Tx2)
    assert np.abs(xm - x2).max() <= 1e-9 * np.abs(x).max()


@DTYPES
def test_degenerate_inputs(rdt):
    sc = c2._log(c2.GMW, 20, 4)
    na = len(sc)
    kw = dict(scales=sc, n_iter=N_ITER, get_w=True, get_rows=True, get_bins=True)
    Tx, Wx, _, _, w, rows, bins = up.mssq_cwt(np.zeros(200, dtype=rdt), c2.GMW, **kw)
    assert not Tx.any() and not Wx.any() and np.isinf(w).all() and (rows == -1).all() and (bins == -1).all()
    x = c2.two_chirps(200, 3).astype(rdt)
    Tx, Wx, _, _, w, rows, bins = up.mssq_cwt(x, c2.GMW, gamma=1e6, **kw)
    assert np.abs(Wx).max() < 1e6 and not Tx.any() and np.isinf(w).all() and (rows == -1).all() and (bins == -1).all()
    f_asc = 0.5 * 2.0 ** ((np.arange(na) - (na - 1)) / 4)       # (given: the 'peak' frequencies of a 4-point grid coincide)
    rho = up.mssq_cwt_row_of_bin(c2.GMW, sc, f_asc)
    for xs in (np.full(200, 3.0, dtype=rdt), np.array([1.0, -1.0], dtype=rdt)):    # a constant; N = 2
        for order in (1, 2):
            Tx, Wx, f, _, w, rows, bins = up.mssq_cwt(xs, c2.GMW, order=order, ssq_freqs=f_asc, **kw)
            assert Tx.shape == rows.shape == (na, len(xs)) and np.isfinite(Tx.view(rdt)).all()
            assert np.array_equal(f, f_asc[::-1].astype(rdt))
            assert np.array_equal(np.isinf(w), bins == -1) and np.array_equal(rows == -1, bins == -1)
            assert bins.max() < na and rows.max() < na
            assert np.array_equal(rows, r.walk_rows(bins, rho, N_ITER))
            ref, _ = up.ssqueeze(Wx, r.gather(w, rows), scales=sc, ssq_freqs=f_asc, flipud=True)
            assert np.array_equal(Tx, ref, equal_nan=True)
