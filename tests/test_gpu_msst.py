"""GPU tests of the multisynchrosqueezed STFT, `upstream.mssq_stft` and `upstream.msst_walk` (csrc/stft_msst.hip, DESIGN
4.17), against the numpy model tests/helpers/msst_ref.py.

The walk is integer work: it is compared with `np.array_equal`, on maps built by hand (through `msst_walk`, the same
kernel) and on the transform's own one-step map, recomputed from the `w` the call reports by the upstream rule in the
call's dtype.  The scatter is held to the bound of test_gpu_sst2.py, 4 eps dw sum|Sx| per column.  Frequencies of
order 1 may differ from the model by 10 x the difference between the model's FFT and DFT-matrix arithmetics, on the
bins with |V| >= 1e-2 max|V| and with the model on the library's own window tables, as test_gpu_sst2.py does it."""
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import upstream as up
from tests.helpers import msst_ref as r
from tests.helpers import sst2_ref as m2
from tests.test_gpu_sst2 import lib_tables, strong, two_chirps, window

pytestmark = pytest.mark.gpu

FS = 2.0
N_ITER = 4
# the cases of test_gpu_sst2.py: (N, n_fft, hop, padtype, extra keywords)
CASES = [
    (300, 16, 3, "zero", dict(flipud=True)),
    (600, 64, 1, "reflect", dict()),
    (1024, 256, 4, "reflect", dict(squeezing="lebesgue")),
    (5000, 1024, 7, "symmetric", dict(modulated=False)),
    (9000, 2048, 64, "wrap", dict()),
    (9000, 4096, 128, "replicate", dict()),
    (40, 64, 1, "zero", dict()),
]
IDS = ["%d-%d-%d-%s" % c[:4] for c in CASES]
DTYPES = pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])


# ---------------------------------------------------------------------------------------------- the walk kernel alone
def walk_shapes():
    """(F, n, B): the smallest F and a single column; a tile tail; several tiles with a batch; the largest F."""
    return [(9, 1, 1), (9, 37, 1), (33, 3 * up.msst_tile_cols(33) + 5, 3), (2049, 20, 2)]


def _maps(F, n, B):
    """name -> (map [B, F, n] int32, {n_iter: closed-form answer or None})."""
    k = np.arange(F, dtype=np.int32)

    def full(col):
        return np.ascontiguousarray(np.broadcast_to(col[None, :, None], (B, F, n))).astype(np.int32)
    shift = np.minimum(k + 1, F - 1)
    pair = k ^ 1
    pair[pair >= F] = F - 1                                   # an odd F leaves its last row on itself
    hole = shift.copy()
    hole[5] = -1
    hole_ans = np.where(k < 5, 5, np.minimum(k + 64, F - 1)).astype(np.int32)
    hole_ans[5] = -1
    rng = np.random.default_rng(F * 1000 + n)
    rnd = rng.integers(0, F, size=(B, F, n)).astype(np.int32)
    rnd[rng.random((B, F, n)) < 1 / 3] = -1
    near = np.clip(k[None, :, None] + rng.integers(-3, 4, size=(B, F, n)), 0, F - 1).astype(np.int32)   # short hops, as a ridge
    near[rng.random((B, F, n)) < 1 / 3] = -1
    return {
        "identity": (full(k), {i: full(k) for i in (1, 2, 7, 64)}),
        "none": (full(np.full(F, -1, np.int32)), {i: full(np.full(F, -1, np.int32)) for i in (1, 5, 64)}),
        "shift": (full(shift), {i: full(np.minimum(k + i, F - 1)) for i in (1, 2, 7, 64)}),
        "pairs": (full(pair), {i: full(pair if i % 2 else k) for i in (1, 2, 7, 64)}),
        "hole": (full(hole), {1: full(hole), 64: full(hole_ans), 3: None}),
        "random": (rnd, {i: None for i in (1, 2, 5, 64)}),
        "near": (near, {i: None for i in (2, 16)}),
    }


@pytest.mark.parametrize("shape", range(4), ids=["9x1", "9x37", "33xtiles+5x3", "2049x20x2"])
def test_walk_kernel_follows_the_definition(shape):
    F, n, B = walk_shapes()[shape]
    for name, (m, answers) in _maps(F, n, B).items():
        for n_iter, closed in answers.items():
            ref = r.walk(m, n_iter)
            if closed is not None:
                assert np.array_equal(ref, closed), ("the model itself", name, n_iter)
            got = up.msst_walk(m, n_iter)
            assert got.dtype == np.int32 and got.shape == m.shape
            assert np.array_equal(got, ref), (name, n_iter, int((got != ref).sum()))
    m2d = _maps(F, n, B)["random"][0][0]
    assert np.array_equal(up.msst_walk(m2d, 5), r.walk(m2d, 5))                  # a 2-D map


# ------------------------------------------------------------------------------------------------------ the transform
@functools.lru_cache(maxsize=None)
def gpu(i, rdt, order=2, n_iter=N_ITER):
    N, n, hop, pad, kw = CASES[i]
    out = up.mssq_stft(two_chirps(N, i).astype(rdt), window(n), n_fft=n, hop_len=hop, fs=FS, padtype=pad, order=order,
                       n_iter=n_iter, get_w=True, get_bins=True, **kw)
    for a in out:
        a.setflags(write=False)
    return out


def own_bins(w, F, flipud, rdt, n_iter, fs=FS):
    """The model's walk of the bins recomputed from the call's own w (upstream rule, the call's dtype), flip last."""
    m, dw = r.bins_of(w, F, fs, rdt)
    c = r.walk(m, n_iter)
    return (np.where(c >= 0, F - 1 - c, -1) if flipud else c), dw


@DTYPES
@pytest.mark.parametrize("i", [0, 3], ids=[IDS[0], IDS[3]])
def test_one_step_of_order_two_is_ssq_stft2(i, rdt):
    N, n, hop, pad, kw = CASES[i]
    x = two_chirps(N, i).astype(rdt)
    Tx, Sx, f, Sfs, w, bins = gpu(i, rdt, 2, 1)
    Tx2, Sx2, f2, Sfs2, w2 = up.ssq_stft2(x, window(n), n_fft=n, hop_len=hop, fs=FS, padtype=pad, get_w=True, **kw)
    assert Tx.dtype == Tx2.dtype and w.dtype == w2.dtype and bins.dtype == np.int32
    assert np.array_equal(Tx.view(rdt), Tx2.view(rdt)) and np.array_equal(Sx.view(rdt), Sx2.view(rdt))
    assert np.array_equal(w, w2) and np.array_equal(f, f2) and np.array_equal(Sfs, Sfs2)


@DTYPES
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_bins_are_the_walk_of_the_calls_own_map(i, rdt):
    N, n, hop, pad, kw = CASES[i]
    F = n // 2 + 1
    Tx, Sx, f, Sfs, w, bins = gpu(i, rdt)
    assert Tx.shape == Sx.shape == w.shape == bins.shape == (F, (N - 1) // hop + 1)
    assert Tx.dtype == Sx.dtype == (np.complex64 if rdt == np.float32 else np.complex128)
    assert w.dtype == Sfs.dtype == f.dtype == rdt and bins.dtype == np.int32
    Sfs_ref = np.linspace(0, .5 * FS, F, dtype=rdt)
    assert np.array_equal(Sfs, Sfs_ref) and np.array_equal(f, Sfs_ref[::-1] if kw.get("flipud") else Sfs_ref)
    assert np.array_equal(np.isinf(w), bins == -1)
    ref, _ = own_bins(w, F, kw.get("flipud", False), rdt, N_ITER)
    one, _ = own_bins(w, F, kw.get("flipud", False), rdt, 1)
    print("%d of %d kept coefficients moved past their one-step bin" % ((ref != one).sum(), (ref >= 0).sum()))
    assert np.array_equal(bins, ref)


@DTYPES
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_tx_is_the_scatter_of_the_calls_own_bins(i, rdt):
    """Tx == the rows-ascending scatter of the call's own Sx under the call's own bins, within 4 eps dw sum|Sx| per
    column (the bound of test_gpu_sst2.py::test_tx_is_the_scatter_of_the_calls_own_map)."""
    N, n, hop, pad, kw = CASES[i]
    F = n // 2 + 1
    Tx, Sx, _, _, w, bins = gpu(i, rdt)
    dw = rdt(np.linspace(0, .5 * FS, F)[1])
    ref = r.scatter(Sx, bins, dw, kw.get("squeezing", "sum"))
    tol = 4 * np.finfo(rdt).eps * float(dw) * np.abs(Sx).sum(0).astype(np.float64)
    err = np.abs(Tx.astype(np.complex128) - ref).max(0)
    print("worst column: %.3g of its tolerance" % (err / np.maximum(tol, 1e-300)).max())
    assert (err <= tol).all()


@pytest.mark.parametrize("i", [1, 3], ids=[IDS[1], IDS[3]])
def test_order_one_reports_the_first_order_frequency(i):
    N, n, hop, pad, kw = CASES[i]
    F = n // 2 + 1
    x, win = two_chirps(N, i), window(n)
    tabs = lib_tables(win)
    mk = dict(hop_len=hop, fs=FS, padtype=pad, order=1, n_iter=N_ITER, tables=tabs, **kw)
    V, wm, bm, _ = r.mssq_stft_ref(x, win, n, **mk)
    wd = r.mssq_stft_ref(x, win, n, arith="dft", **mk)[1]
    Tx, Sx, _, _, w, bins = gpu(i, np.float64, 1)
    big = strong(V)
    tol = 10 * np.abs(wm - wd)[big].max()
    ew = np.abs(w - wm)[big].max()
    print("w err %.3g (tol %.3g, %d strong bins)" % (ew, tol, big.sum()))
    assert np.array_equal(np.isinf(w), bm == -1)
    assert ew <= tol
    ref, _ = own_bins(w, F, kw.get("flipud", False), np.float64, N_ITER)
    assert np.array_equal(bins, ref)
    w2 = gpu(i, np.float64, 2)[4]
    assert not np.array_equal(w, w2)                                           # (the two orders are different maps)


@DTYPES
@pytest.mark.parametrize("N,n,hop", [(600, 64, 1), (3000, 1024, 7)])
def test_batch_equals_single_calls_and_is_deterministic(rdt, N, n, hop):
    X = np.stack([two_chirps(N, s) for s in (11, 12, 13)]).astype(rdt)
    win = window(n)
    kw = dict(n_fft=n, hop_len=hop, fs=FS, n_iter=N_ITER, get_w=True, get_bins=True)
    B = up.mssq_stft(X, win, **kw)
    assert B[0].shape == B[5].shape == (3, n // 2 + 1, (N - 1) // hop + 1)
    for b in range(3):
        one = up.mssq_stft(X[b], win, **kw)
        for k in (0, 1, 4, 5):
            assert np.array_equal(B[k][b], one[k]), (b, k)
    again = up.mssq_stft(X, win, **kw)
    for k in (0, 1, 4, 5):
        assert np.array_equal(B[k], again[k]), k


def test_concentrates_an_fm_signal_where_one_step_smears_it():
    """The sinusoidal FM of DESIGN 4.17 (N = 1024, n_fft = 256, Gaussian sigma = 24, hop 1): the share of each column's
    |Tx|^2 in the column's largest cell over columns n_fft .. N - n_fft.  Model: 0.958 at n_iter 4, 0.824 at 1."""
    N, n = 1024, 256
    x, _ = r.fm_signal(N)
    win = m2.gauss_window(n, 24)
    s_model = r.top_cell_share(r.mssq_stft_ref(x, win, n, order=2, n_iter=4)[3], n)
    s4 = r.top_cell_share(up.mssq_stft(x, win, n_fft=n, order=2, n_iter=4)[0], n)
    s1 = r.top_cell_share(up.ssq_stft2(x, win, n_fft=n)[0], n)
    print("top-cell share: n_iter 4 %.4f (model %.4f), ssq_stft2 %.4f" % (s4, s_model, s1))
    assert s4 >= s_model - 0.01
    assert s4 > s1


def test_inverts_like_the_second_order_transform():
    N, n = 600, 64
    x = two_chirps(N, 5)
    win = window(n)
    Txm = up.mssq_stft(x, win, n_fft=n, n_iter=N_ITER)[0]
    Tx2 = up.ssq_stft2(x, win, n_fft=n)[0]
    xm, x2 = up.issq_stft(Txm, win), up.issq_stft(Tx2, win)
    print("inverse difference %.3g, reconstruction error %.3g" % (np.abs(xm - x2).max(), np.abs(xm - x).max()))
    assert not np.array_equal(Txm, Tx2)
    assert np.abs(xm - x2).max() <= 1e-9 * np.abs(x).max()


@DTYPES
def test_degenerate_inputs(rdt):
    N, n = 500, 64
    F = n // 2 + 1
    win = window(n)
    kw = dict(n_fft=n, hop_len=3, n_iter=N_ITER, get_w=True, get_bins=True)
    eps = np.finfo(rdt).eps
    Tx, Sx, _, _, w, bins = up.mssq_stft(np.zeros(N, dtype=rdt), win, **kw)
    assert not Tx.any() and not Sx.any() and np.isinf(w).all() and (bins == -1).all()
    Tx, Sx, _, _, w, bins = up.mssq_stft(np.full(N, 3.0, dtype=rdt), win, **kw)
    assert np.isfinite(Tx.view(rdt)).all() and Tx.any()
    assert np.isinf(w[np.abs(Sx) < 5 * eps]).all() and np.isfinite(w[np.abs(Sx) > 20 * eps]).all()
    assert np.array_equal(bins, own_bins(w, F, False, rdt, N_ITER, fs=1.0)[0])
    assert np.array_equal(np.isinf(w), bins == -1) and bins.max() < F
    for order in (1, 2):                                                        # a one-sample signal: one column
        Tx, Sx, _, _, w, bins = up.mssq_stft(np.array([3.0], dtype=rdt), win, n_fft=n, order=order, n_iter=N_ITER, get_w=True,
                                             get_bins=True)
        assert Tx.shape == bins.shape == (F, 1) and np.isfinite(Tx.view(rdt)).all() and Tx.any()
        assert np.array_equal(np.isinf(w), bins == -1) and bins.max() < F
        dw = rdt(np.linspace(0, .5, F)[1])
        assert np.abs(Tx - r.scatter(Sx, bins, dw)).max() <= 4 * eps * float(dw) * np.abs(Sx).sum()
    x = two_chirps(N, 2).astype(rdt)
    Tx, Sx, _, _, w, bins = up.mssq_stft(x, win, gamma=1e6, **kw)
    assert np.abs(Sx).max() < 1e6 and not Tx.any() and np.isinf(w).all() and (bins == -1).all()
