"""GPU tests of the second-order synchrosqueezed STFT, `upstream.ssq_stft2` (csrc/stft_sst2.hip), against
the numpy model tests/helpers/sst2_ref.py.

The model runs on the library's own fp64 window tables (`ssq_ssq_stft2_window_tables`, held to numpy's by
tests/test_sst2_surface.py).  Tolerances come from the model's disagreement with itself, never from the kernel: fp64
frequencies may differ from the model by 10 x the difference between the model's FFT and DFT-matrix arithmetics on the same input (the kernel is a
third rounding order: radix-16 passes, FMA contraction), fp32 ones by 10 x the difference between the model in
complex64 and in complex128.  Both are taken on the bins with |V| >= 1e-2 max|V|; so is the bin comparison, because on
weaker bins the operator is a quotient of two small numbers and the model's own arithmetics land in different bins.
Sx is held to the project's STFT tolerances (1e-11 / 2e-6 of max|Sx|)."""
import ctypes as C
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.helpers import sst2_ref as m

pytestmark = pytest.mark.gpu

FS = 2.0
# (N, n_fft, hop, padtype, extra keywords): L = 1; several frames per wave and a tail round; ...; one wave per frame;
# a frame across two waves; 4096; a pad wider than the signal
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


def two_chirps(N, seed=0):
    """Two crossing linear chirps (0.1 -> 0.4 and 0.4 -> 0.1 cycles/sample) plus 1e-3 seeded noise."""
    a, _ = m.chirp(N, 0.1, 0.4)
    b, _ = m.chirp(N, 0.4, 0.1)
    return a + b + 1e-3 * np.random.default_rng(seed).standard_normal(N)


def window(n_fft):
    return m.gauss_window(n_fft, n_fft / 10.0)


def lib_tables(win):
    """(g, g1, g2, tg, tg1) as the library builds them on the host (`ssq_ssq_stft2_window_tables`)."""
    g = np.ascontiguousarray(win, dtype=np.float64)
    t = [np.empty(len(g)) for _ in range(4)]
    _lib.check(_lib.load().ssq_ssq_stft2_window_tables(g.ctypes.data_as(C.c_void_p), len(g),
                                                       *[a.ctypes.data_as(C.c_void_p) for a in t]))
    return (g, *t)


@functools.lru_cache(maxsize=None)
def model(i, arith="fft", dtype=np.complex128):
    """The model on case i, on the window tables of the library (the definition's: `host_math.h::diff_window`)."""
    N, n, hop, pad, kw = CASES[i]
    out = m.sst2_ref(two_chirps(N, i), window(n), n, hop_len=hop, fs=FS, padtype=pad, arith=arith, dtype=dtype,
                     tables=lib_tables(window(n)), **kw)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gpu(i, rdt):
    N, n, hop, pad, kw = CASES[i]
    out = up.ssq_stft2(two_chirps(N, i).astype(rdt), window(n), n_fft=n, hop_len=hop, fs=FS, padtype=pad, get_w=True, **kw)
    for a in out:
        a.setflags(write=False)
    return out


def bins_of(w2, F, flipud, rdt):
    """The upstream rule on a frequency map, in the map's own dtype -> bins (meaningless where w2 is inf)."""
    Sfs = np.linspace(0, .5 * FS, F)
    dw = rdt(Sfs[1] - Sfs[0])
    with np.errstate(all="ignore"):
        v = np.maximum((w2 - rdt(Sfs[0])) / dw, rdt(0))
        kk = np.minimum(np.rint(v), F - 1)
    kk = np.where(np.isnan(kk), 0, kk).astype(np.int64)
    return (F - 1 - kk if flipud else kk), v, dw


def strong(V):
    return np.abs(V) >= 1e-2 * np.abs(V).max()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_parity_float64(i):
    """Sx, w2 and the bins against the model.  Measured on an MI355X: Sx <= 4e-16 of its maximum, no bin differs, and
    the w2 error on strong bins is 7e-15 ... 1.8e-10 against bounds of 6e-14 ... 5.5e-10 (closest: 5000-1024-7, 1.8e-10
    against 5.5e-10).  Against the model on numpy-built tables instead of the library's the error is 7.5e-8 there: g2,
    a second derivative by FFT, carries 1e-11 of rounding noise that differs between FFTs."""
    N, n, hop, pad, kw = CASES[i]
    F = n // 2 + 1
    V, w2m, kkm, Txm = model(i)
    w2d = model(i, "dft")[1]
    Tx, Sx, ssq_freqs, Sfs, w2 = gpu(i, np.float64)
    assert Tx.shape == Sx.shape == w2.shape == V.shape and Tx.dtype == Sx.dtype == np.complex128 and w2.dtype == np.float64
    Sfs_ref = np.linspace(0, .5 * FS, F)
    assert np.array_equal(Sfs, Sfs_ref) and np.array_equal(ssq_freqs, Sfs_ref[::-1] if kw.get("flipud") else Sfs_ref)
    eS = np.abs(Sx - V).max() / np.abs(V).max()
    big = strong(V)
    tol = 10 * np.abs(w2m - w2d)[big].max()
    ew = np.abs(w2 - w2m)[big].max()
    kk, _, _ = bins_of(w2, F, kw.get("flipud", False), np.float64)
    _, vm, _ = bins_of(w2m, F, False, np.float64)
    tie = np.abs(vm - np.floor(vm) - 0.5) < 1e-9
    nbad = int(((kk != kkm) & big & ~tie).sum())
    print("Sx %.3g  w2 err %.3g (tol %.3g, %d strong bins)  kk differ %d" % (eS, ew, tol, big.sum(), nbad))
    assert eS <= 1e-11
    assert np.array_equal(np.isinf(w2), kkm == -1)
    assert ew <= tol
    assert nbad == 0


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_parity_float32(i):
    """float32 in, complex64 / float32 out; the kernel computes in fp64 and rounds on store.  Measured on an MI355X: Sx
    <= 6e-8 of its maximum; w2 error on strong bins 1e-6 ... 1.1e-2 against bounds of 2.2e-5 ... 1.8e-1 (closest:
    9000-2048-64, 1.6e-3 against 4.6e-3); share of strong bins in another bin than the complex128 model's at most
    5.5e-4 (5000-1024-7; cap 1e-3) -- what is left is the rounding of the INPUT to float32.  With fp32 transforms the
    shares were 2.0e-3 and 1.5e-3 at n_fft 1024 and 4096 (the complex64 model itself: 1.1e-3 and 8e-4)."""
    N, n, hop, pad, kw = CASES[i]
    F = n // 2 + 1
    V, w2m, kkm, _ = model(i)
    w2s = model(i, "fft", np.complex64)[1]
    Tx, Sx, ssq_freqs, Sfs, w2 = gpu(i, np.float32)
    assert Tx.dtype == Sx.dtype == np.complex64 and w2.dtype == Sfs.dtype == ssq_freqs.dtype == np.float32
    eS = np.abs(Sx - V).max() / np.abs(V).max()
    big = strong(V)
    tol = 10 * np.abs(w2s.astype(np.float64) - w2m)[big].max()
    ew = np.abs(w2.astype(np.float64) - w2m)[big].max()
    kk, _, _ = bins_of(w2, F, kw.get("flipud", False), np.float32)
    share = ((kk != kkm) & big).sum() / big.sum()
    print("Sx %.3g  w2 err %.3g (tol %.3g, %d strong bins)  kk differ share %.3g" % (eS, ew, tol, big.sum(), share))
    assert eS <= 2e-6
    assert ew <= tol
    assert share <= 1e-3


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_tx_is_the_scatter_of_the_calls_own_map(i, rdt):
    """Tx == the rows-ascending scatter of the call's own Sx under the bins recomputed from its own w2 by the upstream
    rule in the same dtype, within 4 eps dw sum|Sx| per column."""
    N, n, hop, pad, kw = CASES[i]
    F = n // 2 + 1
    Tx, Sx, _, _, w2 = gpu(i, rdt)
    kk, _, dw = bins_of(w2, F, kw.get("flipud", False), rdt)
    keep = np.isfinite(w2)
    cdt = Tx.dtype.type
    add = np.full(Sx.shape, dw / rdt(F), dtype=cdt) if kw.get("squeezing") == "lebesgue" else (Sx * dw).astype(cdt)
    ref = np.zeros_like(Tx)
    cols = np.arange(Tx.shape[1])
    for r in range(F):
        k = keep[r]
        ref[kk[r, k], cols[k]] += add[r, k]
    tol = 4 * np.finfo(rdt).eps * float(dw) * np.abs(Sx).sum(0).astype(np.float64)
    err = np.abs(Tx.astype(np.complex128) - ref).max(0)
    print("worst column: %.3g of its tolerance" % (err / np.maximum(tol, 1e-300)).max())
    assert (err <= tol).all()


def test_concentrates_a_chirp_where_first_order_smears_it():
    """The chirp of DESIGN 4.11's table (0.05 -> 0.45 cycles/sample, N = 1024, n_fft = 256, Gaussian sigma = 24, hop 1):
    the share of |Tx|^2 on the chirp's own bin over columns n_fft .. N - n_fft."""
    N, n = 1024, 256
    x, fi = m.chirp(N, 0.05, 0.45)
    win = m.gauss_window(n, 24)
    c = np.arange(n, N - n)
    own = np.rint(fi / (0.5 / (n // 2))).astype(int)[c]

    def share(Tx):
        P = np.abs(Tx) ** 2
        return P[own, c].sum() / P[:, c].sum()
    s_model = share(m.sst2_ref(x, win, n)[3])
    s2 = share(up.ssq_stft2(x, win, n_fft=n)[0])
    s1 = share(up.ssq_stft(x, win, n_fft=n)[0])
    print("own-bin share: second order %.4f (model %.4f), first order %.4f" % (s2, s_model, s1))
    assert s_model > 0.95
    assert s2 >= s_model - 0.01
    assert s1 < 0.2


def test_inverts_like_the_first_order_transform():
    N, n = 600, 64
    x = two_chirps(N, 5)
    win = window(n)
    Tx2 = up.ssq_stft2(x, win, n_fft=n)[0]
    Tx1 = up.ssq_stft(x, win, n_fft=n)[0]
    x2, x1 = up.issq_stft(Tx2, win), up.issq_stft(Tx1, win)
    print("inverse difference %.3g, reconstruction error %.3g" % (np.abs(x2 - x1).max(), np.abs(x2 - x).max()))
    assert np.abs(x2 - x1).max() <= 1e-9 * np.abs(x).max()


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("N,n,hop", [(600, 64, 1), (3000, 1024, 7)])
def test_batch_equals_single_calls_and_is_deterministic(rdt, N, n, hop):
    X = np.stack([two_chirps(N, s) for s in (11, 12, 13)]).astype(rdt)
    win = window(n)
    kw = dict(n_fft=n, hop_len=hop, fs=FS, get_w=True)
    B = up.ssq_stft2(X, win, **kw)
    assert B[0].shape == (3, n // 2 + 1, (N - 1) // hop + 1)
    for b in range(3):
        one = up.ssq_stft2(X[b], win, **kw)
        for k in (0, 1, 4):
            assert np.array_equal(B[k][b], one[k]), (b, k)
    again = up.ssq_stft2(X, win, **kw)
    for k in (0, 1, 4):
        assert np.array_equal(B[k], again[k]), k


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
def test_degenerate_inputs(rdt):
    N, n = 500, 64
    win = window(n)
    Tx, Sx, _, _, w2 = up.ssq_stft2(np.zeros(N, dtype=rdt), win, n_fft=n, hop_len=3, get_w=True)
    assert not Tx.any() and not Sx.any() and np.isinf(w2).all()
    Tx, Sx, _, _, w2 = up.ssq_stft2(np.full(N, 3.0, dtype=rdt), win, n_fft=n, hop_len=3, get_w=True)
    assert np.isfinite(Tx.view(rdt)).all() and Tx.any()
    assert np.isinf(w2[np.abs(Sx) < 5 * np.finfo(rdt).eps]).all() and np.isfinite(w2[np.abs(Sx) > 20 * np.finfo(rdt).eps]).all()
    x = two_chirps(N, 2).astype(rdt)
    Tx, Sx, _, _, w2 = up.ssq_stft2(x, win, n_fft=n, hop_len=3, gamma=1e6, get_w=True)
    assert np.abs(Sx).max() < 1e6 and not Tx.any() and np.isinf(w2).all()
