"""GPU tests of the time-reassigned synchrosqueezed STFT, `upstream.tssq_stft` (csrc/stft_tsst.hip), against
the numpy model tests/helpers/tsst_ref.py.

The model runs on the library's own fp64 window tables (`ssq_ssq_stft2_window_tables`, held to numpy's by
tests/test_sst2_surface.py).  Tolerances come from the model's disagreement with itself, never from the kernel: fp64
offsets may differ from the model by 10 x the difference between the model's FFT and DFT-matrix arithmetics on the same
input, fp32 ones by 10 x the difference between the model in complex64 and in complex128.  Both are taken on the bins
with |V| >= 1e-2 max|V|; so is the comparison of target columns.  Sx is held to the project's STFT tolerances
(1e-11 / 2e-6 of max|Sx|).  The scatter check's reference sums the complex128 products in extended precision: an
ordered complex128 sum of the up to 2 H + 1 contributions of a cell would itself be off by about sqrt(H) eps of their
size, which is the bound under test (8 eps) at H = 2048."""
import ctypes as C
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.helpers import sst2_ref as s2
from tests.helpers import tsst_ref as m

pytestmark = pytest.mark.gpu

FS = 250.0
# (N, n_fft, hop, padtype, extra keywords): one lane per frame and 1024-frame operator tiles (a tile edge inside the
# signal); a hop that does not divide n; modulated=False; one full wave per frame; multi-wave frames, H = 16; a signal
# shorter than the window (every target clamped); H = 2048, the largest reach: two scatter tiles of 4096 targets whose
# halos cover half of each other (order 2 only)
CASES = [
    (1500, 16, 1, "reflect", dict()),
    (3000, 64, 3, "zero", dict()),
    (4000, 256, 1, "symmetric", dict(modulated=False)),
    (5000, 1024, 7, "wrap", dict()),
    (9000, 2048, 64, "replicate", dict()),
    (40, 64, 1, "zero", dict()),
    (6000, 4096, 1, "reflect", dict()),
]
RUNS = [(i, order) for i in range(len(CASES)) for order in (1, 2) if not (i == len(CASES) - 1 and order == 1)]
IDS = ["%d-%d-%d-%s-o%d" % (CASES[i][:4] + (order,)) for i, order in RUNS]


def two_chirps(N, seed=0):
    """Two crossing linear chirps (0.1 -> 0.4 and 0.4 -> 0.1 cycles/sample) plus 1e-3 seeded noise."""
    a, _ = s2.chirp(N, 0.1, 0.4)
    b, _ = s2.chirp(N, 0.4, 0.1)
    return a + b + 1e-3 * np.random.default_rng(seed).standard_normal(N)


def signal(N, seed=0):
    """The chirps plus impulses of height 8 at N//5, N//2, N//2 + 9 and 4N//5."""
    return two_chirps(N, seed) + m.impulses(N, (N // 5, N // 2, N // 2 + 9, 4 * N // 5), 8.0)


def window(n_fft):
    return s2.gauss_window(n_fft, n_fft / 10.0)


@functools.lru_cache(maxsize=None)
def lib_tables(n_fft):
    """(g, g1, g2, tg, tg1) as the library builds them on the host (`ssq_ssq_stft2_window_tables`)."""
    g = np.ascontiguousarray(window(n_fft), dtype=np.float64)
    t = [np.empty(len(g)) for _ in range(4)]
    _lib.check(_lib.load().ssq_ssq_stft2_window_tables(g.ctypes.data_as(C.c_void_p), len(g),
                                                       *[a.ctypes.data_as(C.c_void_p) for a in t]))
    return (g, *t)


@functools.lru_cache(maxsize=None)
def model(i, order, arith="fft", dtype=np.complex128):
    """(V, tau, tgt) of the model on case i, on the window tables of the library; computed once, read-only."""
    N, n, hop, pad, kw = CASES[i]
    out = m.tsst_ref(signal(N, i), window(n), n, hop_len=hop, fs=FS, padtype=pad, order=order, arith=arith, dtype=dtype,
                     tables=lib_tables(n), squeeze=False, **kw)[:3]
    for a in out:
        a.setflags(write=False)
    return out


def other_cols(i):
    """The frames on which the model's other arithmetics run, and on which tau is compared with a tolerance derived from
    them: all of them, but every 6th where the map has over 2M bins (6000-4096-1: the DFT-matrix product of all its
    frames alone would take 20 s).  Sx, the kept bins and the target columns are compared on every bin regardless."""
    N, n, hop, pad, kw = CASES[i]
    nfr = (N - 1) // hop + 1
    return np.arange(0, nfr, max(1, (n // 2 + 1) * nfr // 2_000_000))


@functools.lru_cache(maxsize=None)
def model_tau(i, order, arith, dtype):
    """tau alone, on `other_cols`, of another arithmetic of the model (what a tolerance is derived from)."""
    N, n, hop, pad, kw = CASES[i]
    return m.tsst_ref(signal(N, i), window(n), n, hop_len=hop, fs=FS, padtype=pad, order=order, arith=arith, dtype=dtype,
                      tables=lib_tables(n), squeeze=False, cols=other_cols(i), **kw)[1]


@functools.lru_cache(maxsize=None)
def gpu(i, order, rdt):
    N, n, hop, pad, kw = CASES[i]
    out = up.tssq_stft(signal(N, i).astype(rdt), window(n), n_fft=n, hop_len=hop, fs=FS, padtype=pad, order=order,
                       get_tau=True, **kw)
    for a in out:
        a.setflags(write=False)
    return out


def strong(V):
    return np.abs(V) >= 1e-2 * np.abs(V).max()


@pytest.mark.parametrize("i,order", RUNS, ids=IDS)
def test_parity_float64(i, order):
    """Sx, tau and the target columns against the model.  Measured on an MI355X: Sx <= 5.8e-16 of its maximum, the +inf
    pattern equal, no target differs, and the tau error on strong bins is 8e-17 ... 1.3e-10 s against bounds of 1.2e-15
    ... 5.7e-9 s: 0.02 ... 0.12 of the bound (closest: 40-64-1 order 2, 1.1e-15 against 9.4e-15; 1500-16-1 order 1, 8.0e-17
    against 1.2e-15)."""
    N, n, hop, pad, kw = CASES[i]
    V, taum, tgtm = model(i, order)
    taud = model_tau(i, order, "dft", np.complex128)
    Tx, Sx, times, Sfs, tau = gpu(i, order, np.float64)
    nfr = (N - 1) // hop + 1
    assert Tx.shape == Sx.shape == tau.shape == V.shape == (n // 2 + 1, nfr)
    assert Tx.dtype == Sx.dtype == np.complex128 and tau.dtype == times.dtype == Sfs.dtype == np.float64
    assert np.array_equal(times, np.arange(nfr) * hop / FS) and np.array_equal(Sfs, np.linspace(0, .5 * FS, n // 2 + 1))
    eS = np.abs(Sx - V).max() / np.abs(V).max()
    big = strong(V)
    c = other_cols(i)
    tol = 10 * np.abs(taum[:, c] - taud)[big[:, c]].max()
    et = np.abs(tau - taum)[:, c][big[:, c]].max()
    tgt, _ = m.targets(tau, hop, FS)
    _, vm = m.targets(taum, hop, FS)
    tie = np.abs(vm - np.floor(vm) - 0.5) < 1e-9
    nbad = int(((tgt != tgtm) & big & ~tie).sum())
    print("Sx %.3g  tau err %.3g s = %.3g samples (tol %.3g s, %d strong bins)  targets differ %d"
          % (eS, et, et * FS, tol, big.sum(), nbad))
    assert eS <= 1e-11
    assert np.array_equal(np.isinf(tau), tgtm == -1)
    assert et <= tol
    assert nbad == 0


@pytest.mark.parametrize("i,order", RUNS, ids=IDS)
def test_parity_float32(i, order):
    """float32 in, complex64 / float32 out; the kernel computes in fp64 on the widened signal and rounds on store.
    Measured on an MI355X: Sx <= 6.6e-8 of its maximum; tau error on strong bins 1.4e-8 ... 2.0e-2 s against bounds of
    2.3e-7 ... 0.39 s: 0.01 ... 0.15 of the bound (closest: 4000-256-1 order 2, 5.4e-5 against 3.7e-4); share of strong
    bins on another column than the complex128 model's 0 everywhere but 6000-4096-1 (6.7e-5; cap 1e-3) -- the rounding
    of the INPUT to float32: the model in fp64 on the float32-rounded input gives the same figures."""
    N, n, hop, pad, kw = CASES[i]
    V, taum, tgtm = model(i, order)
    taus = model_tau(i, order, "fft", np.complex64)
    Tx, Sx, times, Sfs, tau = gpu(i, order, np.float32)
    assert Tx.dtype == Sx.dtype == np.complex64 and tau.dtype == times.dtype == Sfs.dtype == np.float32
    eS = np.abs(Sx - V).max() / np.abs(V).max()
    big = strong(V)
    c = other_cols(i)
    tol = 10 * np.abs(taus.astype(np.float64) - taum[:, c])[big[:, c]].max()
    et = np.abs(tau.astype(np.float64) - taum)[:, c][big[:, c]].max()
    tgt, _ = m.targets(tau, hop, FS)
    share = ((tgt != tgtm) & big).sum() / big.sum()
    print("Sx %.3g  tau err %.3g s = %.3g samples (tol %.3g s, %d strong bins)  targets differ share %.3g"
          % (eS, et, et * FS, tol, big.sum(), share))
    assert eS <= 2e-6
    assert et <= tol
    assert share <= 1e-3


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("i,order", RUNS, ids=IDS)
def test_tx_is_the_scatter_of_the_calls_own_map(i, order, rdt):
    """Tx == the ascending-source scatter of the call's own Sx, with the rotation factor, under the targets recomputed
    from its own tau by the rule in the same dtype, within 8 eps sum|Sx| of every cell's contributions; and the marginal
    identity per row within 16 eps sum_m |Sx[k, m]|.  Measured on an MI355X: worst cell 0.41 ... 0.50 of its tolerance in
    fp64 (the two roundings of ONE complex product, the kernel's contracted and numpy's not: the figure is the same
    from H = 1 to H = 2048, the compensated sum adds nothing to it) and 0.06 in fp32 (the one rounding on store);
    marginal identity, worst row 0.15 (fp64) and 0.02 (fp32) of its tolerance."""
    N, n, hop, pad, kw = CASES[i]
    Tx, Sx, _, _, tau = gpu(i, order, rdt)
    keep = ~np.isposinf(tau)
    tgt, _ = m.targets(tau, hop, FS)
    ref = m.scatter(Sx, tgt, keep, hop, n, acc=np.longdouble)
    kk, mm = np.nonzero(keep)
    load = np.zeros(Sx.shape)
    np.add.at(load, (kk, tgt[kk, mm]), np.abs(Sx[kk, mm]).astype(np.float64))
    eps = float(np.finfo(rdt).eps)
    err = np.abs(Tx.astype(np.complex128) - ref)
    assert not Tx[load == 0].any()
    worst = (err / np.maximum(8 * eps * load, 1e-300)).max()
    k = np.arange(n // 2 + 1)[:, None]
    ph = np.exp(-2j * np.pi * ((k * np.arange(Sx.shape[1])[None, :] * hop) % n) / n)
    lhs = (Tx.astype(np.complex128) * ph).sum(1)
    rhs = (np.where(keep, Sx, 0).astype(np.complex128) * ph).sum(1)
    mtol = 16 * eps * np.abs(Sx).astype(np.float64).sum(1)
    mworst = (np.abs(lhs - rhs) / np.maximum(mtol, 1e-300)).max()
    print("worst cell: %.3g of its tolerance; marginal identity, worst row: %.3g of its tolerance" % (worst, mworst))
    assert (err <= 8 * eps * load).all()
    assert (np.abs(lhs - rhs) <= mtol).all()


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
def test_isolated_impulse(rdt, order):
    """Every kept bin of an impulse names the impulse's own column, and the column holds sum(g) in every row.  Measured
    on an MI355X: |Tx| / sum(g) - 1 is 0 in fp64 and 1.0e-8 in fp32, both orders."""
    N, n, t0 = 700, 128, 333
    win = window(n)
    Tx, Sx, _, _, tau = up.tssq_stft(m.impulses(N, [t0]).astype(rdt), win, n_fft=n, order=order, get_tau=True)
    keep = ~np.isposinf(tau)
    tgt, _ = m.targets(tau, 1, 1.0)
    assert keep.sum() >= 65 * 100 and (tgt[keep] == t0).all()
    rel = np.abs(np.abs(Tx[:, t0]) / win.sum() - 1).max()
    print("column %d: |Tx| / sum(g) - 1 <= %.3g" % (t0, rel))
    assert rel <= 1e-6
    assert not np.delete(Tx, t0, axis=1).any()


def test_concentration_matches_the_model():
    """The chirp and the four impulses of DESIGN 4.13's table (N = 1024, n_fft = 256, Gaussian sigma = 12, hop 1).
    Measured on an MI355X: the model's values to four digits (chirp 0.0128 / 1.0000, impulses 0.9288 / 0.8893)."""
    from tests.test_tsst_ref import IMPULSES, N, NFFT, SIGMA, chirp_share, impulse_share
    win = s2.gauss_window(NFFT, SIGMA)
    xc, _ = s2.chirp(N, 0.05, 0.45)
    xi = m.impulses(N, IMPULSES)
    for order in (1, 2):
        for name, x, share in (("chirp", xc, chirp_share), ("impulses", xi, impulse_share)):
            sm = share(np.abs(m.tsst_ref(x, win, NFFT, order=order)[3]) ** 2)
            sg = share(np.abs(up.tssq_stft(x, win, n_fft=NFFT, order=order)[0]) ** 2)
            print("%s, order %d: GPU %.4f, model %.4f" % (name, order, sg, sm))
            assert abs(sg - sm) <= 0.01


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("i", [0, 4], ids=["1500-16-1", "9000-2048-64"])
def test_batch_equals_single_calls_and_is_deterministic(rdt, i):
    N, n, hop, pad, kw = CASES[i]
    X = np.stack([signal(N, s) for s in (11, 12, 13, 14, 15)]).astype(rdt)
    win = window(n)
    for order in (1, 2):
        kw = dict(n_fft=n, hop_len=hop, fs=FS, padtype=pad, order=order, get_tau=True)
        B = up.tssq_stft(X, win, **kw)
        assert B[0].shape == (5, n // 2 + 1, (N - 1) // hop + 1)
        for b in range(5):
            one = up.tssq_stft(X[b], win, **kw)
            for k in (0, 1, 4):
                assert np.array_equal(B[k][b], one[k]), (order, b, k)
        again = up.tssq_stft(X, win, **kw)
        for k in (0, 1, 4):
            assert np.array_equal(B[k], again[k]), (order, k)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
def test_degenerate_inputs(rdt, order):
    N, n = 500, 64
    win = window(n)
    Tx, Sx, _, _, tau = up.tssq_stft(np.zeros(N, dtype=rdt), win, n_fft=n, hop_len=3, order=order, get_tau=True)
    assert not Tx.any() and not Sx.any() and np.isposinf(tau).all()
    Tx, Sx, _, _, tau = up.tssq_stft(np.full(N, 3.0, dtype=rdt), win, n_fft=n, hop_len=3, order=order, get_tau=True)
    assert np.isfinite(Tx.view(rdt)).all() and Tx.any()
    Tx, Sx, times, _, tau = up.tssq_stft(np.full(1, 3.0, dtype=rdt), win, n_fft=n, order=order, get_tau=True)
    assert Tx.shape == (n // 2 + 1, 1) and times.shape == (1,) and np.isfinite(Tx.view(rdt)).all()
    x = signal(N, 2).astype(rdt)
    Tx, Sx, _, _, tau = up.tssq_stft(x, win, n_fft=n, hop_len=3, order=order, gamma=1e6, get_tau=True)
    assert np.abs(Sx).max() < 1e6 and not Tx.any() and np.isposinf(tau).all()
