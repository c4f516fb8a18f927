"""GPU tests of the reassigned spectrogram, `upstream.reassign_stft` (csrc/stft_reassign.hip), against the
numpy model tests/helpers/reassign_ref.py.

The model runs on the library's own fp64 window tables (`ssq_ssq_stft2_window_tables`).  Tolerances come from the
model's disagreement with itself, never from the kernel: fp64 `w` and `tau` may differ from the model by 10 x the
difference between the model's FFT and DFT-matrix arithmetics on the same input, fp32 ones by 10 x the difference
between the model in complex64 and in complex128.  Both are taken on the bins with |V| >= 1e-2 max|V|; so is the
comparison of targets.  Sx is held to the project's STFT tolerances (1e-11 / 2e-6 of max|Sx|).

`Rx` is checked as the scatter of the call's OWN maps: the reference adds the returned |Sx|^2 (squared and summed in
extended precision) under the targets recomputed from the returned `w` and `tau`.  With q = P 2^REASSIGN_QUANTUM_LOG2, P
the smallest power of two >= max|Sx|^2 of the returned Sx, a cell R with c contributions may be off by
    c q / 2                  every contribution is rounded to a multiple of q
  + (c + 2) eps64 R          the fp64 |Sx|^2 of every contribution, and the conversion of the cell's integer to fp64
  + eps_out R                the one rounding to the call's dtype
which is derived from the definition, not from the kernel."""
import ctypes as C
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.helpers import reassign_ref as m
from tests.helpers import sst2_ref as s2
from tests.helpers import tsst_ref as ts

pytestmark = pytest.mark.gpu

FS = 250.0
# (N, n_fft, hop, padtype, extra keywords): one lane per frame and the widest scatter tiles; a hop that does not divide
# n; modulated=False, H = 128 and about 30 scatter tiles; H = 512, a halo many times the tile of 31 frames (the largest
# reach tested); a hop that does not divide n at 1024; multi-wave frames; the narrowest tile (7 frames); a signal shorter
# than the window (every time target clamped)
CASES = [
    (1500, 16, 1, "reflect", dict()),
    (3000, 64, 3, "zero", dict()),
    (4000, 256, 1, "symmetric", dict(modulated=False)),
    (2500, 1024, 1, "reflect", dict()),
    (5000, 1024, 7, "wrap", dict()),
    (9000, 2048, 64, "replicate", dict()),
    (40000, 4096, 512, "reflect", dict()),
    (40, 64, 1, "zero", dict()),
]
RUNS = list(range(len(CASES)))
IDS = ["%d-%d-%d-%s" % c[:4] for c in CASES]
EPS64 = float(np.finfo(np.float64).eps)


def signal(N, seed=0):
    """tests/test_gpu_tsst.py's: two crossing chirps (0.1 -> 0.4 and 0.4 -> 0.1 cycles/sample), 1e-3 seeded noise and
    impulses of height 8 at N//5, N//2, N//2 + 9 and 4N//5."""
    a, _ = s2.chirp(N, 0.1, 0.4)
    b, _ = s2.chirp(N, 0.4, 0.1)
    x = a + b + 1e-3 * np.random.default_rng(seed).standard_normal(N)
    return x + ts.impulses(N, (N // 5, N // 2, N // 2 + 9, 4 * N // 5), 8.0)


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
def model(i, arith="fft", dtype=np.complex128):
    """(V, w, tau, kk, tgt) of the model on case i, on the window tables of the library; computed once, read-only."""
    N, n, hop, pad, kw = CASES[i]
    out = m.reassign_ref(signal(N, i), window(n), n, hop_len=hop, fs=FS, padtype=pad, arith=arith, dtype=dtype,
                         tables=lib_tables(n), squeeze=False, **kw)[:5]
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gpu(i, rdt):
    """(Rx, Sx, times, Sfs, w, tau) of the library on case i; computed once, read-only."""
    N, n, hop, pad, kw = CASES[i]
    out = up.reassign_stft(signal(N, i).astype(rdt), window(n), n_fft=n, hop_len=hop, fs=FS, padtype=pad, get_w=True,
                           get_tau=True, **kw)
    for a in out:
        a.setflags(write=False)
    return out


def strong(V):
    return np.abs(V) >= 1e-2 * np.abs(V).max()


def own_targets(w, tau, hop, fs=FS):
    """(keep, k', m') recomputed from a call's own maps by the rules in their dtype."""
    keep = ~np.isposinf(tau)
    return keep, m.bins(w, fs, w.shape[-2]), ts.targets(tau, hop, fs)[0]


def quantum(Sx):
    """q of a returned Sx: P 2^REASSIGN_QUANTUM_LOG2, P the smallest power of two >= max |Sx|^2."""
    mx = float(m.energy(Sx).max())
    return 0.0 if mx == 0 else 2.0 ** (int(np.ceil(np.log2(mx))) + up.REASSIGN_QUANTUM_LOG2)


def scatter_check(Rx, Sx, w, tau, hop, fs=FS):
    """Rx against the extended-precision scatter of the call's own maps -> (worst cell error / its bound, the error of
    the energy identity / the bound summed over the cells); asserts nothing."""
    keep, kk, tgt = own_targets(w, tau, hop, fs)
    ref, cnt = m.scatter(m.energy(Sx, np.longdouble), kk, tgt, keep, np.longdouble)
    R = ref.astype(np.float64)
    eps_out = float(np.finfo(Rx.dtype).eps)
    bound = cnt * quantum(Sx) / 2 + (cnt + 2) * EPS64 * R + eps_out * R
    err = np.abs(Rx.astype(np.longdouble) - ref).astype(np.float64)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    kept = m.energy(Sx, np.longdouble)[keep].sum()
    total = float(abs(Rx.astype(np.longdouble).sum() - kept)) / max(float(bound.sum()), 1e-300)
    return worst, total, bool((Rx[cnt == 0] == 0).all())


@pytest.mark.parametrize("i", RUNS, ids=IDS)
def test_parity_float64(i):
    """Sx, w, tau and the targets against the model.  Measured on an MI355X: see DESIGN 4.14."""
    N, n, hop, pad, kw = CASES[i]
    V, wm, taum, kkm, tgtm = model(i)
    _, wd, taud, _, _ = model(i, "dft")
    Rx, Sx, times, Sfs, w, tau = gpu(i, np.float64)
    nfr = (N - 1) // hop + 1
    assert Rx.shape == Sx.shape == w.shape == tau.shape == V.shape == (n // 2 + 1, nfr)
    assert Sx.dtype == np.complex128 and Rx.dtype == w.dtype == tau.dtype == times.dtype == Sfs.dtype == np.float64
    assert np.array_equal(times, np.arange(nfr) * hop / FS) and np.array_equal(Sfs, np.linspace(0, .5 * FS, n // 2 + 1))
    eS = np.abs(Sx - V).max() / np.abs(V).max()
    big = strong(V)
    tolw, tolt = 10 * np.abs(wm - wd)[big].max(), 10 * np.abs(taum - taud)[big].max()
    ew, et = np.abs(w - wm)[big].max(), np.abs(tau - taum)[big].max()
    keep, kk, tgt = own_targets(w, tau, hop)
    share = (((kk != kkm) | (tgt != tgtm)) & big).sum() / big.sum()
    print("Sx %.3g  w err %.3g Hz (tol %.3g)  tau err %.3g s (tol %.3g)  %d strong bins, targets differ share %.3g"
          % (eS, ew, tolw, et, tolt, big.sum(), share))
    assert eS <= 1e-11
    assert np.array_equal(np.isposinf(tau), kkm == -1) and np.array_equal(np.isposinf(w), kkm == -1)
    assert ew <= tolw and et <= tolt
    assert share <= 1e-3
    assert (Rx >= 0).all()


@pytest.mark.parametrize("i", RUNS, ids=IDS)
def test_parity_float32(i):
    """float32 in, complex64 / float32 out; the kernel computes in fp64 on the widened signal and rounds on store.
    Measured on an MI355X: see DESIGN 4.14."""
    N, n, hop, pad, kw = CASES[i]
    V, wm, taum, kkm, tgtm = model(i)
    _, ws, taus, _, _ = model(i, "fft", np.complex64)
    Rx, Sx, times, Sfs, w, tau = gpu(i, np.float32)
    assert Sx.dtype == np.complex64 and Rx.dtype == w.dtype == tau.dtype == times.dtype == Sfs.dtype == np.float32
    eS = np.abs(Sx - V).max() / np.abs(V).max()
    big = strong(V)
    tolw = 10 * np.abs(ws.astype(np.float64) - wm)[big].max()
    tolt = 10 * np.abs(taus.astype(np.float64) - taum)[big].max()
    ew, et = np.abs(w.astype(np.float64) - wm)[big].max(), np.abs(tau.astype(np.float64) - taum)[big].max()
    keep, kk, tgt = own_targets(w, tau, hop)
    share = (((kk != kkm) | (tgt != tgtm)) & big).sum() / big.sum()
    print("Sx %.3g  w err %.3g Hz (tol %.3g)  tau err %.3g s (tol %.3g)  %d strong bins, targets differ share %.3g"
          % (eS, ew, tolw, et, tolt, big.sum(), share))
    assert eS <= 2e-6
    kept32 = np.abs(V) > 10 * float(np.finfo(np.float32).eps)            # the model's rule at float32's default gamma
    assert np.array_equal(keep, kept32) and np.array_equal(np.isposinf(w), ~kept32)
    assert ew <= tolw and et <= tolt
    assert share <= 1e-3
    assert (Rx >= 0).all()


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("i", RUNS, ids=IDS)
def test_rx_is_the_scatter_of_the_calls_own_map(i, rdt):
    """Every cell within the derived bound of the module docstring, the energy identity within the bound summed over the
    cells, and a cell without a contribution exactly 0.  Measured on an MI355X: see DESIGN 4.14."""
    N, n, hop, pad, kw = CASES[i]
    Rx, Sx, _, _, w, tau = gpu(i, rdt)
    worst, total, clean = scatter_check(Rx, Sx, w, tau, hop)
    print("worst cell: %.3g of its bound; energy identity: %.3g of the summed bound" % (worst, total))
    assert clean
    assert worst <= 1 and total <= 1


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
def test_isolated_impulse(rdt):
    """Every kept bin of an impulse names the impulse's own column and its own row; the column holds |Sx|^2 summed over
    the frames, and every other cell is exactly 0."""
    N, n, t0 = 1000, 256, 333
    Rx, Sx, _, _, w, tau = up.reassign_stft(ts.impulses(N, [t0]).astype(rdt), window(n), n_fft=n, get_w=True, get_tau=True)
    keep, kk, tgt = own_targets(w, tau, 1, 1.0)
    assert keep.sum() >= 129 * 200 and (tgt[keep] == t0).all() and (kk[keep] == np.nonzero(keep)[0]).all()
    worst, total, clean = scatter_check(Rx, Sx, w, tau, 1, 1.0)
    col = np.where(keep, m.energy(Sx, np.longdouble), 0).sum(1)
    rel = float(np.abs(Rx[:, t0].astype(np.longdouble) - col).max() / col.max())
    print("column %d: worst cell %.3g of its bound, %.3g of the largest" % (t0, worst, rel))
    assert worst <= 1 and total <= 1 and clean
    assert not np.delete(Rx, t0, axis=1).any()


def test_concentration_matches_the_model():
    """DESIGN 4.14's table: the GPU result reproduces the model's shares to four digits."""
    from tests.test_reassign_ref import NFFT, SIGMA, TABLE, model_maps, table_shares
    win = s2.gauss_window(NFFT, SIGMA)
    got = table_shares(lambda x: up.reassign_stft(x, win, n_fft=NFFT)[:2])
    want = table_shares(model_maps)
    for (name, _, _, _, _), (gr, gs), (mr, ms) in zip(TABLE, got, want):
        print("%-8s reassigned: GPU %.5f, model %.5f   |Sx|^2: GPU %.5f, model %.5f" % (name, gr, mr, gs, ms))
        assert abs(gr - mr) <= 5e-5 and abs(gs - ms) <= 5e-5


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("i", [0, 3], ids=["1500-16-1", "2500-1024-1"])
def test_batch_equals_single_calls_and_is_deterministic(rdt, i):
    N, n, hop, pad, kw = CASES[i]
    X = np.stack([signal(N, s) * a for s, a in ((11, 1.0), (12, 3.0), (13, 0.01))]).astype(rdt)    # three scales P
    win = window(n)
    kw = dict(n_fft=n, hop_len=hop, fs=FS, padtype=pad, get_w=True, get_tau=True)
    B = up.reassign_stft(X, win, **kw)
    assert B[0].shape == (3, n // 2 + 1, (N - 1) // hop + 1)
    for b in range(3):
        one = up.reassign_stft(X[b], win, **kw)
        for k in (0, 1, 4, 5):
            assert np.array_equal(B[k][b], one[k]), (b, k)
    again = up.reassign_stft(X, win, **kw)
    for k in (0, 1, 4, 5):
        assert np.array_equal(B[k], again[k]), k


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
def test_degenerate_inputs(rdt):
    N, n = 500, 64
    win = window(n)
    kw = dict(n_fft=n, hop_len=3, get_w=True, get_tau=True)
    Rx, Sx, _, _, w, tau = up.reassign_stft(np.zeros(N, dtype=rdt), win, **kw)
    assert not Rx.any() and not Sx.any() and np.isposinf(w).all() and np.isposinf(tau).all()
    Rx, Sx, _, _, w, tau = up.reassign_stft(np.full(N, 3.0, dtype=rdt), win, **kw)
    assert np.isfinite(Rx).all() and Rx.any() and (Rx >= 0).all() and not np.isnan(w).any() and not np.isnan(tau).any()
    assert scatter_check(Rx, Sx, w, tau, 3, 1.0)[0] <= 1
    Rx, Sx, times, _, w, tau = up.reassign_stft(np.array([3.0, -1.0], dtype=rdt), win, n_fft=n, get_w=True, get_tau=True)
    assert Rx.shape == (n // 2 + 1, 2) and times.shape == (2,) and np.isfinite(Rx).all() and Rx.any()
    assert scatter_check(Rx, Sx, w, tau, 1, 1.0)[0] <= 1
    Rx, Sx, _, _, w, tau = up.reassign_stft(signal(N, 2).astype(rdt), win, gamma=1e6, **kw)
    assert np.abs(Sx).max() < 1e6 and not Rx.any() and np.isposinf(w).all() and np.isposinf(tau).all()
