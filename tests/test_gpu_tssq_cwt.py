"""GPU tests of the time-reassigned synchrosqueezed CWT, `upstream.tssq_cwt` (csrc/cwt_tsst.hip), against the
numpy model tests/helpers/tssq_cwt_ref.py, by the method of tests/test_gpu_reassign_cwt.py.

The model runs on the library's own fp64 wavelet tables (`ssq_ssq_cwt2_tables`).  Tolerances come from the model's
disagreement with itself, never from the kernel: fp64 `tau` may differ from the model by 10 x the difference between the
model's FFT and DFT-matrix arithmetics on the same input (the kernels are a third rounding order), float32 `tau` by that
bound plus one float32 ulp of the model ON THE FLOAT32-ROUNDED SIGNAL WITH FLOAT32'S GAMMA (the arithmetic is fp64 with
one rounding; the complex128 model is not the reference of a float32 call: the input rounding and the other gamma alone
move 3.9 % of the strong order-2 bins at N = 40).  Both are taken on the bins with |W| >= 1e-2 max|W|; so is the
comparison of targets, where a strong bin may land on either side only if, measured against that tolerance,
    its position tau / dt in the model is within the tolerance of a rounding boundary, or
    |d2| is within the tolerance of N, or |num| within the relative tolerance of gamma^2 (the order-2 choice may flip;
    the relative tolerance is 10 x the model's own disagreement on |num| relative to the larger of |num| and gamma^2),
and the share of strong bins so exempted is at most 1e-2 a case.

`Tx` is checked as the scatter of the call's OWN maps: the reference rotates the returned Wx under the returned targets at
`tssq_cwt_row_freqs` and sums in extended precision.  With q = A 2^tssq_cwt_quantum_log2(N), A the smallest power of two
>= sqrt(Pmax), Pmax the smallest power of two >= max|Wx|^2 of the returned Wx, a part (real or imaginary) T of a cell with
c contributions of mass M = sum(|Re Wx| + |Im Wx|) may be off by
    c q / 2                  every contribution's part is rounded to a multiple of q
  + 4 eps64 M                the rotation and the product in fp64: the angle in turns is exact up to one rounding of a
                             value <= 1/2 (2 pi 2^-55 < 0.2 eps64 in phase), sinpi and cospi are good to 2 ulp of a value
                             <= 1 (2 eps64), the two products and their sum round once each (1.5 eps64 of |a| + |b|):
                             below 3.7 eps64 (|a| + |b|) a contribution
  + eps_out |T|              the conversion of the cell's integer to fp64 (eps64 / 2) and the one rounding to the call's
                             dtype
which is derived from the definition, not from the kernel."""
import ctypes as C
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.helpers import cwt_sst2_ref as c2
from tests.helpers import tssq_cwt_ref as m
from tests.helpers.reassign_cwt_ref import time_targets
from tests.helpers.tsst_ref import impulses

pytestmark = pytest.mark.gpu

FS = 2.0
GMW, MORLET = ("gmw", {"gamma": 3.0, "beta": 60.0}), ("morlet", {"mu": 13.4})
S0 = {"gmw": c2.gmw_wc(3.0, 60.0) / np.pi, "morlet": 13.4 / np.pi}      # the scale whose peak sits at Nyquist
EPS64 = float(np.finfo(np.float64).eps)
LD = np.longdouble


def _log(wavelet, count, nv):
    return S0[wavelet[0]] * 2.0 ** (np.arange(count) / nv)


@functools.lru_cache(maxsize=None)
def _piecewise():
    return np.ascontiguousarray(up.process_scales("log-piecewise", 777, MORLET, nv=8), dtype=np.float64).reshape(-1)


# tests/test_gpu_reassign_cwt.py's five shapes: (N, scales, wavelet, padtype)
CASES = [
    (300, lambda: _log(GMW, 37, 8), GMW, "reflect"),
    (40, lambda: _log(MORLET, 20, 4), MORLET, "zero"),
    (1000, lambda: np.linspace(2, 60, 50), GMW, "symmetric"),
    (777, _piecewise, MORLET, "wrap"),
    (2500, lambda: _log(GMW, 12, 2), GMW, "replicate"),
]
IDS = ["300-log37-gmw-reflect", "40-log20-morlet-zero", "1000-linear50-gmw-symmetric", "777-piecewise-morlet-wrap",
       "2500-log12-gmw-replicate"]
RUNS = list(range(len(CASES)))
ORDERS = [1, 2]
RDTS = [np.float64, np.float32]
RDT_IDS = ["f64", "f32"]


def signal(N, seed=0):
    """tests/test_gpu_reassign_cwt.py's signal: two crossing chirps (0.1 -> 0.4 and 0.4 -> 0.1 cycles/sample, 1e-3 seeded
    noise) with an impulse of height 8 at 2N/5."""
    a, _ = c2.chirp(N, 0.1, 0.4)
    b, _ = c2.chirp(N, 0.4, 0.1)
    return a + b + 1e-3 * np.random.default_rng(seed).standard_normal(N) + impulses(N, [2 * N // 5], 8.0)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def model_wavelet(wavelet):
    return (wavelet[0], *up._wavelet(wavelet)[1:]) if wavelet[0] == "gmw" else (wavelet[0], up._wavelet(wavelet)[1])


@functools.lru_cache(maxsize=None)
def lib_tables(i):
    """(T0, T1) [na, P] of case i as the library evaluates them on the host (`ssq_ssq_cwt2_tables`)."""
    N, sc, wavelet, pad = CASES[i]
    scales, P = sc(), c2.p2up(N)[0]
    code, p0, p1 = up._wavelet(wavelet)
    T0, T1 = np.zeros((len(scales), P)), np.zeros((len(scales), P))
    for r, a in enumerate(scales):
        _lib.check(_lib.load().ssq_ssq_cwt2_tables(code, p0, p1, float(a), P, _vp(T0[r]), _vp(T1[r])))
    return T0, T1


@functools.lru_cache(maxsize=None)
def model(i, order, arith="fft", f32=False):
    """(W, tau, mm, details) of the model on case i, on the library's tables; f32: on the float32-rounded input, reported
    in float32 with float32's default gamma.  Computed once, read-only."""
    N, sc, wavelet, pad = CASES[i]
    x = signal(N, i)
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    W, tau, mm, _, d = m.tssq_cwt_ref(x, model_wavelet(wavelet), sc(), dt=1 / FS, padtype=pad, order=order, arith=arith,
                                      tabs=lib_tables(i), rdt=np.float32 if f32 else np.float64, squeeze=False,
                                      details=True)
    for a in (W, tau, mm):
        a.setflags(write=False)
    return W, tau, mm, d


@functools.lru_cache(maxsize=None)
def gpu(i, order, rdt):
    """(Tx, Wx, scales, row_freqs, tau, mm) of the library on case i; computed once, read-only."""
    N, sc, wavelet, pad = CASES[i]
    out = up.tssq_cwt(signal(N, i).astype(rdt), wavelet, scales=sc(), fs=FS, padtype=pad, order=order, get_tau=True,
                      get_targets=True)
    for a in out:
        a.setflags(write=False)
    return out


def strong(W):
    return np.abs(W) >= 1e-2 * np.abs(W).max()


def fp64_bounds(i, order, gamma=10 * EPS64):
    """(tau bound in seconds, relative bound on the comparison of |num| with gamma^2) on the strong bins: 10 x the model's
    'fft'-against-'dft' disagreement; that of |num| relative to the larger of |num| and gamma^2, the two sides of the
    comparison (a |num| that is all rounding noise but orders of magnitude above gamma^2 does not flip)."""
    W, taum, _, d = model(i, order)
    _, taud, _, dd = model(i, order, "dft")
    big = strong(W)
    tolt = 10 * np.abs(taum - taud)[big].max()
    if order == 1:
        return tolt, 0.0
    an, ad = np.abs(d["num"]), np.abs(dd["num"])
    return tolt, 10 * float((np.abs(an - ad) / np.maximum(an, gamma ** 2))[big].max())


def exemptions(i, order, f32, bound):
    """(tie, flip) of case i: the bins whose model position is within `bound` (seconds, scalar or per bin) of a rounding
    boundary, and those whose order-2 choice may flip (|d2| within the bound of N, |num| within the relative bound of
    gamma^2)."""
    N = CASES[i][0]
    W, taum, _, d = model(i, order, "fft", f32)
    gamma = 10 * float(np.finfo(np.float32 if f32 else np.float64).eps)
    with np.errstate(all="ignore"):
        v = taum.astype(np.float64) * FS
        tie = np.abs(v - np.floor(v) - 0.5) <= np.maximum(bound * FS, 1e-12)
        flip = np.zeros(W.shape, dtype=bool)
        if order == 2:
            flip = np.abs(np.abs(d["d2"]) - N) <= bound * FS
            flip |= np.abs(np.abs(d["num"]) - gamma ** 2) <= fp64_bounds(i, order, gamma)[1] * gamma ** 2
    return tie, flip


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("i", RUNS, ids=IDS)
def test_parity_float64(i, order):
    """Wx bitwise `ssq_cwt2`'s; tau and the targets against the model.  Measured on an MI355X: see DESIGN 4.16."""
    N, sc, wavelet, pad = CASES[i]
    W, taum, mmm, d = model(i, order)
    tolt, _ = fp64_bounds(i, order)
    Tx, Wx, scales, row_freqs, tau, mm = gpu(i, order, np.float64)
    assert Tx.shape == Wx.shape == tau.shape == mm.shape == W.shape == (len(sc()), N)
    assert Tx.dtype == Wx.dtype == np.complex128 and tau.dtype == scales.dtype == row_freqs.dtype == np.float64
    assert mm.dtype == np.int32
    assert np.array_equal(scales, sc()) and np.array_equal(row_freqs, up.tssq_cwt_row_freqs(wavelet, sc()) * FS)
    Wx2 = up.ssq_cwt2(signal(N, i), wavelet, scales=sc(), fs=FS, padtype=pad)[1]
    assert np.array_equal(Wx, Wx2)
    big = strong(W)
    tie, flip = exemptions(i, order, False, tolt)
    et = np.abs(tau - taum)[big & ~flip].max()
    nbad = int(((mm != mmm) & big & ~tie & ~flip).sum())
    share = ((tie | flip) & big).sum() / big.sum()
    print("Wx %.3g of max  tau err %.3g s (tol %.3g, ratio %.3g)  %d strong bins, targets differ %d (%d of them exempt), "
          "exempt share %.3g (ties %d, flips %d)" % (np.abs(Wx - W).max() / np.abs(W).max(), et, tolt, et / tolt, big.sum(),
                                                     ((mm != mmm) & big).sum(), ((mm != mmm) & big & (tie | flip)).sum(),
                                                     share, (tie & big).sum(), (flip & big).sum()))
    assert np.array_equal(np.isposinf(tau), np.isposinf(taum))
    assert et <= tolt
    assert nbad == 0
    assert share <= 1e-2


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("i", RUNS, ids=IDS)
def test_parity_float32(i, order):
    """float32 in, complex64 / float32 / int32 out; the kernels compute in fp64 and round once on store.  The reference is
    the model on the float32-rounded signal with float32's gamma.  Measured on an MI355X: see DESIGN 4.16."""
    Wf, tauf, mmf, d = model(i, order, "fft", True)
    tolt, _ = fp64_bounds(i, order)
    Tx, Wx, scales, row_freqs, tau, mm = gpu(i, order, np.float32)
    assert Tx.dtype == Wx.dtype == np.complex64 and tau.dtype == scales.dtype == row_freqs.dtype == np.float32
    assert mm.dtype == np.int32
    tolW = 10 * np.abs(Wf.astype(np.complex64) - Wf).max() / np.abs(Wf).max()
    eW = np.abs(Wx - Wf).max() / np.abs(Wf).max()
    big = strong(Wf)
    with np.errstate(all="ignore"):
        bt = tolt + np.spacing(np.abs(tauf)).astype(np.float64)
    tie, flip = exemptions(i, order, True, np.where(np.isfinite(bt), bt, tolt))
    ok = big & ~flip
    assert np.isfinite(tau[big]).all()
    et = np.abs(tau[ok].astype(np.float64) - tauf[ok].astype(np.float64))
    nbad = int(((mm != mmf) & big & ~tie & ~flip).sum())
    share = ((tie | flip) & big).sum() / big.sum()
    print("Wx %.3g of max (tol %.3g)  tau worst %.3g of (fp64 bound + 1 ulp)  %d strong bins, targets differ %d, exempt "
          "share %.3g (ties %d, flips %d)" % (eW, tolW, (et / bt[ok]).max(), big.sum(), ((mm != mmf) & big).sum(), share,
                                              (tie & big).sum(), (flip & big).sum()))
    assert eW <= tolW
    assert np.array_equal(np.isposinf(tau), np.isposinf(tauf))
    assert (et <= bt[ok]).all()
    assert nbad == 0
    assert share <= 1e-2


@pytest.mark.parametrize("rdt", RDTS, ids=RDT_IDS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("i", RUNS, ids=IDS)
def test_targets_follow_the_reported_tau(i, order, rdt):
    """mm is the time rule recomputed in the call's dtype from the returned tau, exactly; -1 exactly where tau is inf."""
    N = CASES[i][0]
    Tx, Wx, _, _, tau, mm = gpu(i, order, rdt)
    gone = np.isposinf(tau)
    assert not np.isneginf(tau).any()
    assert np.array_equal(mm == -1, gone)
    assert np.array_equal(mm[~gone], time_targets(tau, 1 / FS)[~gone])
    assert (mm[~gone] >= 0).all() and (mm[~gone] < N).all()


def quantum(Wx):
    """q of a returned Wx [na, N]: A 2^tssq_cwt_quantum_log2(N)."""
    mx = float((Wx.real.astype(np.float64) ** 2 + Wx.imag.astype(np.float64) ** 2).max())
    if mx == 0 or not np.isfinite(mx):
        return 0.0
    lp = int(np.ceil(np.log2(mx)))
    return 2.0 ** (-(-lp // 2) + up.tssq_cwt_quantum_log2(Wx.shape[-1]))


def scatter_check(Tx, Wx, mm, nu):
    """Tx against the extended-precision scatter of the call's own maps -> (worst part of a cell's error / its bound, the
    worst row of the marginal identity / the cell bounds summed over the row, every cell without a contribution exactly
    0)."""
    re, im, cnt, mass = m.scatter(Wx, mm, nu)
    eps_out = float(np.finfo(Tx.real.dtype).eps)
    base = cnt * quantum(Wx) / 2 + 4 * EPS64 * mass
    b_re = base + eps_out * np.abs(re).astype(np.float64)
    b_im = base + eps_out * np.abs(im).astype(np.float64)
    e_re = np.abs(Tx.real.astype(LD) - re).astype(np.float64)
    e_im = np.abs(Tx.imag.astype(LD) - im).astype(np.float64)
    worst = float(max((e_re / np.maximum(b_re, 1e-300)).max(), (e_im / np.maximum(b_im, 1e-300)).max()))
    a, b = m.marginal(Tx, nu, np.ones(Tx.shape, dtype=bool)), m.marginal(Wx, nu, mm >= 0)
    err = np.hypot((a[0] - b[0]).astype(np.float64), (a[1] - b[1]).astype(np.float64))
    row = float((err / np.maximum((b_re + b_im).sum(axis=1), 1e-300)).max())
    clean = bool((Tx[cnt == 0] == 0).all())
    return worst, row, clean


@pytest.mark.parametrize("rdt", RDTS, ids=RDT_IDS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("i", RUNS, ids=IDS)
def test_tx_is_the_scatter_of_the_calls_own_maps(i, order, rdt):
    """Every part of every cell within the derived bound of the module docstring, the marginal identity of every row within
    the cell bounds summed over the row, and a cell without a contribution exactly 0.  Measured on an MI355X: see DESIGN
    4.16."""
    N, sc, wavelet, pad = CASES[i]
    Tx, Wx, _, _, tau, mm = gpu(i, order, rdt)
    worst, row, clean = scatter_check(Tx, Wx, mm, up.tssq_cwt_row_freqs(wavelet, sc()))
    print("worst cell: %.3g of its bound; marginal identity, worst row: %.3g of the summed bound" % (worst, row))
    assert clean
    assert worst <= 1 and row <= 1
    assert (mm != np.arange(N)[None, :])[mm >= 0].any()                  # (something moved)


@pytest.mark.parametrize("rdt", RDTS, ids=RDT_IDS)
@pytest.mark.parametrize("order", ORDERS)
def test_batch_equals_single_calls_and_is_deterministic(order, rdt):
    X = np.stack([signal(300, sd) * a for sd, a in ((11, 1.0), (12, 300.0), (13, 1e-4))]).astype(rdt)   # three scales A
    kw = dict(scales=_log(GMW, 37, 8), fs=FS, order=order, get_tau=True, get_targets=True)
    B = up.tssq_cwt(X, GMW, **kw)
    assert B[0].shape == B[1].shape == B[4].shape == B[5].shape == (3, 37, 300)
    for b in range(3):
        one = up.tssq_cwt(X[b], GMW, **kw)
        for k in range(6):
            assert np.array_equal(B[k][b] if k not in (2, 3) else B[k], one[k]), (b, k)
    again = up.tssq_cwt(X, GMW, **kw)
    for k in range(6):
        assert np.array_equal(B[k], again[k]), k


@pytest.mark.parametrize("rdt", RDTS, ids=RDT_IDS)
@pytest.mark.parametrize("order", ORDERS)
def test_chunking_does_not_change_a_bit(order, rdt):
    """`work_limit_bytes` for 16 rows per chunk: the 2 x 37 rows go as 16 + 16 + 16 + 16 + 10, one chunk across the two
    signals, the last one partial; then one row per chunk."""
    lib = _lib.load()
    B, N, na = 2, 300, 37
    code = _lib.SSQ_F32 if rdt == np.float32 else _lib.SSQ_F64
    X = np.stack([signal(N, sd) for sd in (21, 22)]).astype(rdt)
    kw = dict(scales=_log(GMW, na, 8), fs=FS, order=order, get_tau=True, get_targets=True)
    mn = C.c_int64(0)
    assert lib.ssq_tssq_cwt_workspace_bytes(code, B, N, na, order, C.byref(mn)) > 0
    P, M = c2.p2up(N)[0], 2 if order == 1 else 5
    ref = up.tssq_cwt(X, GMW, **kw)
    for limit in (mn.value + 15 * 32 * M * P, mn.value):
        out = up.tssq_cwt(X, GMW, work_limit_bytes=limit, **kw)
        for k in range(6):
            assert np.array_equal(ref[k], out[k]), (limit, k)


@pytest.mark.parametrize("rdt", RDTS, ids=RDT_IDS)
@pytest.mark.parametrize("order", ORDERS)
def test_isolated_impulse(order, rdt):
    """padtype='zero', on the scales whose wavelet fits the padded length (tests/test_tssq_cwt_ref.py): every strong bin
    names the impulse's column, so that column holds the coherent sum of their rotated coefficients and nearly all of the
    energy."""
    from tests.test_tssq_cwt_ref import FIT, GMW as MW, N, SCALES, T0, column_share
    Tx, Wx, _, _, tau, mm = up.tssq_cwt(impulses(N, [T0]).astype(rdt), GMW, scales=SCALES[:FIT], padtype="zero", order=order,
                                        get_tau=True, get_targets=True)
    big = strong(Wx)
    assert big.sum() > 5000 and (mm[big] == T0).all()
    worst, row, clean = scatter_check(Tx, Wx, mm, up.tssq_cwt_row_freqs(GMW, SCALES[:FIT]))
    print("column %d: %.6f of the energy of Tx (%.6f of Wx); worst cell %.3g of its bound"
          % (T0, column_share(Tx, T0), column_share(Wx, T0), worst))
    assert worst <= 1 and row <= 1 and clean
    assert column_share(Tx, T0) > 0.99


def test_concentration_matches_the_model():
    """DESIGN 4.16's table: the GPU results reproduce its shares to four digits in fp64."""
    from tests.test_tssq_cwt_ref import SCALES, TABLE, table_shares

    def transform(x, wavelet, pad, order):
        w = GMW if wavelet[0] == "gmw" else MORLET
        return up.tssq_cwt(x, w, scales=SCALES, padtype=pad, order=order)[:2]
    got = table_shares(transform)
    for key, want in TABLE.items():
        print("%-32s GPU %.5f   table %.4f" % (key, got[key], want))
    for key, want in TABLE.items():
        assert abs(got[key] - want) <= 5e-5, key


@pytest.mark.parametrize("rdt", RDTS, ids=RDT_IDS)
def test_degenerate_inputs(rdt):
    sc = _log(GMW, 20, 4)
    nu = up.tssq_cwt_row_freqs(GMW, sc)
    kw = dict(scales=sc, get_tau=True, get_targets=True)
    Tx, Wx, _, _, tau, mm = up.tssq_cwt(np.zeros(200, dtype=rdt), GMW, **kw)
    assert not Tx.any() and not Wx.any() and np.isposinf(tau).all() and (mm == -1).all()
    Tx, Wx, _, _, tau, mm = up.tssq_cwt(np.full(200, 3.0, dtype=rdt), GMW, **kw)
    assert np.isfinite(Tx.view(rdt)).all() and not np.isnan(tau).any()
    worst, row, clean = scatter_check(Tx, Wx, mm, nu)
    assert worst <= 1 and row <= 1 and clean
    # N = 2, na = 2: P = 4, the two scales whose peaks sit on its bins 2 and 1
    sc2 = _log(GMW, 2, 1)
    Tx, Wx, _, _, tau, mm = up.tssq_cwt(np.array([3.0, -1.0], dtype=rdt), GMW, scales=sc2, padtype="zero", get_tau=True,
                                        get_targets=True)
    assert Tx.shape == (2, 2) and np.isfinite(Tx.view(rdt)).all() and Tx.any() and (mm >= 0).all()
    worst, row, clean = scatter_check(Tx, Wx, mm, up.tssq_cwt_row_freqs(GMW, sc2))
    assert worst <= 1 and row <= 1 and clean
    Tx, Wx, _, _, tau, mm = up.tssq_cwt(signal(200, 2).astype(rdt), GMW, gamma=1e6, **kw)
    assert np.abs(Wx).max() < 1e6 and not Tx.any() and np.isposinf(tau).all() and (mm == -1).all()
    # one infinite sample: every transform of the signal is NaN, nothing is defined to move, and Tx is all zero; the other
    # signal of the batch is what it is alone
    X = np.stack([signal(200, 4), signal(200, 5)]).astype(rdt)
    X[0, 77] = np.inf
    Tx, Wx, _, _, tau, mm = up.tssq_cwt(X, GMW, **kw)
    assert not Tx[0].any() and not np.isfinite(Wx[0].view(rdt)).any()
    one = up.tssq_cwt(X[1], GMW, **kw)
    assert np.array_equal(Tx[1], one[0]) and np.array_equal(mm[1], one[5])


@pytest.mark.parametrize("rdt", RDTS, ids=RDT_IDS)
def test_options(rdt):
    x = signal(300, 7).astype(rdt)
    kw = dict(scales=_log(GMW, 37, 8), fs=FS)
    full = up.tssq_cwt(x, GMW, get_tau=True, get_targets=True, **kw)
    bare = up.tssq_cwt(x, GMW, **kw)
    assert len(full) == 6 and len(bare) == 4 and np.array_equal(bare[0], full[0]) and np.array_equal(bare[1], full[1])
    only_mm = up.tssq_cwt(x, GMW, get_targets=True, **kw)
    assert len(only_mm) == 5 and np.array_equal(only_mm[4], full[5]) and np.array_equal(only_mm[0], full[0])
    first = up.tssq_cwt(x, GMW, order=1, get_targets=True, **kw)
    assert np.array_equal(first[1], full[1]) and not np.array_equal(first[4], full[5])
    t = np.arange(300) / FS
    timed = up.tssq_cwt(x, GMW, scales=kw["scales"], t=t, get_tau=True)
    assert np.array_equal(timed[0], full[0]) and np.array_equal(timed[4], full[4])
