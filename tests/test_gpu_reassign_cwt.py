"""GPU tests of the reassigned scalogram, `upstream.reassign_cwt` (csrc/cwt_reassign.hip), against the numpy
model tests/helpers/reassign_cwt_ref.py.

The model runs on the library's own fp64 wavelet tables (`ssq_ssq_cwt2_tables`).  Tolerances come from the model's
disagreement with itself, never from the kernel: fp64 `w` and `tau` may differ from the model by 10 x the difference
between the model's FFT and DFT-matrix arithmetics on the same input (the kernels are a third rounding order), float32
ones by that bound plus one float32 ulp of the model on the float32-rounded input (the arithmetic is fp64 with one
rounding).  Both are taken on the bins with |W| >= 1e-2 max|W|; so is the comparison of targets, where a bin whose
position in the model is within the allowed error of a rounding boundary may land on either side of it (their share is
bounded).

`Rx` is checked as the scatter of the call's OWN maps: the reference adds the returned |Wx|^2 (squared and summed in
extended precision) under the returned targets.  With q = Pmax 2^reassign_cwt_quantum_log2(na, N), Pmax the smallest
power of two >= max|Wx|^2 of the returned Wx, a cell R with c contributions may be off by
    c q / 2                  every contribution is rounded to a multiple of q
  + (c + 2) eps64 R          the fp64 |Wx|^2 of every contribution, and the conversion of the cell's integer to fp64
  + eps_out R                the one rounding to the call's dtype
which is derived from the definition, not from the kernel."""
import ctypes as C
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.helpers import cwt_sst2_ref as c2
from tests.helpers import reassign_cwt_ref as m
from tests.helpers import ssqueeze_ref as sq
from tests.helpers.tsst_ref import impulses

pytestmark = pytest.mark.gpu

FS = 2.0
GMW, MORLET = ("gmw", {"gamma": 3.0, "beta": 60.0}), ("morlet", {"mu": 13.4})
S0 = {"gmw": c2.gmw_wc(3.0, 60.0) / np.pi, "morlet": 13.4 / np.pi}      # the scale whose peak sits at Nyquist
EPS64 = float(np.finfo(np.float64).eps)


def _log(wavelet, count, nv):
    return S0[wavelet[0]] * 2.0 ** (np.arange(count) / nv)


@functools.lru_cache(maxsize=None)
def _piecewise():
    return np.ascontiguousarray(up.process_scales("log-piecewise", 777, MORLET, nv=8), dtype=np.float64).reshape(-1)


# tests/test_gpu_cwt_sst2.py's five shapes: (N, scales, wavelet, padtype, extra keywords)
CASES = [
    (300, lambda: _log(GMW, 37, 8), GMW, "reflect", dict()),
    (40, lambda: _log(MORLET, 20, 4), MORLET, "zero", dict(flipud=False)),
    (1000, lambda: np.linspace(2, 60, 50), GMW, "symmetric", dict(maprange="maximal")),
    (777, _piecewise, MORLET, "wrap", dict(maprange="peak")),
    (2500, lambda: _log(GMW, 12, 2), GMW, "replicate", dict()),
]
IDS = ["300-log37-gmw-reflect", "40-log20-morlet-zero", "1000-linear50-gmw-symmetric", "777-piecewise-morlet-wrap",
       "2500-log12-gmw-replicate"]
RUNS = list(range(len(CASES)))


def signal(N, seed=0):
    """tests/test_gpu_cwt_sst2.py's two crossing chirps (0.1 -> 0.4 and 0.4 -> 0.1 cycles/sample, 1e-3 seeded noise) with
    an impulse of height 8 at 2N/5, so that tau is not small everywhere."""
    a, _ = c2.chirp(N, 0.1, 0.4)
    b, _ = c2.chirp(N, 0.4, 0.1)
    return a + b + 1e-3 * np.random.default_rng(seed).standard_normal(N) + impulses(N, [2 * N // 5], 8.0)


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
    """(scales, row_const, f_asc, kind, f_idx) of case i: the grids `reassign_cwt` derives (shared with `ssq_cwt2`)."""
    N, sc, wavelet, pad, kw = CASES[i]
    code, p0, p1 = up._wavelet(wavelet)
    return up._cwt_freq_grid(sc(), None, None, kw.get("maprange", "peak"), N, code, p0, p1, 1 / FS)


@functools.lru_cache(maxsize=None)
def model(i, arith="fft", f32=False):
    """(W, w, tau, kk, mm) of the model on case i, on the library's tables; f32: on the float32-rounded input, reported in
    float32 with float32's default gamma.  Computed once, read-only."""
    N, sc, wavelet, pad, kw = CASES[i]
    s, _, f, kind, f_idx = grids(i)
    x = signal(N, i)
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    mw = (wavelet[0], *up._wavelet(wavelet)[1:])
    out = m.reassign_cwt_ref(x, mw, s, f, kind, f_idx, dt=1 / FS, padtype=pad, flipud=kw.get("flipud", True), arith=arith,
                             tabs=lib_tables(wavelet, s, c2.p2up(N)[0]), rdt=np.float32 if f32 else np.float64,
                             squeeze=False)[:5]
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gpu(i, rdt):
    """(Rx, Wx, ssq_freqs, scales, w, tau, kk, mm) of the library on case i; computed once, read-only."""
    N, sc, wavelet, pad, kw = CASES[i]
    out = up.reassign_cwt(signal(N, i).astype(rdt), wavelet, scales=sc(), fs=FS, padtype=pad, get_w=True, get_tau=True,
                          get_targets=True, **kw)
    for a in out:
        a.setflags(write=False)
    return out


def strong(W):
    return np.abs(W) >= 1e-2 * np.abs(W).max()


def fp64_bounds(i):
    """(w bound, tau bound) on the strong bins: 10 x the model's 'fft'-against-'dft' disagreement."""
    W, wm, taum = model(i)[:3]
    _, wd, taud = model(i, "dft")[:3]
    big = strong(W)
    return 10 * np.abs(wm - wd)[big].max(), 10 * np.abs(taum - taud)[big].max()


def near_a_boundary(i, tolw, tolt):
    """The bins of case i whose position in the model is within the allowed error of a rounding boundary, along
    frequency (the position moved by tolw crosses a half-integer) or along time (tau / dt within tolt / dt of one)."""
    s, _, f, kind, f_idx = grids(i)
    W, wm, taum = model(i)[:3]
    with np.errstate(all="ignore"):
        lo, hi = (c2.bin_positions(np.maximum(wm + d, 0), f, kind, f_idx)[1] for d in (-tolw, tolw))
        v = c2.bin_positions(wm, f, kind, f_idx)[1]
        width = np.maximum(np.abs(hi - lo), 1e-9)
        tie_k = np.abs(v - np.floor(v) - 0.5) <= width
        vt = taum * FS
        tie_m = np.abs(vt - np.floor(vt) - 0.5) <= max(tolt * FS, 1e-9)
    return tie_k | tie_m


def quantum(Wx):
    """q of a returned Wx [na, N]: Pmax 2^reassign_cwt_quantum_log2(na, N)."""
    mx = float(m.energy(Wx).max())
    return 0.0 if mx == 0 else 2.0 ** (int(np.ceil(np.log2(mx))) + up.reassign_cwt_quantum_log2(*Wx.shape))


def scatter_check(Rx, Wx, kk, mm):
    """Rx against the extended-precision scatter of the call's own maps -> (worst cell error / its bound, the error of
    the energy identity / the bound summed over the cells, every cell without a contribution exactly 0)."""
    keep = kk >= 0
    ref, cnt = m.scatter(m.energy(Wx, np.longdouble), kk, mm, keep, np.longdouble)
    R = ref.astype(np.float64)
    eps_out = float(np.finfo(Rx.dtype).eps)
    bound = cnt * quantum(Wx) / 2 + (cnt + 2) * EPS64 * R + eps_out * R
    err = np.abs(Rx.astype(np.longdouble) - ref).astype(np.float64)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    kept = m.energy(Wx, np.longdouble)[keep].sum()
    total = float(abs(Rx.astype(np.longdouble).sum() - kept)) / max(float(bound.sum()), 1e-300)
    return worst, total, bool((Rx[cnt == 0] == 0).all())


@pytest.mark.parametrize("i", RUNS, ids=IDS)
def test_parity_float64(i):
    """Wx bitwise `ssq_cwt2`'s; w, tau and the targets against the model.  Measured on an MI355X: see DESIGN 4.15."""
    N, sc, wavelet, pad, kw = CASES[i]
    s, _, f, kind, f_idx = grids(i)
    W, wm, taum, kkm, mmm = model(i)
    tolw, tolt = fp64_bounds(i)
    Rx, Wx, ssq_freqs, scales, w, tau, kk, mm = gpu(i, np.float64)
    assert Rx.shape == Wx.shape == w.shape == tau.shape == kk.shape == mm.shape == W.shape == (len(s), N)
    assert Wx.dtype == np.complex128 and Rx.dtype == w.dtype == tau.dtype == ssq_freqs.dtype == scales.dtype == np.float64
    assert kk.dtype == mm.dtype == np.int32
    assert np.array_equal(scales, s) and np.array_equal(ssq_freqs, f[::-1])
    Wx2 = up.ssq_cwt2(signal(N, i), wavelet, scales=sc(), fs=FS, padtype=pad, **kw)[1]
    assert np.array_equal(Wx, Wx2)
    big = strong(W)
    ew, et = np.abs(w - wm)[big].max(), np.abs(tau - taum)[big].max()
    tie = near_a_boundary(i, tolw, tolt)
    nbad = int((((kk != kkm) | (mm != mmm)) & big & ~tie).sum())
    ntie = int((tie & big).sum())
    print("Wx %.3g of max  w err %.3g Hz (tol %.3g, ratio %.3g)  tau err %.3g s (tol %.3g, ratio %.3g)  %d strong bins, "
          "targets differ %d, near a boundary %d" % (np.abs(Wx - W).max() / np.abs(W).max(), ew, tolw, ew / tolw, et, tolt,
                                                      et / tolt, big.sum(), nbad, ntie))
    assert np.array_equal(np.isposinf(w), kkm == -1) and np.array_equal(np.isposinf(tau), kkm == -1)
    assert ew <= tolw and et <= tolt
    assert nbad == 0
    assert ntie <= 1e-3 * big.sum()
    assert (Rx >= 0).all()


@pytest.mark.parametrize("i", RUNS, ids=IDS)
def test_parity_float32(i):
    """float32 in, complex64 / float32 / int32 out; the kernels compute in fp64 and round once on store.  Measured on an
    MI355X: see DESIGN 4.15."""
    W, wm, taum, kkm, mmm = model(i)                             # the complex128 model: the targets' reference
    Wf, wf, tauf = model(i, "fft", True)[:3]                     # on the float32-rounded input, in float32
    tolw, tolt = fp64_bounds(i)
    Rx, Wx, ssq_freqs, scales, w, tau, kk, mm = gpu(i, np.float32)
    assert Wx.dtype == np.complex64 and Rx.dtype == w.dtype == tau.dtype == ssq_freqs.dtype == scales.dtype == np.float32
    assert kk.dtype == mm.dtype == np.int32
    tolW = 10 * np.abs(Wf.astype(np.complex64) - Wf).max() / np.abs(Wf).max()
    eW = np.abs(Wx - Wf).max() / np.abs(Wf).max()
    big = strong(Wf)
    assert np.isfinite(w[big]).all() and np.isfinite(tau[big]).all()
    ew = np.abs(w[big].astype(np.float64) - wf[big].astype(np.float64))
    et = np.abs(tau[big].astype(np.float64) - tauf[big].astype(np.float64))
    bw = tolw + np.spacing(np.abs(wf[big])).astype(np.float64)
    bt = tolt + np.spacing(np.abs(tauf[big])).astype(np.float64)
    share = (((kk != kkm) | (mm != mmm)) & strong(W)).sum() / strong(W).sum()
    print("Wx %.3g of max (tol %.3g)  w worst %.3g of (fp64 bound + 1 ulp)  tau worst %.3g  targets differ share %.3g"
          % (eW, tolW, (ew / bw).max(), (et / bt).max(), share))
    assert eW <= tolW
    assert (ew <= bw).all() and (et <= bt).all()
    assert share <= 1e-3
    assert (Rx >= 0).all()


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("i", RUNS, ids=IDS)
def test_targets_follow_the_reported_maps(i, rdt):
    """kk is `upstream.ssqueeze`'s bin rule on the reported w (tests/test_gpu_ssqueeze.py's arithmetic: the restatement
    in float64 on the map widened to float64; fp64 exact, float32 a share of at most 1e-3 at half-bin ties), mm the time
    rule recomputed in the call's dtype, exactly; the bins that are not kept are those of w."""
    N, sc, wavelet, pad, kw = CASES[i]
    s, _, f, kind, f_idx = grids(i)
    Rx, Wx, _, _, w, tau, kk, mm = gpu(i, rdt)
    gone = np.isposinf(w)
    assert np.array_equal(kk == -1, gone) and np.array_equal(mm == -1, gone) and np.array_equal(np.isposinf(tau), gone)
    ref = sq.bins(w.astype(np.float64), sq.bin_params(f, kind != "linear"), len(s) - 1, kw.get("flipud", True))
    differ = ((kk != ref) & ~gone).sum() / max((~gone).sum(), 1)
    print("kk differs from the restatement on a share of %.3g" % differ)
    assert differ == 0 if rdt == np.float64 else differ <= 1e-3
    assert np.array_equal(mm[~gone], m.time_targets(tau, 1 / FS)[~gone])
    assert (kk[~gone] < len(s)).all() and (mm[~gone] < N).all()


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("i", RUNS, ids=IDS)
def test_rx_is_the_scatter_of_the_calls_own_maps(i, rdt):
    """Every cell within the derived bound of the module docstring, the energy identity within the bound summed over the
    cells, and a cell without a contribution exactly 0.  Measured on an MI355X: see DESIGN 4.15."""
    Rx, Wx, _, _, w, tau, kk, mm = gpu(i, rdt)
    worst, total, clean = scatter_check(Rx, Wx, kk, mm)
    print("worst cell: %.3g of its bound; energy identity: %.3g of the summed bound" % (worst, total))
    assert clean
    assert worst <= 1 and total <= 1


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
def test_batch_equals_single_calls_and_is_deterministic(rdt):
    X = np.stack([signal(300, sd) * a for sd, a in ((11, 1.0), (12, 300.0), (13, 1e-4))]).astype(rdt)   # three scales Pmax
    kw = dict(scales=_log(GMW, 37, 8), fs=FS, get_w=True, get_tau=True, get_targets=True)
    B = up.reassign_cwt(X, GMW, **kw)
    assert B[0].shape == B[1].shape == B[4].shape == B[7].shape == (3, 37, 300)
    for b in range(3):
        one = up.reassign_cwt(X[b], GMW, **kw)
        for k in (0, 1, 4, 5, 6, 7):
            assert np.array_equal(B[k][b], one[k]), (b, k)
    again = up.reassign_cwt(X, GMW, **kw)
    for k in (0, 1, 4, 5, 6, 7):
        assert np.array_equal(B[k], again[k]), k


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
def test_chunking_does_not_change_a_bit(rdt):
    """`work_limit_bytes` for 16 rows per chunk: the 2 x 37 rows go as 16 + 16 + 16 + 16 + 10, one chunk across the two
    signals, the last one partial; then one row per chunk."""
    lib = _lib.load()
    B, N, na = 2, 300, 37
    code = _lib.SSQ_F32 if rdt == np.float32 else _lib.SSQ_F64
    X = np.stack([signal(N, sd) for sd in (21, 22)]).astype(rdt)
    sc = _log(GMW, na, 8)
    wcode, p0, p1 = up._wavelet(GMW)
    s, _, f, kind, f_idx = up._cwt_freq_grid(sc, None, None, "peak", N, wcode, p0, p1, 1 / FS)
    mn = C.c_int64(0)
    assert lib.ssq_reassign_cwt_workspace_bytes(code, B, N, na, C.byref(mn)) > 0
    P = c2.p2up(N)[0]
    limit = mn.value + 15 * 96 * P
    res = []
    for lim in (0, limit, mn.value):
        Rx, w, tau = (np.empty((B, na, N), dtype=rdt) for _ in range(3))
        Wx = np.empty((B, na, N), dtype=np.complex64 if rdt == np.float32 else np.complex128)
        kk, mm = (np.empty((B, na, N), dtype=np.int32) for _ in range(2))
        _lib.check(lib.ssq_reassign_cwt_host(code, _vp(X), B, N, wcode, p0, p1, _vp(s), na, 1 / FS, _vp(f), up.FREQS[kind],
                                             f_idx or 0, 0, -1.0, up.VARIANT_FLIPUD, lim, _vp(Rx), _vp(Wx), _vp(w), _vp(tau),
                                             _vp(kk), _vp(mm)))
        res.append((Rx, Wx, w, tau, kk, mm))
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert np.array_equal(a, b)
    ref = up.reassign_cwt(X, GMW, scales=sc, fs=FS, get_w=True, get_tau=True, get_targets=True)
    for a, k in zip(res[0], (0, 1, 4, 5, 6, 7)):
        assert np.array_equal(a, ref[k]), k


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
def test_isolated_impulse(rdt):
    """padtype='zero', on the scales whose wavelet fits the padded length (tests/test_reassign_cwt_ref.py): every strong
    bin names the impulse's column, so that column holds at least their energy, and every cell without a contribution is
    exactly 0."""
    from tests.test_reassign_cwt_ref import FIT, GMW as MW, N, SCALES
    t0 = 200
    Rx, Wx, _, _, w, tau, kk, mm = up.reassign_cwt(impulses(N, [t0]).astype(rdt), ("gmw", {"gamma": MW[1], "beta": MW[2]}),
                                                   scales=SCALES[:FIT], padtype="zero", maprange="maximal", get_w=True,
                                                   get_tau=True, get_targets=True)
    big = strong(Wx)
    assert big.sum() > 5000 and (mm[big] == t0).all() and (kk[big] >= 0).all()
    f = up._cwt_freq_grid(SCALES[:FIT], None, None, "maximal", N, 0, MW[1], MW[2], 1.0)[2]
    own = sq.bins(w.astype(np.float64), sq.bin_params(f, True), FIT - 1, True)       # the row of its own frequency
    assert ((kk != own) & big).sum() <= (0 if rdt == np.float64 else 1e-3 * big.sum())
    worst, total, clean = scatter_check(Rx, Wx, kk, mm)
    E = m.energy(Wx, np.longdouble)
    col, rest = float(Rx[:, t0].astype(np.longdouble).sum()), float(np.delete(Rx, t0, axis=1).astype(np.longdouble).sum())
    print("column %d: %.6f of the energy; worst cell %.3g of its bound" % (t0, col / (col + rest), worst))
    assert worst <= 1 and total <= 1 and clean
    assert col >= float(E[big].sum()) * (1 - 1e-6)
    outside = np.ones(Rx.shape, dtype=bool)
    outside[:, t0] = False
    hit = np.zeros(Rx.shape, dtype=bool)
    hit[kk[kk >= 0], mm[kk >= 0]] = True
    assert not Rx[outside & ~hit].any()


def test_concentration_matches_the_model():
    """DESIGN 4.15's table: the GPU results reproduce the model's shares to four digits (the first-order column from
    `ssq_cwt`'s Tx: a constant row weight does not change a share)."""
    from tests.test_reassign_cwt_ref import FREQS, GMW as MW, N, SCALES, TABLE, model_table, table_shares
    wavelet = ("gmw", {"gamma": MW[1], "beta": MW[2]})
    kw = dict(scales=SCALES, maprange="maximal", flipud=False)
    assert np.allclose(up.reassign_cwt(np.ones(N), wavelet, **kw)[2][::-1], FREQS, rtol=1e-14)
    got = table_shares(lambda x: up.reassign_cwt(x, wavelet, **kw)[0].astype(np.float64),
                       lambda x: m.energy(up.ssq_cwt(x, wavelet, **kw)[0]))
    for (name, _, _, _), (gr, gs), (mr, ms) in zip(TABLE, got, model_table()):
        print("%-8s reassigned: GPU %.5f, model %.5f   first-order SST: GPU %.5f, model %.5f" % (name, gr, mr, gs, ms))
    for (gr, gs), (mr, ms) in zip(got, model_table()):
        assert abs(gr - mr) <= 5e-5 and abs(gs - ms) <= 5e-5


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
def test_degenerate_inputs(rdt):
    sc = _log(GMW, 20, 4)
    kw = dict(scales=sc, get_w=True, get_tau=True, get_targets=True)
    Rx, Wx, _, _, w, tau, kk, mm = up.reassign_cwt(np.zeros(200, dtype=rdt), GMW, **kw)
    assert not Rx.any() and not Wx.any() and np.isposinf(w).all() and np.isposinf(tau).all()
    assert (kk == -1).all() and (mm == -1).all()
    Rx, Wx, _, _, w, tau, kk, mm = up.reassign_cwt(np.full(200, 3.0, dtype=rdt), GMW, **kw)
    assert np.isfinite(Rx).all() and (Rx >= 0).all() and not np.isnan(w).any() and not np.isnan(tau).any()
    worst, total, clean = scatter_check(Rx, Wx, kk, mm)
    assert worst <= 1 and total <= 1 and clean
    # N = 2, na = 2: P = 4, the two scales whose peaks sit on its bins 2 and 1 ('zero' padding: a reflected pair of
    # samples is a constant plus a Nyquist term, which no analytic wavelet of these scales sees)
    Rx, Wx, _, _, w, tau, kk, mm = up.reassign_cwt(np.array([3.0, -1.0], dtype=rdt), GMW, scales=_log(GMW, 2, 1),
                                                   padtype="zero", get_w=True, get_tau=True, get_targets=True)
    assert Rx.shape == (2, 2) and np.isfinite(Rx).all() and Rx.any() and (kk >= 0).all()
    worst, total, clean = scatter_check(Rx, Wx, kk, mm)
    assert worst <= 1 and total <= 1 and clean
    Rx, Wx, _, _, w, tau, kk, mm = up.reassign_cwt(signal(200, 2).astype(rdt), GMW, gamma=1e6, **kw)
    assert np.abs(Wx).max() < 1e6 and not Rx.any() and np.isposinf(w).all() and (kk == -1).all() and (mm == -1).all()
    # one infinite sample: every transform of the signal is NaN, no energy is defined, and Rx is all zero (documented in
    # `reassign_cwt`); the other signal of the batch is what it is alone
    X = np.stack([signal(200, 4), signal(200, 5)]).astype(rdt)
    X[0, 77] = np.inf
    Rx, Wx, _, _, w, tau, kk, mm = up.reassign_cwt(X, GMW, **kw)
    assert not Rx[0].any() and not np.isfinite(Wx[0].view(rdt)).any()
    one = up.reassign_cwt(X[1], GMW, **kw)
    assert np.array_equal(Rx[1], one[0]) and np.array_equal(kk[1], one[6])


@pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
def test_options(rdt):
    x = signal(300, 7).astype(rdt)
    kw = dict(scales=_log(GMW, 37, 8), fs=FS)
    full = up.reassign_cwt(x, GMW, get_w=True, get_tau=True, get_targets=True, **kw)
    bare = up.reassign_cwt(x, GMW, **kw)
    assert len(bare) == 4 and np.array_equal(bare[0], full[0]) and np.array_equal(bare[1], full[1])
    only_tau = up.reassign_cwt(x, GMW, get_tau=True, **kw)
    assert len(only_tau) == 5 and np.array_equal(only_tau[4], full[5]) and np.array_equal(only_tau[0], full[0])
    down = up.reassign_cwt(x, GMW, flipud=False, get_w=True, get_targets=True, **kw)
    assert np.array_equal(down[0][::-1], full[0]) and np.array_equal(down[2], full[2])      # (ssq_freqs: as ssq_cwt2's)
    assert np.array_equal(down[4], full[4]) and np.array_equal(down[6], full[7])
    assert np.array_equal(np.where(down[5] >= 0, 36 - down[5], -1), full[6])
