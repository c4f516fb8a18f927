"""GPU tests of the synchroextracting and transient-extracting CWT, `upstream.set_cwt` and `upstream.tet_cwt`
(csrc/cwt_extract.hip), against the numpy model tests/helpers/extract_cwt_ref.py and against the kernels of
`ssq_cwt2`, `mssq_cwt` and `tssq_cwt`, whose maps they read.

The model runs on the library's own fp64 wavelet tables (`ssq_ssq_cwt2_tables`).  Tolerances come from the model's
disagreement with itself, never from the kernel: an fp64 map may differ from the model by 10 x the difference between the
model's FFT and DFT-matrix arithmetics on the same input, an fp32 one by 10 x the difference between the model in
complex64 arithmetic (`maps_in`) and in complex128, both on the cells with |W| >= 1e-2 max|W| (the margin of DESIGN 4.23,
for its reason).  Wx is held to the bounds of tests/test_gpu_cwt_sst2.py (10 x the model's FFT-against-DFT disagreement
of W; 2 eps of float32), and the share of strong cells whose keep decision differs from the complex128 model's to the
family's cap, 1e-3.  The inputs are such that the model's own rule taken in float32 and in float64 disagree on no strong
cell.  What holds bit for bit: Te = where(keep, Wx, +0) with `keep` rebuilt on the host, by the model's rule functions,
from the map the call itself reports and `set_cwt_row_edges`."""
import ctypes as C
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.helpers import cwt_sst2_ref as c2
from tests.helpers import extract_cwt_ref as m
from tests.helpers.tsst_ref import impulses

pytestmark = pytest.mark.gpu

FS = 2.0
DT = 1 / FS
GMW, MORLET = ("gmw", {"gamma": 3.0, "beta": 60.0}), ("morlet", {"mu": 13.4})
S0 = {"gmw": c2.gmw_wc(3.0, 60.0) / np.pi, "morlet": 13.4 / np.pi}      # the scale whose peak sits at Nyquist
EPS32, EPS64 = float(np.finfo(np.float32).eps), float(np.finfo(np.float64).eps)


def _log(wavelet, count, nv):
    return S0[wavelet[0]] * 2.0 ** (np.arange(count) / nv)


@functools.lru_cache(maxsize=None)
def _piecewise():
    """upstream's log-piecewise grid of 1000 samples at 8 to the octave without its first scale: 64 scales, the transition
    two scales from the end."""
    s = np.ascontiguousarray(up.process_scales("log-piecewise", 1000, MORLET, nv=8), dtype=np.float64).reshape(-1)[1:]
    assert len(s) == 64 and up._scales(s)[1] == "log-piecewise"
    return s


# (N, scales, wavelet, padtype): the four shapes (40, 7), (300, 33), (1000, 64), (6181, 20) -- columns that are no multiple
# of 256, one workgroup and several, tails of the row stride, DESIGN 4.22's tile case -- with the five pad types, both
# wavelets and the three scale grids spread over them
CASES = [
    (40, lambda: _log(MORLET, 7, 2), MORLET, "zero"),
    (300, lambda: _log(GMW, 33, 8), GMW, "reflect"),
    (300, lambda: np.linspace(2, 40, 33), GMW, "replicate"),
    (1000, _piecewise, MORLET, "wrap"),
    (6181, lambda: _log(GMW, 20, 4), GMW, "symmetric"),
]
IDS = ["40-log7-morlet-zero", "300-log33-gmw-reflect", "300-linear33-gmw-replicate", "1000-piecewise64-morlet-wrap",
       "6181-log20-gmw-symmetric"]
AXES = ("set", "tet")
RUNS = [(i, axis, order) for i in range(len(CASES)) for axis in AXES for order in (1, 2)]
ALL = pytest.mark.parametrize("i,axis,order", RUNS, ids=["%s-%s-o%d" % (IDS[i], axis, order) for i, axis, order in RUNS])
DTYPES = pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])


def signal(N, seed=None):
    """Two crossing chirps (0.05 -> 0.45, and 0.7 x a 0.40 -> 0.10 sweep) plus four impulses of height 8 at 0.29 N, 0.49 N,
    0.51 N and 0.78 N, on a floor of 1e-9 of seeded noise; seed: 0.05 of seeded noise on top.  The floor keeps every |W|
    of a float64 call orders of magnitude above its gamma of 2.2e-15: without it the rows far from both chirps hold
    nothing but the rounding noise of the transforms, and which of those cells fall below gamma is not a property of the
    definition (6181 samples, 20 scales: 209 of them).  It is far below float32's gamma of 1.2e-6, so a float32 call's
    +inf pattern stays a large one (40 % of the cells of that shape)."""
    a, _ = c2.chirp(N, 0.05, 0.45)
    b, _ = c2.chirp(N, 0.40, 0.10)
    x = a + 0.7 * b + impulses(N, [int(f * N) for f in (0.29, 0.49, 0.51, 0.78)], 8.0)
    x = x + 1e-9 * np.random.default_rng(N).standard_normal(N)
    return x if seed is None else x + 0.05 * np.random.default_rng(seed).standard_normal(N)


def call(axis, x, wavelet, **kw):
    """-> (Te, Wx, map) of `set_cwt` / `tet_cwt` with the map asked for."""
    if axis == "set":
        Te, Wx, _, _, w = up.set_cwt(x, wavelet, get_w=True, **kw)
        return Te, Wx, w
    Te, Wx, _, _, tau = up.tet_cwt(x, wavelet, get_tau=True, **kw)
    return Te, Wx, tau


def keep_of(axis, mp, wavelet, scales):
    """The keep rule rebuilt on the host from a reported map, in the map's own dtype, by the model's rule functions."""
    return m.keep_freq(mp, up.set_cwt_row_edges(wavelet, scales, fs=FS)) if axis == "set" else m.keep_time(mp, DT)


def model_wavelet(wavelet):
    return (wavelet[0], *up._wavelet(wavelet)[1:]) if wavelet[0] == "gmw" else (wavelet[0], up._wavelet(wavelet)[1])


@functools.lru_cache(maxsize=None)
def lib_tables(i):
    from tests.test_gpu_cwt_sst2 import lib_tables as tables
    N, sc, wavelet, pad = CASES[i]
    return tables(wavelet, sc(), c2.p2up(N)[0])


def _input(i, rounded):
    x = signal(CASES[i][0])
    return x.astype(np.float32).astype(np.float64) if rounded else x


@functools.lru_cache(maxsize=None)
def _sst2_parent(i, arith, rounded):
    N, sc, wavelet, pad = CASES[i]
    return m.sst2_parent(_input(i, rounded), model_wavelet(wavelet), sc(), DT, pad, 10 * (EPS32 if rounded else EPS64), arith,
                         lib_tables(i))


@functools.lru_cache(maxsize=None)
def model(i, axis, order, arith="fft", rounded=False):
    """(Te, W, map, keep) of the model on case i, on the wavelet tables of the library; computed once, read-only.
    rounded: on the input rounded to float32, in float32 with its default gamma (what a float32 call's kernel sees)."""
    N, sc, wavelet, pad = CASES[i]
    kw = dict(dt=DT, padtype=pad, order=order, arith=arith, tabs=lib_tables(i), rdt=np.float32 if rounded else np.float64)
    if axis == "set":
        out = m.set_cwt_ref(_input(i, rounded), model_wavelet(wavelet), sc(), parent=_sst2_parent(i, arith, rounded), **kw)
    else:
        out = m.tet_cwt_ref(_input(i, rounded), model_wavelet(wavelet), sc(), **kw)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model_c64(i, order):
    """(W, w, tau) of the model in complex64 arithmetic on case i (`maps_in`): what the float32 tolerance of a map is taken from."""
    N, sc, wavelet, pad = CASES[i]
    return m.maps_in(signal(N), model_wavelet(wavelet), sc(), np.complex64, dt=DT, padtype=pad, order=order, tabs=lib_tables(i))


@functools.lru_cache(maxsize=None)
def gpu(i, axis, order, rdt):
    N, sc, wavelet, pad = CASES[i]
    out = call(axis, signal(N).astype(rdt), wavelet, scales=sc(), fs=FS, padtype=pad, order=order)
    for a in out:
        a.setflags(write=False)
    return out


def strong(W):
    return np.abs(W) >= 1e-2 * np.abs(W).max()


def same_bits(a, b):
    """Equal bit for bit (a -0 is not a +0; NaN equals the same NaN)."""
    u = {4: np.uint32, 8: np.uint64}[a.real.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(u), np.ascontiguousarray(b).view(u))


# ---------------------------------------------------------------------------------------------- 1. self-consistency ----
@DTYPES
@ALL
def test_te_is_wx_under_the_calls_own_map_bitwise(i, axis, order, rdt):
    """Te is bit for bit where(keep, Wx, +0 + 0i), `keep` rebuilt on the host from the map the call reports and
    `set_cwt_row_edges` by the model's rule functions, in the call's dtype: the test that the kernel applies the stated
    rule, on every run."""
    N, sc, wavelet, pad = CASES[i]
    Te, Wx, mp = gpu(i, axis, order, rdt)
    cdt = np.complex64 if rdt == np.float32 else np.complex128
    assert Te.shape == Wx.shape == mp.shape == (len(sc()), N)
    assert Te.dtype == Wx.dtype == cdt and mp.dtype == rdt
    keep = keep_of(axis, mp, wavelet, sc())
    print("kept %d of %d cells (%d live)" % (keep.sum(), keep.size, (~np.isposinf(mp)).sum()))
    assert keep.any() and not keep.all()
    assert same_bits(Te, m.extract(Wx, keep))
    assert not np.isneginf(mp).any()
    gamma = 10 * float(np.finfo(rdt).eps)
    sure = np.abs(np.abs(Wx) - gamma) > 1e-3 * gamma             # (Wx is the fp64 W rounded: not on the threshold itself)
    assert np.array_equal(np.isposinf(mp)[sure], (np.abs(Wx) < gamma)[sure])


def test_returned_grids():
    N, sc, wavelet, pad = CASES[1]
    for fn in (up.set_cwt, up.tet_cwt):
        for rdt in (np.float64, np.float32):
            out = fn(signal(N).astype(rdt), wavelet, scales=sc(), fs=FS, padtype=pad)
            assert len(out) == 4 and out[2].dtype == out[3].dtype == rdt
            assert np.array_equal(out[2], sc().astype(rdt))
            assert np.array_equal(out[3], (up.tssq_cwt_row_freqs(wavelet, sc()) * FS).astype(rdt))
    t = np.arange(N) / FS
    assert same_bits(up.set_cwt(signal(N), wavelet, scales=sc(), t=t, padtype=pad)[0], gpu(1, "set", 2, np.float64)[0])


# ------------------------------------------------------------------------------------------------ 2. against the model ----
@ALL
def test_parity_float64(i, axis, order):
    """Wx, the +inf pattern, the map and the keep decision against the model.  Measured on an MI355X: see DESIGN 4.24."""
    N, sc, wavelet, pad = CASES[i]
    Tem, W, mpm, keepm = model(i, axis, order)
    _, Wd, mpd, _ = model(i, axis, order, "dft")
    Te, Wx, mp = gpu(i, axis, order, np.float64)
    tolW = 10 * np.abs(W - Wd).max() / np.abs(W).max()
    eW = np.abs(Wx - W).max() / np.abs(W).max()
    big = strong(W)
    with np.errstate(invalid="ignore"):
        tol = 10 * np.abs(mpm - mpd)[big].max()
        em = np.abs(mp - mpm)[big].max()
    share = (keep_of(axis, mp, wavelet, sc()) != keepm)[big].mean()
    print("Wx %.3g (tol %.3g)  map err %.3g (tol %.3g, %d strong cells)  keep differs on a share of %.3g"
          % (eW, tolW, em, tol, big.sum(), share))
    assert eW <= tolW
    assert np.array_equal(np.isposinf(mp), np.isposinf(mpm))
    assert em <= tol
    assert share <= 1e-3


@ALL
def test_parity_float32(i, axis, order):
    """float32 in, complex64 / float32 out; the kernel computes in fp64 on the widened signal and rounds on store.  The
    +inf pattern is that of the fp64 model on the float32-rounded input with float32's gamma; the map's bound is 10 x the
    disagreement of the model in complex64 arithmetic with the model in complex128; the model's own rule taken in float32
    on its fp64 map disagrees with its float64 rule on no strong cell (the inputs are chosen so).  Measured on an MI355X:
    see DESIGN 4.24."""
    N, sc, wavelet, pad = CASES[i]
    Tem, W, mpm, keepm = model(i, axis, order)
    mps = model_c64(i, order)[1 if axis == "set" else 2]
    _, Wr, mpr, keepr = model(i, axis, order, rounded=True)
    Te, Wx, mp = gpu(i, axis, order, np.float32)
    eW = np.abs(Wx - Wr).max() / np.abs(Wr).max()
    big = strong(W)
    with np.errstate(invalid="ignore"):
        tol = 10 * np.abs(mps.astype(np.float64) - mpm)[big].max()
        em = np.abs(mp.astype(np.float64) - mpm)[big].max()
    share = (keep_of(axis, mp, wavelet, sc()) != keepm)[big].mean()
    share_rule = (keep_of(axis, mpm.astype(np.float32), wavelet, sc()) != keepm)[big].mean()
    share_r = (keepr != keepm)[big].mean()
    print("Wx %.3g  map err %.3g (tol %.3g, %d strong cells)  keep differs on a share of %.3g (the model's float32 rule: "
          "%.3g; the fp64 model on the rounded input: %.3g)" % (eW, em, tol, big.sum(), share, share_rule, share_r))
    assert share_rule == 0
    assert eW <= 2 * EPS32
    assert np.array_equal(np.isposinf(mp), np.isposinf(mpr))
    assert em <= tol
    assert share <= 1e-3


# ------------------------------------------------------------------------------------- 3. against the parents' kernels ----
@DTYPES
@ALL
def test_against_the_kernels_of_the_parents(i, axis, order, rdt):
    """Wx is bitwise `ssq_cwt2`'s and `tssq_cwt`'s.  On every strong cell set_cwt keeps what `keep_freq` keeps of
    `ssq_cwt2`'s w (order 2; order 1: of `mssq_cwt(order=1, n_iter=1)`'s), tet_cwt what `tssq_cwt` would move by r = 0.
    Whether the maps are bitwise theirs is printed, not asserted (inlining changes the contraction)."""
    N, sc, wavelet, pad = CASES[i]
    Te, Wx, mp = gpu(i, axis, order, rdt)
    x = signal(N).astype(rdt)
    kw = dict(scales=sc(), fs=FS, padtype=pad)
    if axis == "set":
        if order == 2:
            _, Wp, _, _, mpp = up.ssq_cwt2(x, wavelet, get_w=True, **kw)
        else:
            _, Wp, _, _, mpp = up.mssq_cwt(x, wavelet, order=1, n_iter=1, get_w=True, **kw)
    else:
        _, Wp, _, _, mpp = up.tssq_cwt(x, wavelet, order=order, get_tau=True, **kw)
    big = strong(Wx)
    differ = int((keep_of(axis, mp, wavelet, sc()) != keep_of(axis, mpp, wavelet, sc()))[big].sum())
    print("keep differs on %d of %d strong cells; map bitwise theirs: %s" % (differ, big.sum(), same_bits(mp, mpp)))
    assert same_bits(Wx, Wp)
    assert differ == 0


# ------------------------------------------------------------------------------------------------- 4. bit identities ----
@DTYPES
@pytest.mark.parametrize("i", [0, 1], ids=[IDS[0], IDS[1]])
def test_batch_equals_single_calls_and_optional_outputs_change_nothing(rdt, i):
    N, sc, wavelet, pad = CASES[i]
    X = np.stack([signal(N, s) for s in (11, 12, 13)]).astype(rdt)
    for axis in AXES:
        for order in (1, 2):
            args = dict(scales=sc(), fs=FS, padtype=pad, order=order)
            B = call(axis, X, wavelet, **args)
            assert B[0].shape == (3, len(sc()), N)
            for b in range(3):
                one = call(axis, X[b], wavelet, **args)
                for k in range(3):
                    assert same_bits(B[k][b], one[k]), (axis, order, b, k)
            fn = up.set_cwt if axis == "set" else up.tet_cwt
            bare = fn(X, wavelet, get_Wx=False, **args)
            assert bare[1] is None and len(bare) == 4
            assert same_bits(bare[0], B[0]), (axis, order)
            assert same_bits(fn(X, wavelet, **args)[1], B[1]), (axis, order)


@DTYPES
@pytest.mark.parametrize("order", [1, 2])
def test_chunking_does_not_change_a_bit(order, rdt):
    """`work_limit_bytes` for 16 rows per chunk: the 2 x 33 rows go as 16 + 16 + 16 + 16 + 2, one chunk across the two
    signals, the last one ragged; then min_bytes, one row per chunk."""
    lib = _lib.load()
    N, sc, wavelet, pad = CASES[1]
    na = len(sc())
    X = np.stack([signal(N, s) for s in (21, 22)]).astype(rdt)
    mn = C.c_int64(0)
    assert lib.ssq_extract_cwt_workspace_bytes(_lib.SSQ_F32 if rdt == np.float32 else _lib.SSQ_F64, 2, N, na, order, C.byref(mn)) > 0
    P, M = c2.p2up(N)[0], 2 if order == 1 else 5
    assert mn.value == 16 * P * (2 + 2 * M)
    for axis in AXES:
        kw = dict(scales=sc(), fs=FS, padtype=pad, order=order)
        ref = call(axis, X, wavelet, **kw)
        for limit in (mn.value + 15 * 32 * M * P, mn.value):
            out = call(axis, X, wavelet, work_limit_bytes=limit, **kw)
            for k in range(3):
                assert same_bits(ref[k], out[k]), (axis, limit, k)


def _exec(lib, d, X, wavelet, scales, pad, ax, order, ws, outs, stream=None, ms=None):
    """`ssq_extract_cwt_exec` on device buffers of the Door `d`; outs: the three device buffers or None."""
    rdt = X.dtype.type
    code = _lib.SSQ_F32 if rdt == np.float32 else _lib.SSQ_F64
    wcode, p0, p1 = up._wavelet(wavelet)
    nu = up.tssq_cwt_row_freqs(wavelet, scales)
    edges = up.set_cwt_row_edges(wavelet, scales, fs=FS)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                                     # noqa: E731
    dx, dws = d.buf(X.nbytes, X), d.buf(ws[0])
    return lib.ssq_extract_cwt_exec(code, dx.p, X.shape[0], X.shape[1], wcode, p0, p1, vp(scales), vp(nu), vp(edges),
                                    len(scales), DT, up.PAD_MODES[pad], ax, order, -1.0, *[o.p if o else None for o in outs],
                                    dws.p, ws[1], stream, None if ms is None else ms.ctypes.data_as(C.POINTER(C.c_float)))


@DTYPES
def test_device_door_equals_the_host_call(rdt):
    """`ssq_extract_cwt_exec` on buffers from `ssq_dev_malloc` with guards behind every buffer, on a workspace of exactly
    min_bytes and of the preferred size, on the NULL stream and on a stream of the caller's: Te, Wx and the map equal the
    host call's bit for bit, with and without the optional outputs; kernel_ms is ONE float."""
    from tests.test_gpu_grid_limits import Door
    lib = _lib.load()
    N, sc, wavelet, pad = CASES[1]
    scales = sc()
    X = np.stack([signal(N, s) for s in (31, 32, 33)]).astype(rdt)
    cdt = np.complex64 if rdt == np.float32 else np.complex128
    shape = (3, len(scales), N)
    cells = int(np.prod(shape))
    st = C.c_void_p()
    _lib.check(lib.ssq_stream_create(C.byref(st)))
    try:
        for ax, axis in enumerate(AXES):
            for order in (2, 1):
                host = call(axis, X, wavelet, scales=scales, fs=FS, padtype=pad, order=order)
                mn = C.c_int64(0)
                pref = int(lib.ssq_extract_cwt_workspace_bytes(_lib.SSQ_F32 if rdt == np.float32 else _lib.SSQ_F64, 3, N,
                                                               len(scales), order, C.byref(mn)))
                assert 0 < mn.value < pref
                for ws, stream, full in ((mn.value, None, True), (pref, st, True), (pref, None, False)):
                    ms = np.full(3, -7.0, dtype=np.float32)
                    with Door() as d:
                        dT = d.buf(cells * np.dtype(cdt).itemsize)
                        dW = d.buf(cells * np.dtype(cdt).itemsize) if full else None
                        dm = d.buf(cells * np.dtype(rdt).itemsize) if full else None
                        _lib.check(_exec(lib, d, X, wavelet, scales, pad, ax, order, (ws, ws), (dT, dW, dm), stream, ms))
                        dev = [dT.get(shape, cdt)] + ([dW.get(shape, cdt), dm.get(shape, rdt)] if full else [])
                    assert ms[0] > 0 and ms[1] == -7.0 and ms[2] == -7.0
                    for name, a, h in zip(("Te", "Wx", "map"), dev, host):
                        assert same_bits(a, np.ascontiguousarray(h)), (axis, order, ws, name)
    finally:
        lib.ssq_stream_destroy(st)


def test_a_workspace_one_byte_short_is_refused_with_te_untouched():
    from tests.test_gpu_grid_limits import Door
    lib = _lib.load()
    N, sc, wavelet, pad = CASES[1]
    scales = sc()
    X = np.stack([signal(N, s) for s in (31, 32)]).astype(np.float32)
    cells = 2 * len(scales) * N
    mn = C.c_int64(0)
    assert lib.ssq_extract_cwt_workspace_bytes(_lib.SSQ_F32, 2, N, len(scales), 2, C.byref(mn)) > 0
    for ax in (0, 1):
        with Door() as d:
            dT = d.buf(cells * 8)
            rc = _exec(lib, d, X, wavelet, scales, pad, ax, 2, (mn.value, mn.value - 1), (dT, None, None))
            assert rc != 0 and "workspace" in lib.ssq_last_error().decode()
            assert (dT.get((cells,), np.complex64).view(np.uint8) == 0xA5).all()      # nothing ran: Te is as it was filled


# ----------------------------------------------------------------------------------------------------- 5. grid limit ----
@pytest.mark.parametrize("axis", AXES)
def test_more_rows_than_the_grids_y_limit(axis):
    """514 signals x 128 scales = 65792 rows in one chunk, past the 65535 blocks of the grid's y dimension, which stride:
    rows 0, 65535 and 65791 -- signal 0, and the last row of signals 511 and 513 -- equal their single-signal calls."""
    na, N = 128, 16
    scales = _log(GMW, na, 32)
    rng = np.random.default_rng(5)
    base = rng.standard_normal((7, N)).astype(np.float32)
    base[:, 5] += 4.0
    idx = np.arange(514) % 7
    X = np.ascontiguousarray(base[idx])
    mn = C.c_int64(0)
    for order in (2, 1):
        pref = _lib.load().ssq_extract_cwt_workspace_bytes(_lib.SSQ_F32, 514, N, na, order, C.byref(mn))
        assert pref == 16 * 32 * (514 + 2 * (5 if order == 2 else 2) * 514 * na)             # every row in ONE chunk
        Te, Wx, mp = call(axis, X, GMW, scales=scales, order=order)
        assert Te.shape == (514, na, N)
        for b, row in ((0, 0), (511, na - 1), (513, na - 1)):
            assert b * na + row in (0, 65535, 65791)
            one = call(axis, base[idx[b]], GMW, scales=scales, order=order)
            assert one[0].any() and (one[0] == 0).any()
            for got, want in zip((Te[b], Wx[b], mp[b]), one):
                assert same_bits(got[row], want[row]), (order, b, row)
                assert same_bits(got, want), (order, b)


# ------------------------------------------------------------------------------------------------------ 6. semantics ----
@pytest.mark.parametrize("order", [1, 2])
@DTYPES
def test_impulse_share_matches_the_model(rdt, order):
    from tests.test_extract_cwt_ref import IMPULSE_SHARE, SCALES, T0, column_share, impulse
    Te, Wx, _, _ = up.tet_cwt(impulse().astype(rdt), GMW, scales=SCALES, padtype="zero", order=order)
    share = column_share(Te.astype(np.complex128))
    print("order %d: %.6f of the kept energy on column %d (model %.4f)" % (order, share, T0, IMPULSE_SHARE[order]))
    assert abs(share - IMPULSE_SHARE[order]) <= 5e-5
    assert (Te[:, T0] != 0).all() and same_bits(Te[:, T0], Wx[:, T0])


@pytest.mark.parametrize("order", [1, 2])
@DTYPES
def test_chirp_share_matches_the_model(rdt, order):
    from tests.test_extract_cwt_ref import CHIRP_SHARE, SCALES, chirp, own_row_share
    Te = up.set_cwt(chirp()[0].astype(rdt), GMW, scales=SCALES, order=order, get_Wx=False)[0]
    share = own_row_share(Te.astype(np.complex128))
    print("order %d: own-row share %.7f (model %.3f)" % (order, share, CHIRP_SHARE[order]))
    assert abs(share - CHIRP_SHARE[order]) <= 5e-4


@DTYPES
def test_degenerate_inputs(rdt):
    N, sc, wavelet, pad = CASES[1]
    for axis in AXES:
        for order in (1, 2):
            Te, Wx, mp = call(axis, np.zeros(N, dtype=rdt), wavelet, scales=sc(), fs=FS, order=order)
            assert not Te.any() and not Wx.any() and np.isposinf(mp).all()
            assert not np.signbit(Te.real).any() and not np.signbit(Te.imag).any()
            Te, Wx, mp = call(axis, signal(N).astype(rdt), wavelet, scales=sc(), fs=FS, order=order, gamma=1e6)
            assert not Te.any() and Wx.any() and np.isposinf(mp).all()
    # N = 2, na = 2: P = 4
    Te, Wx, mp = call("tet", np.array([3.0, -1.0], dtype=rdt), GMW, scales=_log(GMW, 2, 1), padtype="zero")
    assert Te.shape == (2, 2) and np.isfinite(Wx.view(rdt)).all()
    # one infinite sample: every map of that signal is NaN, a NaN is kept nowhere; the other signal is what it is alone
    X = np.stack([signal(N, 4), signal(N, 5)]).astype(rdt)
    X[0, 77] = np.inf
    for axis in AXES:
        Te, Wx, mp = call(axis, X, wavelet, scales=sc(), fs=FS)
        assert not Te[0].any() and not np.isfinite(Wx[0].view(rdt)).any()
        one = call(axis, X[1], wavelet, scales=sc(), fs=FS)
        assert same_bits(Te[1], one[0]) and Te[1].any()
