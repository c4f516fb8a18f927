"""GPU tests of the synchroextracting and transient-extracting STFT, `upstream.set_stft` and `upstream.tet_stft`
(csrc/stft_extract.hip), against the numpy model tests/helpers/extract_ref.py and against the kernels of
`mssq_stft` and `tssq_stft`, whose maps they read.

The model runs on the library's own fp64 window tables (`ssq_ssq_stft2_window_tables`).  Tolerances come from the model's
disagreement with itself, never from the kernel: an fp64 map may differ from the model by 10 x the difference between the
model's FFT and DFT-matrix arithmetics on the same input, an fp32 one by 10 x the difference between the model in
complex64 and in complex128, both on the cells with |V| >= 1e-2 max|V|.  Sx is held to the project's STFT tolerances
(1e-11 / 2e-6 of max|Sx|), and the share of strong cells whose keep decision differs from the complex128 model's or from
the parent kernels' to the family's cap, 1e-3.  What holds bit for bit: Te = where(keep, Sx, +0) with `keep` rebuilt on
the host from the map the call itself reports."""
import ctypes as C
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.helpers import extract_ref as m
from tests.helpers import sst2_ref as s2
from tests.helpers import tsst_ref as ts
from tests.test_gpu_tsst import lib_tables, window

pytestmark = pytest.mark.gpu

FS = 250.0
EPS32 = float(np.finfo(np.float32).eps)
# (N, n_fft, hop, padtype, extra keywords): 256 frames a round and a ragged last tile; a hop that does not divide n;
# modulated=False; a 4-frame tile; a frame spanning several waves; one frame per round; a signal shorter than the window
CASES = [
    (300, 16, 1, "reflect", dict()),
    (1000, 64, 3, "zero", dict()),
    (1024, 256, 1, "symmetric", dict(modulated=False)),
    (4096, 1024, 8, "wrap", dict()),
    (4096, 2048, 64, "replicate", dict()),
    (5000, 4096, 64, "reflect", dict()),
    (40, 64, 1, "zero", dict()),
]
AXES = ("set", "tet")
RUNS = [(i, axis, order) for i in range(len(CASES)) for axis in AXES for order in (1, 2)]
IDS = ["%d-%d-%d-%s-%s-o%d" % (CASES[i][:4] + (axis, order)) for i, axis, order in RUNS]
ALL = pytest.mark.parametrize("i,axis,order", RUNS, ids=IDS)
DTYPES = pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])


def signal(N):
    """Two crossing chirps (0.05 -> 0.45, and 0.7 x a 0.40 -> 0.10 sweep) plus four impulses of height 8 at 0.29 N, 0.49 N,
    0.51 N and 0.78 N."""
    a, _ = s2.chirp(N, 0.05, 0.45)
    b, _ = s2.chirp(N, 0.40, 0.10)
    return a + 0.7 * b + ts.impulses(N, [int(f * N) for f in (0.29, 0.49, 0.51, 0.78)], 8.0)


def call(axis, x, win, **kw):
    """-> (Te, Sx, map) of `set_stft` / `tet_stft` with the map asked for."""
    if axis == "set":
        Te, Sx, _, w = up.set_stft(x, win, get_w=True, **kw)
        return Te, Sx, w
    Te, Sx, _, _, tau = up.tet_stft(x, win, get_tau=True, **kw)
    return Te, Sx, tau


def keep_of(axis, mp, hop, fs=FS):
    """The keep rule rebuilt on the host from a reported map, in the map's own dtype."""
    return m.keep_freq(mp, fs) if axis == "set" else m.keep_time(mp, hop, fs)


@functools.lru_cache(maxsize=None)
def model(i, axis, order, arith="fft", dtype=np.complex128, rounded=False):
    """(Te, V, map, keep) of the model on case i, on the window tables of the library; computed once, read-only.
    rounded: on the input rounded to float32 with float32's default gamma (what a float32 call's kernel sees)."""
    N, n, hop, pad, kw = CASES[i]
    x = signal(N)
    extra = dict(gamma=10 * EPS32) if rounded else dict()
    if rounded:
        x = x.astype(np.float32).astype(np.float64)
    ref = m.set_ref if axis == "set" else m.tet_ref
    out = ref(x, window(n), n, hop_len=hop, fs=FS, padtype=pad, order=order, arith=arith, dtype=dtype,
              tables=lib_tables(n), **extra, **kw)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gpu(i, axis, order, rdt):
    N, n, hop, pad, kw = CASES[i]
    out = call(axis, signal(N).astype(rdt), window(n), n_fft=n, hop_len=hop, fs=FS, padtype=pad, order=order, **kw)
    for a in out:
        a.setflags(write=False)
    return out


def strong(V):
    return np.abs(V) >= 1e-2 * np.abs(V).max()


def same_bits(a, b):
    """Equal bit for bit (a -0 is not a +0; NaN equals the same NaN)."""
    u = {4: np.uint32, 8: np.uint64}[a.real.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(u), np.ascontiguousarray(b).view(u))


# ---------------------------------------------------------------------------------------------- 1. self-consistency ----
@DTYPES
@ALL
def test_te_is_sx_under_the_calls_own_map_bitwise(i, axis, order, rdt):
    """Te is bit for bit where(keep, Sx, +0 + 0i), `keep` rebuilt on the host from the map the call reports by the rule in
    the call's dtype: any tile, transpose or store-loop error shows here."""
    N, n, hop, pad, kw = CASES[i]
    Te, Sx, mp = gpu(i, axis, order, rdt)
    cdt = np.complex64 if rdt == np.float32 else np.complex128
    assert Te.shape == Sx.shape == mp.shape == (n // 2 + 1, (N - 1) // hop + 1)
    assert Te.dtype == Sx.dtype == cdt and mp.dtype == rdt
    keep = keep_of(axis, mp, hop)
    print("kept %d of %d cells (%d live)" % (keep.sum(), keep.size, (~np.isposinf(mp)).sum()))
    assert keep.any() and not keep.all()
    assert same_bits(Te, m.extract(Sx, keep))
    gamma = 10 * float(np.finfo(rdt).eps)
    sure = np.abs(np.abs(Sx) - gamma) > 1e-3 * gamma             # (Sx is the fp64 V rounded: not on the threshold itself)
    assert np.array_equal(np.isposinf(mp)[sure], (np.abs(Sx) <= gamma)[sure])


# ------------------------------------------------------------------------------------------------ 2. against the model ----
@ALL
def test_parity_float64(i, axis, order):
    """Sx, the +inf pattern, the map and the keep decision against the model.  Measured on an MI355X: Sx <= 3.9e-16 of its
    maximum, the +inf pattern equal, the map error on strong cells at 0.02 ... 0.19 of its bound, and no strong cell whose
    keep differs from the model's in any of the 28 runs."""
    N, n, hop, pad, kw = CASES[i]
    Tem, V, mpm, keepm = model(i, axis, order)
    mpd = model(i, axis, order, "dft")[2]
    Te, Sx, mp = gpu(i, axis, order, np.float64)
    eS = np.abs(Sx - V).max() / np.abs(V).max()
    big = strong(V)
    with np.errstate(invalid="ignore"):
        tol = 10 * np.abs(mpm - mpd)[big].max()
        em = np.abs(mp - mpm)[big].max()
    share = (keep_of(axis, mp, hop) != keepm)[big].mean()
    print("Sx %.3g  map err %.3g (tol %.3g, %d strong cells)  keep differs on a share of %.3g" % (eS, em, tol, big.sum(), share))
    assert eS <= 1e-11
    assert np.array_equal(np.isposinf(mp), np.isposinf(mpm))
    assert em <= tol
    assert share <= 1e-3


@ALL
def test_parity_float32(i, axis, order):
    """float32 in, complex64 / float32 out; the kernel computes in fp64 on the widened signal and rounds on store.  The
    +inf pattern is that of the complex128 model on the float32-rounded input with float32's gamma.  Measured on an
    MI355X: Sx <= 7.3e-8 of its maximum; the map error on strong cells at 0.03 ... 0.15 of its bound; the share of strong
    cells whose keep differs from the complex128 model's is 0 in 23 of 28 runs and 7.6e-6 ... 7.4e-5 in the others (all SET:
    1024-256-1 order 2, 4096-1024-8 and 5000-4096-64 both orders; cap 1e-3), of which the fp64 model on the rounded input
    reproduces 6.2e-5 and 4.6e-5: the rounding of the INPUT; the rest is the rule taken in float32."""
    N, n, hop, pad, kw = CASES[i]
    Tem, V, mpm, keepm = model(i, axis, order)
    mps = model(i, axis, order, "fft", np.complex64)[2]
    Te, Sx, mp = gpu(i, axis, order, np.float32)
    eS = np.abs(Sx - V).max() / np.abs(V).max()
    big = strong(V)
    with np.errstate(invalid="ignore"):
        tol = 10 * np.abs(mps.astype(np.float64) - mpm)[big].max()
        em = np.abs(mp.astype(np.float64) - mpm)[big].max()
    share = (keep_of(axis, mp, hop) != keepm)[big].mean()
    share_r = (model(i, axis, order, rounded=True)[3] != keepm)[big].mean()
    print("Sx %.3g  map err %.3g (tol %.3g, %d strong cells)  keep differs on a share of %.3g (the fp64 model on the "
          "rounded input: %.3g)" % (eS, em, tol, big.sum(), share, share_r))
    assert eS <= 2e-6
    assert np.array_equal(np.isposinf(mp), np.isposinf(model(i, axis, order, rounded=True)[2]))
    assert em <= tol
    assert share <= 1e-3


# ------------------------------------------------------------------------------------- 3. against the parent's kernels ----
@DTYPES
@ALL
def test_keep_agrees_with_the_kernels_of_mssq_stft_and_tssq_stft(i, axis, order, rdt):
    """set_stft keeps what `mssq_stft(order, n_iter=1)` leaves on its own row, tet_stft what `tssq_stft` would move by
    r = 0: compared on the strong cells, cap 1e-3.  Whether Sx and the maps are bitwise theirs is printed, not asserted.
    Measured on an MI355X: keep differs on no strong cell in all 56 runs; Sx is bitwise theirs in all 56; the map in all 28
    order-1 runs and in 20 of the 28 order-2 runs (the inlined second-order operator ends on another last bit on some cells
    of 300-16-1, 1024-256-1 and 5000-4096-64)."""
    N, n, hop, pad, kw = CASES[i]
    Te, Sx, mp = gpu(i, axis, order, rdt)
    x, win = signal(N).astype(rdt), window(n)
    args = dict(n_fft=n, hop_len=hop, fs=FS, padtype=pad, order=order, **kw)
    if axis == "set":
        _, Sp, _, _, mpp, bins = up.mssq_stft(x, win, n_iter=1, get_w=True, get_bins=True, **args)
        keepp = bins == np.arange(n // 2 + 1)[:, None]
    else:
        _, Sp, _, _, mpp = up.tssq_stft(x, win, get_tau=True, **args)
        keepp = m.keep_time(mpp, hop, FS)
    big = strong(Sx)
    share = (keep_of(axis, mp, hop) != keepp)[big].mean()
    print("keep differs on a share of %.3g of %d strong cells; Sx bitwise theirs: %s; map bitwise theirs: %s"
          % (share, big.sum(), same_bits(Sx, Sp), same_bits(mp, mpp)))
    assert share <= 1e-3


# ------------------------------------------------------------------------------------------------- 4. bit identities ----
@DTYPES
@pytest.mark.parametrize("i", [0, 4], ids=["300-16-1", "4096-2048-64"])
def test_batch_equals_single_calls_and_optional_outputs_change_nothing(rdt, i):
    N, n, hop, pad, kw = CASES[i]
    X = np.stack([signal(N) + 0.05 * np.random.default_rng(s).standard_normal(N) for s in (11, 12, 13)]).astype(rdt)
    win = window(n)
    for axis in AXES:
        for order in (1, 2):
            args = dict(n_fft=n, hop_len=hop, fs=FS, padtype=pad, order=order, **kw)
            B = call(axis, X, win, **args)
            assert B[0].shape == (3, n // 2 + 1, (N - 1) // hop + 1)
            for b in range(3):
                one = call(axis, X[b], win, **args)
                for k in range(3):
                    assert same_bits(B[k][b], one[k]), (axis, order, b, k)
            fn = up.set_stft if axis == "set" else up.tet_stft
            bare = fn(X, win, get_Sx=False, **args)
            assert bare[1] is None and len(bare) == (3 if axis == "set" else 4)
            assert same_bits(bare[0], B[0]), (axis, order)
            assert same_bits(fn(X, win, **args)[1], B[1]), (axis, order)


@DTYPES
def test_device_door_equals_the_host_call(rdt):
    """`ssq_extract_stft_exec` on buffers from `ssq_dev_malloc`, a workspace of exactly `ssq_extract_stft_workspace_bytes`
    (none at all for float64: NULL and 0 bytes) and guards behind every buffer: Te, Sx and the map equal the host call's bit
    for bit, with and without the optional outputs; kernel_ms is ONE float."""
    from tests.test_gpu_grid_limits import FS as FS_ST
    from tests.test_gpu_grid_limits import HOP, NFFT, Door, assert_same, gwin
    from tests.test_gpu_host_slices import signals
    lib = _lib.load()
    X = signals(rdt)
    B, N = X.shape
    code = _lib.SSQ_F32 if rdt == np.float32 else _lib.SSQ_F64
    cdt = np.complex64 if rdt == np.float32 else np.complex128
    win = gwin()
    shape = (B, NFFT // 2 + 1, (N - 1) // HOP + 1)
    cells = int(np.prod(shape))
    ws = int(lib.ssq_extract_stft_workspace_bytes(code, B, N, NFFT, HOP))
    assert ws == (8 * B * N if rdt == np.float32 else 0)
    for ax, axis in enumerate(AXES):
        for order in (2, 1):
            host = call(axis, X, win, n_fft=NFFT, hop_len=HOP, fs=FS_ST, order=order)
            for full in (True, False):
                ms = np.full(2, -7.0, dtype=np.float32)
                with Door() as d:
                    dx = d.buf(X.nbytes, X)
                    dws = d.buf(ws) if ws else None
                    dT = d.buf(cells * np.dtype(cdt).itemsize)
                    dS = d.buf(cells * np.dtype(cdt).itemsize) if full else None
                    dm = d.buf(cells * np.dtype(rdt).itemsize) if full else None
                    _lib.check(lib.ssq_extract_stft_exec(
                        code, dx.p, B, N, win.ctypes.data_as(C.c_void_p), NFFT, HOP, FS_ST, up.PAD_MODES["reflect"], ax, order,
                        -1.0, 3, dT.p, dS.p if full else None, dm.p if full else None, dws.p if ws else None, ws,
                        ms.ctypes.data_as(C.POINTER(C.c_float))))
                    dev = [dT.get(shape, cdt)] + ([dS.get(shape, cdt), dm.get(shape, rdt)] if full else [])
                assert ms[0] > 0 and ms[1] == -7.0
                for name, a, h in zip(("Te", "Sx", "map"), dev, host):
                    assert_same(a, np.ascontiguousarray(h), "%s order %d: device %s against the host call's" % (axis, order, name))
                    assert same_bits(a, np.ascontiguousarray(h))


def test_a_workspace_one_byte_short_is_refused_without_a_launch():
    from tests.test_gpu_grid_limits import HOP, NFFT, Door, gwin
    from tests.test_gpu_host_slices import signals
    lib = _lib.load()
    X = signals(np.float32)
    B, N = X.shape
    win = gwin()
    cells = B * (NFFT // 2 + 1) * ((N - 1) // HOP + 1)
    ws = int(lib.ssq_extract_stft_workspace_bytes(_lib.SSQ_F32, B, N, NFFT, HOP))
    with Door() as d:
        dx, dws, dT = d.buf(X.nbytes, X), d.buf(ws), d.buf(cells * 8)
        rc = lib.ssq_extract_stft_exec(_lib.SSQ_F32, dx.p, B, N, win.ctypes.data_as(C.c_void_p), NFFT, HOP, 2.0, 0, 0, 2, -1.0,
                                       3, dT.p, None, None, dws.p, ws - 1, None)
        assert rc != 0 and "workspace" in lib.ssq_last_error().decode()
        assert (dT.get((cells,), np.complex64).view(np.uint8) == 0xA5).all()      # nothing ran: Te is as it was filled


@DTYPES
def test_host_slices_change_nothing(rdt):
    from tests.test_gpu_grid_limits import FS as FS_ST
    from tests.test_gpu_grid_limits import HOP, NFFT, gwin
    from tests.test_gpu_host_slices import assert_slices_change_nothing, signals
    X = signals(rdt)
    for axis in AXES:
        for order in (1, 2):
            assert_slices_change_nothing(
                lambda: call(axis, X, gwin(), n_fft=NFFT, hop_len=HOP, fs=FS_ST, order=order), "%s order %d" % (axis, order))


# ------------------------------------------------------------------------------------------------------ 5. semantics ----
@pytest.mark.parametrize("order", [1, 2])
@DTYPES
def test_tone_identity(rdt, order):
    """A tone on a bin centre comes back from the cells SET keeps, to within 10 x the complex128 model's own error (the
    model on the float32-rounded input, Te rounded to complex64, is at 2.2e-8 and 9.8e-8: inside it too)."""
    from tests.test_extract_ref import NFFT, SIGMA, TONE_ERR, tone, tone_error
    win = s2.gauss_window(NFFT, SIGMA)
    Te = up.set_stft(tone().astype(rdt), win, n_fft=NFFT, order=order, get_Sx=False)[0]
    err = tone_error(Te.astype(np.complex128), win)
    tol = 10 * TONE_ERR[order]
    print("order %d: relative L2 error %.3e (model %.3e)" % (order, err, TONE_ERR[order]))
    assert err <= tol


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("hop", [1, 4])
@DTYPES
def test_isolated_impulse_under_tet(rdt, hop, order):
    from tests.test_extract_ref import IMPULSES, N, NFFT, SIGMA
    win = s2.gauss_window(NFFT, SIGMA)
    Te, Sx, _, _ = up.tet_stft(ts.impulses(N, IMPULSES).astype(rdt), win, n_fft=NFFT, hop_len=hop, order=order)
    seen = np.abs(Sx) > 1e-6
    cols = [t0 // hop for t0 in IMPULSES]
    assert np.unique(np.nonzero((Te != 0) & seen)[1]).tolist() == cols
    assert np.allclose(np.abs(Te[:, cols]), win[NFFT // 2], rtol=1e-6, atol=0)
    assert not np.delete(Te, cols, axis=1)[np.delete(seen, cols, axis=1)].any()


@pytest.mark.parametrize("order", [1, 2])
def test_chirp_share_matches_the_model(order):
    from tests.test_extract_ref import COLS, NFFT, SIGMA, chirp, own_bin_share
    x, _ = chirp()
    win = s2.gauss_window(NFFT, SIGMA)
    sm = own_bin_share(m.set_ref(x, win, NFFT, order=order)[0])
    Te, _, _, w = up.set_stft(x, win, n_fft=NFFT, order=order, get_w=True)
    sg = own_bin_share(Te)
    print("order %d: own-bin share GPU %.4f, model %.4f; kept per column %.3f" % (order, sg, sm, (Te[:, COLS] != 0).sum(0).mean()))
    assert abs(sg - sm) <= 5e-4


def test_degenerate_inputs():
    win = window(64)
    for fn in (up.set_stft, up.tet_stft):
        out = fn(np.zeros(500, dtype=np.float32), win, n_fft=64, hop_len=3)
        assert not out[0].any() and not out[1].any() and not np.signbit(out[0].real).any()
        out = fn(signal(500), win, n_fft=64, hop_len=3, gamma=1e6)
        assert not out[0].any() and out[1].any()
        out = fn(np.full(1, 3.0), win, n_fft=64)
        assert out[0].shape == (33, 1)


# ----------------------------------------------------------------------------------------------------- 6. grid limit ----
@pytest.mark.parametrize("axis", AXES)
def test_a_batch_of_65537_signals(axis):
    """the batch goes through the grid's y dimension 65535 signals a launch; signals 0, 65535 and 65536
    equal their single calls."""
    from tests.test_gpu_tsst import two_chirps
    base = np.stack([two_chirps(16, 70 + b) for b in range(7)]).astype(np.float32)
    base[:, 5] += 4.0
    idx = np.arange(65537) % 7
    win = window(16)
    Te, Sx, mp = call(axis, np.ascontiguousarray(base[idx]), win, n_fft=16, order=1)
    assert Te.shape == (65537, 9, 16)
    for b in (0, 65535, 65536):
        one = call(axis, base[idx[b]], win, n_fft=16, order=1)
        assert one[0].any() and (one[0] == 0).any()
        for got, want in zip((Te[b], Sx[b], mp[b]), one):
            assert same_bits(got, want), b
