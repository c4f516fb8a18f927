"""The slices of the synchronous host entry points after the first (csrc/dev_buffers.h: `slice_signals`, `host_sliced`).

A host entry point keeps as many signals on the device as fit, and every test shape of the suite fits whole: without a cap
the loop over slices runs once and `b0 > 0` never happens.  `ssq_host_slice_cap` (include/ssq_hip.h) caps the slice for
the whole process, so here every caller of `slice_signals` runs 5 signals in slices of 2, 2, 1 and of 1, and every array
it returns must equal the uncapped call's bit for bit (`np.array_equal`): the H2D offset of a slice, the D2H offset of
every output, the optional outputs, and a workspace carved for fewer signals than the batch.

The STFT family runs its smallest shape (5 signals of 32 samples, n_fft 16, hop 8: tests/test_gpu_grid_limits.py's);
the signals differ and each carries an impulse, which moves time targets.

Which hosts slice: the fp64 STFT pipelines (ssq_stft2, mssq_stft, tssq_stft, tmssq_stft, reassign_stft), the batched
inverses and the walks, on a workspace that is linear in the signals; and the two ConceFT transforms (conceft_stft,
conceft_cwt), whose workspace is fixed by the call (`work_limit_bytes`) and walked in inner slices under every host
slice.  The fp64 CWT map pipelines take the batch whole."""
import ctypes as C

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.test_gpu_grid_limits import (CWT_IDS, CWT_RUNS, FS, GMW, HOP, N_ST, NFFT, STFT_IDS, STFT_RUNS, base_signals,
                                        cwt_grids, cwt_host, cwt_scales, gwin, stft_host)

pytestmark = pytest.mark.gpu

B = 5
CAPS = (2, 1)
DTYPES = pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])


def signals(rdt):
    """[5, 32]: five different base signals of the grid-limits module and on each, at another sample, an impulse six times
    its largest sample, 5 samples from the centre of a frame (hop 8: more than half a hop, so the frame's bins move)."""
    X = base_signals(N_ST)[:B].copy()
    for b, at in enumerate((5, 11, 13, 19, 29)):
        X[b, at] += 6.0 * np.abs(X[b]).max()
    return X.astype(rdt)


def capped(call):
    """-> [the arrays of call() without a cap, with slices of 2, with slices of 1]; the cap is 0 again afterwards."""
    lib = _lib.load()
    try:
        runs = []
        for cap in (0,) + CAPS:
            _lib.check(lib.ssq_host_slice_cap(cap))
            runs.append([np.array(a, copy=True) for a in call()])
    finally:
        _lib.check(lib.ssq_host_slice_cap(0))
    return runs


def assert_slices_change_nothing(call, what):
    whole, *sliced = capped(call)
    assert len(whole) > 0
    for cap, got in zip(CAPS, sliced):
        assert len(got) == len(whole)
        for k, (a, w) in enumerate(zip(got, whole)):
            assert a.dtype == w.dtype and a.shape == w.shape and w.shape[0] == B, (what, cap, k)
            assert np.array_equal(a, w, equal_nan=a.dtype.kind in "fc"), "%s: plane %d differs at a cap of %d" % (what, k, cap)


def test_signals_differ_and_move_targets():
    X = signals(np.float64)
    assert all(not np.array_equal(X[a], X[b]) for a in range(B) for b in range(a))
    targets = up.tmssq_stft(X, gwin(), n_fft=NFFT, hop_len=HOP, fs=FS, n_iter=1, get_targets=True)[4]
    frames = np.arange(targets.shape[-1])
    assert all(((targets[b] >= 0) & (targets[b] != frames)).any() for b in range(B))


@DTYPES
@pytest.mark.parametrize("name,order", STFT_RUNS, ids=STFT_IDS)
def test_stft_family(name, order, rdt):
    """ssq_stft2; mssq_stft orders 1 and 2, n_iter 3; tssq_stft orders 1 and 2; reassign_stft: every optional output."""
    X = signals(rdt)
    assert_slices_change_nothing(lambda: stft_host(name, order, X, "reflect"), name)


@DTYPES
def test_tmssq_stft(rdt):
    X = signals(rdt)

    def call():
        out = up.tmssq_stft(X, gwin(), n_fft=NFFT, hop_len=HOP, fs=FS, order=2, n_iter=2, get_tau=True, get_targets=True)
        return [out[0], out[1], out[4], out[5]]
    assert_slices_change_nothing(call, "tmssq_stft")


@pytest.mark.parametrize("cdt", [np.complex128, np.complex64], ids=["c128", "c64"])
def test_batched_inverses(cdt, monkeypatch):
    """`istft` on the fused kernel (its host path slices; the switch holds this small shape on it), and the row sums of
    `issq_stft` and `issq_cwt`."""
    rng = np.random.default_rng(11)
    nfr = (N_ST - 1) // HOP + 1
    monkeypatch.setenv("SSQ_ISTFT_FUSED", "1")
    fused = C.c_int(-1)
    _lib.load().ssq_istft_batch_workspace_bytes(_lib.SSQ_F64, B, nfr, NFFT, HOP, N_ST, C.byref(fused))
    assert fused.value == 1
    S = (rng.standard_normal((B, NFFT // 2 + 1, nfr)) + 1j * rng.standard_normal((B, NFFT // 2 + 1, nfr))).astype(cdt)
    T = (rng.standard_normal((B, NFFT // 2 + 1, N_ST)) + 1j * rng.standard_normal((B, NFFT // 2 + 1, N_ST))).astype(cdt)
    win = gwin()
    assert_slices_change_nothing(lambda: [up.istft(S, win, n_fft=NFFT, hop_len=HOP, N=N_ST)], "istft")
    assert_slices_change_nothing(lambda: [up.issq_stft(T, win, n_fft=NFFT)], "issq_stft")
    assert_slices_change_nothing(lambda: [up.issq_cwt(T, "gmw")], "issq_cwt")


@DTYPES
def test_cwt_map_family_takes_the_batch_whole(rdt):
    """ssq_cwt2, reassign_cwt, tssq_cwt (orders 1 and 2), mssq_cwt and tmssq_cwt (order 2, n_iter 3), every optional output:
    their workspace is not linear in the signals and `work_limit_bytes` is defined for the whole batch, so their hosts do
    not slice and the cap must not touch them.  5 signals of 32 samples, 8 scales at 4 to the octave."""
    X = signals(rdt)
    for (name, order), what in zip(CWT_RUNS, CWT_IDS):
        assert_slices_change_nothing(lambda: cwt_host(name, order, X, 8, 4), what)
    kw = dict(scales=cwt_scales(8, 4), fs=FS, order=2, n_iter=3)

    def mssq():
        out = up.mssq_cwt(X, GMW, get_w=True, get_rows=True, get_bins=True, **kw)
        return [out[0], out[1], out[4], out[5], out[6]]

    def tmssq():
        out = up.tmssq_cwt(X, GMW, get_tau=True, get_targets=True, **kw)
        return [out[0], out[1], out[4], out[5]]
    assert_slices_change_nothing(mssq, "mssq_cwt")
    assert_slices_change_nothing(tmssq, "tmssq_cwt")


# ---- ConceFT: 2 tapers / orders, 3 draws, every optional output ----
CF_J, CF_M, CF_SEED = 2, 3, 2
CF_NA, CF_NV = 8, 4


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _code(rdt):
    return _lib.SSQ_F32 if rdt == np.float32 else _lib.SSQ_F64


def _cdt(rdt):
    return np.complex64 if rdt == np.float32 else np.complex128


def conceft_stft_call(X):
    out = up.conceft_stft(X, up.hermite_windows(NFFT, CF_J), n_fft=NFFT, hop_len=HOP, fs=FS, n_draws=CF_M, seed=CF_SEED,
                          get_planes=True, get_w=True)
    return [out[0], out[3], out[4], out[5]]


def conceft_cwt_call(X):
    out = up.conceft_cwt(X, GMW, scales=cwt_scales(CF_NA, CF_NV), orders=CF_J, n_draws=CF_M, seed=CF_SEED, fs=FS,
                         get_Wx=True, get_w=True)
    return [out[0], out[3], out[4]]


@DTYPES
def test_conceft_stft(rdt):
    """5 signals of 32 samples, n_fft 16, hop 8, 2 Hermite tapers, 3 draws: Tx, the planes Sx and dSx, and w."""
    X = signals(rdt)
    assert_slices_change_nothing(lambda: conceft_stft_call(X), "conceft_stft")


@DTYPES
def test_conceft_cwt(rdt):
    """The same signals, 8 scales at 4 to the octave, 2 orders, 3 draws: Tx, the planes Wx, and w."""
    X = signals(rdt)
    assert_slices_change_nothing(lambda: conceft_cwt_call(X), "conceft_cwt")


def under_a_cap_of_two(call):
    lib = _lib.load()
    try:
        _lib.check(lib.ssq_host_slice_cap(2))
        return call()
    finally:
        _lib.check(lib.ssq_host_slice_cap(0))


CF_N_LONG = 600            # at hop 1: 600 frames, more than two store tiles of 256 frames at n_fft 16


def long_signals(rdt):
    """[5, 600]: five different base signals, each with an impulse six times its largest sample at another place."""
    X = base_signals(CF_N_LONG)[:B].copy()
    for b, at in enumerate((5, 131, 257, 300, 590)):
        X[b, at] += 6.0 * np.abs(X[b]).max()
    return X.astype(rdt)


@DTYPES
def test_conceft_stft_least_workspace_under_a_cap(rdt):
    """`ssq_conceft_stft_host` with work_limit_bytes = min_bytes under a cap of 2 against the uncapped default call, on 5
    signals of 600 samples at hop 1.  min_bytes is one store tile (256 frames at n_fft 16) of ONE signal and a signal has
    600 frames, so under host slices of 2, 2, 1 signals the inner slices are one signal wide and 256, 256, 88 frames long:
    the offsets of Tx, Sx, dSx and w of a second inner slice and of a later frame run, under a host slice after the
    first."""
    lib = _lib.load()
    X = long_signals(rdt)
    assert all(not np.array_equal(X[a], X[b]) for a in range(B) for b in range(a))
    N, hop = CF_N_LONG, 1
    tapers = up.hermite_windows(NFFT, CF_J)
    out = up.conceft_stft(X, tapers, n_fft=NFFT, hop_len=hop, fs=FS, n_draws=CF_M, seed=CF_SEED, get_planes=True, get_w=True)
    ref = [out[0], out[3], out[4], out[5]]
    wins = np.ascontiguousarray(tapers)
    adm = wins[:, NFFT // 2].copy()
    r, c = up._conceft_gauge(up._conceft_draws(CF_M, CF_J, CF_SEED), adm)      # what `conceft_stft` hands the library
    F, nfr = NFFT // 2 + 1, (N - 1) // hop + 1
    mn = C.c_int64(0)
    assert lib.ssq_conceft_stft_workspace_bytes(_code(rdt), B, N, NFFT, hop, CF_J, C.byref(mn)) > 0
    csz = np.dtype(_cdt(rdt)).itemsize
    wid = 8 * N if rdt == np.float32 else 0
    tile = 4096 // NFFT
    assert nfr > 2 * tile and mn.value == wid + 2 * CF_J * F * tile * csz        # one tile of one signal: less than a signal
    got = [np.empty((B, F, nfr), _cdt(rdt)), np.empty((B, CF_J, F, nfr), _cdt(rdt)), np.empty((B, CF_J, F, nfr), _cdt(rdt)),
           np.empty((B, CF_M, F, nfr), rdt)]
    freqs = np.empty(F)
    under_a_cap_of_two(lambda: _lib.check(lib.ssq_conceft_stft_host(
        _code(rdt), _vp(X), B, N, _vp(wins), CF_J, NFFT, hop, FS, up.PAD_MODES["reflect"], _vp(r), CF_M,
        float(adm[0] / c.sum()), -1.0, up._variant(True), mn.value, _vp(got[0]), _vp(freqs), _vp(got[1]), _vp(got[2]),
        _vp(got[3]))))
    for k, (a, w) in enumerate(zip(got, ref)):
        assert a.dtype == w.dtype and a.shape == w.shape and w.shape[0] == B and np.array_equal(a, w, equal_nan=True), k


@DTYPES
def test_conceft_cwt_least_workspace_under_a_cap(rdt):
    """`ssq_conceft_cwt_host` with work_limit_bytes = min_bytes (the planes of ONE signal) under a cap of 2: host slices
    of 2, 2, 1 signals, each walked in inner slices of 1, against the uncapped default call."""
    lib = _lib.load()
    X = signals(rdt)
    ref = conceft_cwt_call(X)
    s, rowc, f, kind, f_idx = cwt_grids(CF_NA, CF_NV, N_ST)
    _, p0, p1 = up._wavelet(GMW)
    adm = np.array([up.gmw_adm_ssq(p0, p1, k) for k in range(CF_J)])
    r, c = up._conceft_gauge(up._conceft_draws(CF_M, CF_J, CF_SEED), adm)      # what `conceft_cwt` hands the library
    polys = np.ascontiguousarray(up.gmw_order_coefficients(p0, p1, range(CF_J), average=False))
    mn = C.c_int64(0)
    pref = int(lib.ssq_conceft_cwt_workspace_bytes(_code(rdt), B, N_ST, CF_NA, CF_J, C.byref(mn)))
    assert 0 < mn.value and pref == B * mn.value
    got = [np.empty((B, CF_NA, N_ST), _cdt(rdt)), np.empty((B, CF_J, CF_NA, N_ST), _cdt(rdt)),
           np.empty((B, CF_M, CF_NA, N_ST), rdt)]
    under_a_cap_of_two(lambda: _lib.check(lib.ssq_conceft_cwt_host(
        _code(rdt), _vp(X), B, N_ST, p0, p1, _vp(polys), polys.shape[1], CF_J, _vp(r), CF_M,
        float(adm[0] / c.sum()), _vp(s), CF_NA, 1 / FS, _vp(rowc), _vp(f), up.FREQS[kind], f_idx or 0,
        up.PAD_MODES["reflect"], -1.0, up.VARIANT_FLIPUD, mn.value, _vp(got[0]), _vp(got[1]), _vp(got[2]))))
    for k, (a, w) in enumerate(zip(got, ref)):
        assert a.dtype == w.dtype and a.shape == w.shape and np.array_equal(a, w, equal_nan=True), k


def test_walk_hosts():
    """msst_walk, tmsst_walk, mssq_cwt_walk and tmssq_cwt_walk on [5, 9, 4] maps.  The two STFT walks repack every slice on
    the host and keep a loop of their own; the two CWT walks repack nothing and go through `host_sliced`."""
    rng = np.random.default_rng(12)
    R, n = NFFT // 2 + 1, (N_ST - 1) // HOP + 1
    bins = rng.integers(-1, R, size=(B, R, n)).astype(np.int32)
    assert_slices_change_nothing(lambda: [up.msst_walk(bins, 3)], "msst_walk")
    step = rng.integers(-1, 2, size=(B, R, n))
    targets = np.where(rng.random((B, R, n)) < 0.25, -1, np.clip(np.arange(n) + step, 0, n - 1)).astype(np.int32)
    assert_slices_change_nothing(lambda: [up.tmsst_walk(targets, 3, 1)], "tmsst_walk")
    anywhere = rng.integers(-1, n, size=(B, R, n)).astype(np.int32)
    assert_slices_change_nothing(lambda: [up.tmssq_cwt_walk(anywhere, 3)], "tmssq_cwt_walk")
    f = 0.5 * 2.0 ** ((np.arange(R) - (R - 1)) / 16)                       # an ascending log grid
    w = np.where(bins >= 0, f[np.maximum(bins, 0)], np.inf)
    rho = rng.permutation(R)
    assert_slices_change_nothing(lambda: list(up.mssq_cwt_walk(w, f, rho, 3)), "mssq_cwt_walk")
