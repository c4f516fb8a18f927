"""GPU tests of the time-reassigned multisynchrosqueezed STFT, `upstream.tmssq_stft` and `upstream.tmsst_walk`
(csrc/stft_tmsst.hip), against the numpy model tests/helpers/tmsst_ref.py.

The operator is `tssq_stft`'s: Sx and tau are held bitwise to that call (whose parity with the model
tests/test_gpu_tsst.py holds), not re-derived.  The walk is integer work and is compared exactly.  The scatter is held
as `tssq_stft`'s is: against the extended-precision ascending-source sum of the call's own Sx under the call's own
targets, within 8 eps sum|Sx| of a cell's contributions, eps of the call's dtype."""
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import upstream as up
from tests.helpers import tmsst_ref as m
from tests.helpers import tsst_ref as m1
from tests.test_gpu_tsst import FS, signal, window

pytestmark = pytest.mark.gpu

# (N, n_fft, hop, padtype, n_iter, extra keywords): one lane per frame, reach 4 H = 32; a hop that does not divide n;
# modulated=False, reach 512 (the widest of the 8192-target stage's 1024-frame tiles); multi-wave frames at the largest
# n_iter, reach 1024; a signal shorter than the window (every target clamped); R = 16384, the largest reach: two tiles of
# 4096 targets, each staged with all of the other (order 2 only)
CASES = [
    (1500, 16, 1, "reflect", 4, dict()),
    (3000, 64, 3, "zero", 7, dict()),
    (4000, 256, 1, "symmetric", 4, dict(modulated=False)),
    (9000, 2048, 64, "replicate", 64, dict()),
    (40, 64, 1, "zero", 3, dict()),
    (6000, 4096, 1, "reflect", 8, dict()),
]
RUNS = [(i, order) for i in range(len(CASES)) for order in (1, 2) if not (i == len(CASES) - 1 and order == 1)]
IDS = ["%d-%d-%d-%s-it%d-o%d" % (CASES[i][:5] + (order,)) for i, order in RUNS]
DTYPES = pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])


def call_kw(i, order):
    N, n, hop, pad, n_iter, kw = CASES[i]
    return dict(n_fft=n, hop_len=hop, fs=FS, padtype=pad, order=order, **kw)


@functools.lru_cache(maxsize=None)
def gpu(i, order, rdt):
    """(Tx, Sx, times, Sfs, tau, targets) of case i; computed once, read-only."""
    N, n, hop, pad, n_iter, kw = CASES[i]
    out = up.tmssq_stft(signal(N, i).astype(rdt), window(n), n_iter=n_iter, get_tau=True, get_targets=True, **call_kw(i, order))
    for a in out:
        a.setflags(write=False)
    return out


@DTYPES
@pytest.mark.parametrize("i,order", RUNS, ids=IDS)
def test_operator_and_one_step_are_tssq_stft(i, order, rdt):
    """Sx, tau and the times / frequencies are `tssq_stft`'s bit for bit at any n_iter, and so is Tx at n_iter = 1 (with
    and without `targets`: the walk launch is skipped or writes the one-step map)."""
    N, n, hop, pad, n_iter, kw = CASES[i]
    x = signal(N, i).astype(rdt)
    Tx, Sx, times, Sfs, tau, tgt = gpu(i, order, rdt)
    T1, S1, t1, f1, tau1 = up.tssq_stft(x, window(n), get_tau=True, **call_kw(i, order))
    assert Tx.shape == Sx.shape == tau.shape == tgt.shape == (n // 2 + 1, (N - 1) // hop + 1)
    assert Tx.dtype == Sx.dtype == T1.dtype and tau.dtype == times.dtype == Sfs.dtype == rdt and tgt.dtype == np.int32
    assert np.array_equal(Sx, S1) and np.array_equal(tau, tau1)
    assert np.array_equal(times, t1) and np.array_equal(Sfs, f1)
    one = up.tmssq_stft(x, window(n), n_iter=1, **call_kw(i, order))
    assert len(one) == 4 and np.array_equal(one[0], T1) and np.array_equal(one[1], S1)
    del one
    one = up.tmssq_stft(x, window(n), n_iter=1, get_targets=True, **call_kw(i, order))
    assert np.array_equal(one[0], T1)
    keep = ~np.isposinf(tau1)
    assert np.array_equal(one[4], np.where(keep, m1.targets(tau1, hop, FS)[0], -1))


@DTYPES
@pytest.mark.parametrize("i,order", RUNS, ids=IDS)
def test_targets_are_the_models_walk_of_the_calls_own_map(i, order, rdt):
    """Integers, no tolerance: the one-step targets recomputed from the call's own tau by the rule in its dtype, walked by
    the model."""
    N, n, hop, pad, n_iter, kw = CASES[i]
    Tx, Sx, _, _, tau, tgt = gpu(i, order, rdt)
    keep = ~np.isposinf(tau)
    t1 = np.where(keep, m1.targets(tau, hop, FS)[0], -1)
    want = m.walk(t1, n_iter)
    moved = np.abs(want - np.arange(want.shape[1]))[keep]
    H = (n // 2 - 1) // hop + 1
    print("kept %d of %d bins; largest displacement %d frames (H = %d, n_iter H = %d); %d bins moved past H"
          % (keep.sum(), keep.size, moved.max(initial=0), H, n_iter * H, (moved > H).sum()))
    assert np.array_equal(tgt, want)
    assert moved.max(initial=0) <= n_iter * H


@DTYPES
@pytest.mark.parametrize("i,order", RUNS, ids=IDS)
def test_tx_is_the_scatter_of_the_calls_own_targets(i, order, rdt):
    """Tx == the ascending-source scatter of the call's own Sx, with the rotation by the total displacement, under the
    call's own targets, within 8 eps sum|Sx| of every cell's contributions; and the marginal identity per row within
    16 eps sum_m |Sx[k, m]|.  Measured on an MI355X: worst cell 0.26 ... 0.48 of its tolerance in fp64 and 0.056 ... 0.063 in
    fp32 (the figures of `tssq_stft`'s own test: the reach adds nothing, 0.48 / 0.062 at R = 16384); marginal identity,
    worst row 0.007 ... 0.16 (fp64) and 0.001 ... 0.026 (fp32) of its tolerance."""
    N, n, hop, pad, n_iter, kw = CASES[i]
    Tx, Sx, _, _, tau, tgt = gpu(i, order, rdt)
    keep = tgt >= 0
    assert np.array_equal(keep, ~np.isposinf(tau))
    to = np.maximum(tgt, 0).astype(np.int64)
    ref = m1.scatter(Sx, to, keep, hop, n, acc=np.longdouble)
    kk, mm = np.nonzero(keep)
    load = np.zeros(Sx.shape)
    np.add.at(load, (kk, to[kk, mm]), np.abs(Sx[kk, mm]).astype(np.float64))
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


@pytest.mark.parametrize("n_iter", [1, 4, 64])
@pytest.mark.parametrize("order", [1, 2])
@DTYPES
def test_isolated_impulse(rdt, order, n_iter):
    """Every kept bin of an impulse names the impulse's own column, a fixed point of the map, at any n_iter, and the
    column holds sum(g) in every row."""
    N, n, t0 = 700, 128, 333
    win = window(n)
    Tx, Sx, _, _, tgt = up.tmssq_stft(m1.impulses(N, [t0]).astype(rdt), win, n_fft=n, order=order, n_iter=n_iter,
                                      get_targets=True)
    keep = tgt >= 0
    assert keep.sum() >= 65 * 100 and (tgt[keep] == t0).all()
    rel = np.abs(np.abs(Tx[:, t0]) / win.sum() - 1).max()
    print("column %d: |Tx| / sum(g) - 1 <= %.3g" % (t0, rel))
    assert rel <= 1e-6
    assert not np.delete(Tx, t0, axis=1).any()


def test_concentration_matches_the_model():
    """The signal of DESIGN 4.21's table at order 2, n_iter 4: the model's share (0.9729) to four digits."""
    from tests.test_tmsst_ref import N, NFFT, TABLE, table_share, table_window
    x, _ = m.delay_signal(N)
    sg = m.top_cell_share(up.tmssq_stft(x, table_window(), n_fft=NFFT, order=2, n_iter=4)[0])
    sm = table_share(2, 4)
    print("order 2, n_iter 4: GPU %.6f, model %.6f" % (sg, sm))
    assert abs(sg - sm) < 5e-5 and abs(sg - TABLE[2][4]) < 5e-5


@DTYPES
@pytest.mark.parametrize("i", [0, 3], ids=["1500-16-1", "9000-2048-64"])
def test_batch_equals_single_calls_and_is_deterministic(rdt, i):
    N, n, hop, pad, n_iter, kw = CASES[i]
    X = np.stack([signal(N, s) for s in (11, 12, 13, 14, 15)]).astype(rdt)
    win = window(n)
    for order in (1, 2):
        kw = dict(n_iter=n_iter, get_tau=True, get_targets=True, **call_kw(i, order))
        B = up.tmssq_stft(X, win, **kw)
        assert B[0].shape == (5, n // 2 + 1, (N - 1) // hop + 1)
        for b in range(5):
            one = up.tmssq_stft(X[b], win, **kw)
            for k in (0, 1, 4, 5):
                assert np.array_equal(B[k][b], one[k]), (order, b, k)
        again = up.tmssq_stft(X, win, **kw)
        for k in (0, 1, 4, 5):
            assert np.array_equal(B[k], again[k]), (order, k)


@pytest.mark.parametrize("order", [1, 2])
@DTYPES
def test_degenerate_inputs(rdt, order):
    N, n = 500, 64
    win = window(n)
    kw = dict(n_fft=n, order=order, n_iter=5, get_tau=True, get_targets=True)
    Tx, Sx, _, _, tau, tgt = up.tmssq_stft(np.zeros(N, dtype=rdt), win, hop_len=3, **kw)
    assert not Tx.any() and not Sx.any() and np.isposinf(tau).all() and (tgt == -1).all()
    Tx, Sx, _, _, tau, tgt = up.tmssq_stft(np.full(N, 3.0, dtype=rdt), win, hop_len=3, **kw)
    assert np.isfinite(Tx.view(rdt)).all() and Tx.any() and tgt.max() < Tx.shape[1]
    Tx, Sx, times, _, tau, tgt = up.tmssq_stft(np.full(1, 3.0, dtype=rdt), win, **kw)
    assert Tx.shape == (n // 2 + 1, 1) and times.shape == (1,) and np.isfinite(Tx.view(rdt)).all()
    assert np.isin(tgt, (-1, 0)).all()
    x = signal(N, 2).astype(rdt)
    Tx, Sx, _, _, tau, tgt = up.tmssq_stft(x, win, hop_len=3, gamma=1e6, **kw)
    assert np.abs(Sx).max() < 1e6 and not Tx.any() and np.isposinf(tau).all() and (tgt == -1).all()


# ------------------------------------------------------------------------------------------------------ tmsst_walk ----
def hand_maps(n):
    """name -> (int32 map [n], reach) written by hand"""
    a = np.arange(n)
    shift = np.minimum(a + 1, n - 1)
    hole = shift.copy()
    hole[n // 2::97] = -1
    cyc = np.minimum(a ^ 1, n - 1)
    if n % 2:
        cyc[n - 1] = n - 1                                    # (an odd frame count: the last frame has no partner)
    return {"identity": (a, 1), "none": (np.full(n, -1), 1), "shift": (shift, 1), "cycle": (cyc, 1), "hole": (hole, 1)}


def random_map(shape, reach, seed):
    """Targets within +- reach of their own frame, inside the frames, a third of the entries -1."""
    rng = np.random.default_rng(seed)
    n = shape[-1]
    t = np.clip(np.arange(n) + rng.integers(-reach, reach + 1, size=shape), 0, n - 1)
    return np.where(rng.random(shape) < 1 / 3, -1, t).astype(np.int32)


def walk_sizes(reach, n_iter):
    """(frames, batch or None): one frame; a tile and a tail; three tiles and a tail with a batch of 3"""
    T = up.tmsst_tile_frames(reach, n_iter)
    return [(1, None), (T + 37, None), (3 * T + 129, 3)]


@pytest.mark.parametrize("n_iter", [1, 2, 7, 64])
def test_walk_of_maps_written_by_hand(n_iter):
    for n, B in walk_sizes(1, n_iter):
        for name, (t, reach) in hand_maps(n).items():
            rows = np.stack([t, np.arange(n), t]).astype(np.int32)                                 # [F = 3, n]
            tm = rows if B is None else np.stack([rows] * B)
            got = up.tmsst_walk(tm, n_iter, reach)
            assert got.dtype == np.int32 and got.shape == tm.shape
            assert np.array_equal(got, m.walk(tm, n_iter)), (name, n, B)
            if name == "shift":
                assert np.array_equal(got[..., 0, :], np.broadcast_to(np.minimum(np.arange(n) + n_iter, n - 1), got[..., 0, :].shape))


@pytest.mark.parametrize("reach,n_iter", [(1, 64), (37, 5), (511, 1), (300, 7), (2048, 8)],
                         ids=["r1-it64", "r37-it5", "r511-it1", "r300-it7", "r2048-it8"])
def test_walk_of_random_maps(reach, n_iter):
    """Seeded random maps: chains that cross tile edges in both directions, stop on holes, and (reach 300 x 7, 2048 x 8:
    the 36864-target stage) leave the one-window reach.  2048 x 8 is the largest reach, across two tiles."""
    T = up.tmsst_tile_frames(reach, n_iter)
    sizes = [(T + 2500, None)] if reach == 2048 else walk_sizes(reach, n_iter)
    for n, B in sizes:
        shape = (5, n) if B is None else (B, 5, n)
        t = random_map(shape, reach, seed=n + n_iter)
        got = up.tmsst_walk(t, n_iter, reach)
        want = m.walk(t, n_iter)
        far = np.abs(want - np.arange(n))[want >= 0].max(initial=0)
        print("n %d, batch %s, tile %d: largest displacement %d of %d" % (n, B, T, far, reach * n_iter))
        assert np.array_equal(got, want), (n, B)


# ------------------------------------------------------------------------------------------------ the device door ----
@DTYPES
def test_device_door_equals_the_host_call(rdt):
    """`ssq_tmssq_stft_exec` on buffers from `ssq_dev_malloc`, a workspace of exactly `ssq_tmssq_stft_workspace_bytes` and
    guards behind every buffer (tests/test_gpu_grid_limits.py's Door): Tx, Sx, tau and targets equal `tmssq_stft`'s bit
    for bit.  The family's smallest shape, 5 different signals with an impulse each (tests/test_gpu_host_slices.py)."""
    import ctypes as C

    from ssqueeze_rs_amd import _lib
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
    for order, n_iter in ((2, 2), (1, 3)):
        out = up.tmssq_stft(X, win, n_fft=NFFT, hop_len=HOP, fs=FS_ST, order=order, n_iter=n_iter, get_tau=True,
                            get_targets=True)
        host = [out[0], out[1], out[4], out[5]]
        ws = int(lib.ssq_tmssq_stft_workspace_bytes(code, B, N, NFFT, HOP, n_iter))
        assert ws > 0
        with Door() as d:
            dx, dws = d.buf(X.nbytes, X), d.buf(ws)
            dT, dS = d.buf(cells * np.dtype(cdt).itemsize), d.buf(cells * np.dtype(cdt).itemsize)
            dtau, dtg = d.buf(cells * np.dtype(rdt).itemsize), d.buf(cells * 4)
            _lib.check(lib.ssq_tmssq_stft_exec(code, dx.p, B, N, win.ctypes.data_as(C.c_void_p), NFFT, HOP, FS_ST,
                                               up.PAD_MODES["reflect"], order, -1.0, 3, n_iter, dT.p, dS.p, dtau.p, dtg.p,
                                               dws.p, ws, None))
            dev = [dT.get(shape, cdt), dS.get(shape, cdt), dtau.get(shape, rdt), dtg.get(shape, np.int32)]
        for name, a, h in zip(("Tx", "Sx", "tau", "targets"), dev, host):
            assert_same(a, np.ascontiguousarray(h), "order %d: device %s against the host call's" % (order, name))
