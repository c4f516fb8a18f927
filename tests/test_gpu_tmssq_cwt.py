"""GPU tests of the time-reassigned multisynchrosqueezed CWT, `upstream.tmssq_cwt` (csrc/cwt_tmsst.hip), on
the cases, the signal and the derived bounds of tests/test_gpu_tssq_cwt.py (imported, not copied).

Everything up to the one-step target is `tssq_cwt`'s, and that file checks it against the model; here `Wx` and `tau` are
`np.array_equal` to `tssq_cwt`'s.  The walk is integer-exact: `mm` is `np.array_equal` to the walk by the definition
(tests/helpers/tmsst_ref.walk) of the one-step targets recomputed from the call's own `tau`.  `Tx` is the scatter of the
call's own `Wx` under the call's own `mm`: every part of every cell inside DESIGN 4.16's derived bound
c q / 2 + 4 eps64 M + eps_out |T| (`scatter_check`), which does not depend on where the targets came from."""
import ctypes as C
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.helpers import cwt_sst2_ref as c2
from tests.helpers import tmssq_cwt_ref as m
from tests.helpers import tssq_cwt_ref as m1
from tests.helpers.reassign_cwt_ref import time_targets
from tests.helpers.tmsst_ref import walk
from tests.helpers.tsst_ref import impulses
from tests.test_gpu_tssq_cwt import CASES as CASES1
from tests.test_gpu_tssq_cwt import FS, GMW, IDS as IDS1, MORLET, _log, _vp, scatter_check, signal, strong

pytestmark = pytest.mark.gpu

T, HALO = up.tmssq_cwt_tile_cols()
# the five shapes of tests/test_gpu_tssq_cwt.py, and one for the tile walk: three whole tiles and a partial one
CASES = list(CASES1) + [(3 * T + 37, lambda: _log(GMW, 12, 2), GMW, "reflect")]
IDS = list(IDS1) + ["3T+37-log12-gmw-reflect"]
N_ITER = [4, 3, 7, 64, 2, 4]
RUNS = list(range(len(CASES)))
ORDERS = [1, 2]
RDTS = [np.float64, np.float32]
RDT_IDS = ["f64", "f32"]


@functools.lru_cache(maxsize=None)
def gpu(i, order, rdt, n_iter=None):
    """(Tx, Wx, scales, row_freqs, tau, mm) of `tmssq_cwt` on case i at the case's n_iter; computed once, read-only."""
    N, sc, wavelet, pad = CASES[i]
    out = up.tmssq_cwt(signal(N, i).astype(rdt), wavelet, scales=sc(), fs=FS, padtype=pad, order=order,
                       n_iter=N_ITER[i] if n_iter is None else n_iter, get_tau=True, get_targets=True)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gpu_one_step(i, order, rdt):
    """The same of `tssq_cwt`."""
    N, sc, wavelet, pad = CASES[i]
    out = up.tssq_cwt(signal(N, i).astype(rdt), wavelet, scales=sc(), fs=FS, padtype=pad, order=order, get_tau=True,
                      get_targets=True)
    for a in out:
        a.setflags(write=False)
    return out


def one_step_targets(tau):
    """The one-step targets recomputed from a reported tau in its own dtype, -1 where the bin is not kept."""
    return np.where(np.isposinf(tau), -1, time_targets(tau, 1 / FS))


def far_steps(t1, n_iter):
    """(the longest step of any chain, first step included; the walked steps whose column lay outside the stage of the
    tile the chain started in: the reads the kernel takes from device memory) of the walk of t1 [na, N]."""
    N = t1.shape[-1]
    j = np.arange(N)[None, :]
    lo = j // T * T - HALO
    hi = np.minimum(j // T * T + T, N) + HALO
    longest = int(np.abs(t1 - j)[t1 >= 0].max()) if (t1 >= 0).any() else 0
    far = 0
    c, live = t1.copy(), t1 >= 0
    for _ in range(n_iter - 1):
        nxt = np.take_along_axis(t1, np.maximum(c, 0), axis=-1)
        far += int((live & ((c < lo) | (c >= hi))).sum())
        live = live & (nxt >= 0) & (nxt != c)
        if live.any():
            longest = max(longest, int(np.abs(nxt - c)[live].max()))
        c = np.where(live, nxt, c)
    return longest, far


@pytest.mark.parametrize("rdt", RDTS, ids=RDT_IDS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("i", RUNS, ids=IDS)
def test_wx_and_tau_are_tssq_cwts_and_mm_is_the_walk(i, order, rdt):
    N, sc, wavelet, pad = CASES[i]
    Tx, Wx, scales, row_freqs, tau, mm = gpu(i, order, rdt)
    Tx1, Wx1, scales1, row_freqs1, tau1, mm1 = gpu_one_step(i, order, rdt)
    assert Tx.shape == Wx.shape == tau.shape == mm.shape == (len(sc()), N)
    assert Tx.dtype == Wx.dtype == Wx1.dtype and tau.dtype == rdt and mm.dtype == np.int32
    assert np.array_equal(Wx, Wx1) and np.array_equal(tau, tau1, equal_nan=True)
    assert np.array_equal(scales, scales1) and np.array_equal(row_freqs, row_freqs1)
    t1 = one_step_targets(tau)
    assert np.array_equal(t1, mm1)
    assert np.array_equal(mm, walk(t1, N_ITER[i]))
    assert np.array_equal(mm == -1, np.isposinf(tau))
    longest, far = far_steps(t1, N_ITER[i])
    print("N %d n_iter %d: longest step %d columns (halo %d), %d walked steps read outside the stage, %d bins moved on"
          % (N, N_ITER[i], longest, HALO, far, (mm != mm1).sum()))
    if i != 1:                                                  # (40-morlet: the row is shorter than the halo)
        assert longest > HALO
    if N > T + HALO:
        assert far > 0                                          # the read of the plane in device memory, in a real call
    assert (mm != mm1).any()


@pytest.mark.parametrize("rdt", RDTS, ids=RDT_IDS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("i", RUNS, ids=IDS)
def test_one_step_is_tssq_cwt_bit_for_bit(i, order, rdt):
    N, sc, wavelet, pad = CASES[i]
    ref = gpu_one_step(i, order, rdt)
    got = gpu(i, order, rdt, 1)
    for k in range(6):
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
    bare = up.tmssq_cwt(signal(N, i).astype(rdt), wavelet, scales=sc(), fs=FS, padtype=pad, order=order, n_iter=1)
    assert len(bare) == 4 and np.array_equal(bare[0], ref[0]) and np.array_equal(bare[1], ref[1])


@pytest.mark.parametrize("rdt", RDTS, ids=RDT_IDS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("i", RUNS, ids=IDS)
def test_tx_is_the_scatter_of_the_calls_own_maps(i, order, rdt):
    """Every part of every cell within DESIGN 4.16's derived bound, the marginal identity of every row within the cell
    bounds summed over the row, and a cell without a contribution exactly 0.  Measured on an MI355X: see DESIGN 4.22."""
    N, sc, wavelet, pad = CASES[i]
    Tx, Wx, _, _, tau, mm = gpu(i, order, rdt)
    worst, row, clean = scatter_check(Tx, Wx, mm, up.tssq_cwt_row_freqs(wavelet, sc()))
    print("worst cell: %.3g of its bound; marginal identity, worst row: %.3g of the summed bound" % (worst, row))
    assert clean
    assert worst <= 1 and row <= 1
    # without the targets asked for the walked plane lives in the workspace: the same Tx
    bare = up.tmssq_cwt(signal(N, i).astype(rdt), wavelet, scales=sc(), fs=FS, padtype=pad, order=order, n_iter=N_ITER[i])
    assert len(bare) == 4 and np.array_equal(bare[0], Tx) and np.array_equal(bare[1], Wx)


@pytest.mark.parametrize("rdt", RDTS, ids=RDT_IDS)
@pytest.mark.parametrize("order", ORDERS)
def test_isolated_impulse(order, rdt):
    """tests/test_gpu_tssq_cwt.py's impulse (padtype='zero'): every strong bin names the impulse's column after one step, and
    that column is a fixed point, so it does at n_iter 4 and 64 too."""
    from tests.test_tssq_cwt_ref import FIT, N, SCALES, T0, column_share
    x = impulses(N, [T0]).astype(rdt)
    nu = up.tssq_cwt_row_freqs(GMW, SCALES[:FIT])
    for n_iter in (1, 4, 64):
        Tx, Wx, _, _, tau, mm = up.tmssq_cwt(x, GMW, scales=SCALES[:FIT], padtype="zero", order=order, n_iter=n_iter,
                                             get_tau=True, get_targets=True)
        big = strong(Wx)
        assert big.sum() > 5000 and (mm[big] == T0).all(), n_iter
        worst, row, clean = scatter_check(Tx, Wx, mm, nu)
        print("n_iter %d: column %d holds %.6f of the energy of Tx; worst cell %.3g of its bound"
              % (n_iter, T0, column_share(Tx, T0), worst))
        assert worst <= 1 and row <= 1 and clean
        assert column_share(Tx, T0) > 0.99


@functools.lru_cache(maxsize=None)
def table_lib_tables():
    """(T0, T1) [na, P] of DESIGN 4.22's scales as the library evaluates them on the host (`ssq_ssq_cwt2_tables`)."""
    scales, P = m.table_scales(("gmw", 3.0, 60.0)), c2.p2up(1024)[0]
    code, p0, p1 = up._wavelet(GMW)
    T0, T1 = np.zeros((len(scales), P)), np.zeros((len(scales), P))
    for r, a in enumerate(scales):
        _lib.check(_lib.load().ssq_ssq_cwt2_tables(code, p0, p1, float(a), P, _vp(T0[r]), _vp(T1[r])))
    return T0, T1


@pytest.mark.parametrize("n_iter", [1, 4])
def test_concentration_matches_the_model(n_iter):
    """DESIGN 4.22's table, fp64, order 2: the share of the GPU's Tx equals the model's on the library's own tables within
    10 x the difference between the model's 'fft' and 'dft' arithmetics on that share.  Measured: see DESIGN 4.22."""
    wv = ("gmw", 3.0, 60.0)
    sc = m.table_scales(wv)
    nu = m1.row_freqs(wv, sc)
    x, _ = m.delay_signal(1024, 512.0, 150.0, 4)
    share = {a: m.top_cell_share(m.tmssq_cwt_ref(x, wv, sc, order=2, n_iter=n_iter, arith=a, tabs=table_lib_tables())[3], nu)
             for a in ("fft", "dft")}
    Tx = up.tmssq_cwt(x, GMW, scales=sc, order=2, n_iter=n_iter)[0]
    got = m.top_cell_share(Tx, nu)
    tol = 10 * abs(share["fft"] - share["dft"])
    print("n_iter %d: GPU %.12f  model fft %.12f  dft %.12f  |GPU - fft| %.3g  tolerance %.3g"
          % (n_iter, got, share["fft"], share["dft"], abs(got - share["fft"]), tol))
    assert abs(got - share["fft"]) <= tol


@pytest.mark.parametrize("rdt", RDTS, ids=RDT_IDS)
@pytest.mark.parametrize("order", ORDERS)
def test_batch_equals_single_calls_and_is_deterministic(order, rdt):
    X = np.stack([signal(300, sd) * a for sd, a in ((11, 1.0), (12, 300.0), (13, 1e-4))]).astype(rdt)   # three scales A
    kw = dict(scales=_log(GMW, 37, 8), fs=FS, order=order, n_iter=4, get_tau=True, get_targets=True)
    B = up.tmssq_cwt(X, GMW, **kw)
    assert B[0].shape == B[1].shape == B[4].shape == B[5].shape == (3, 37, 300)
    for b in range(3):
        one = up.tmssq_cwt(X[b], GMW, **kw)
        for k in range(6):
            assert np.array_equal(B[k][b] if k not in (2, 3) else B[k], one[k]), (b, k)
    again = up.tmssq_cwt(X, GMW, **kw)
    for k in range(6):
        assert np.array_equal(B[k], again[k]), k


@pytest.mark.parametrize("rdt", RDTS, ids=RDT_IDS)
@pytest.mark.parametrize("order", ORDERS)
def test_chunking_does_not_change_a_bit(order, rdt):
    """`work_limit_bytes` for 16 rows per chunk (the 2 x 37 rows go as 16 + 16 + 16 + 16 + 10), then one row per chunk;
    the walk runs after all chunks."""
    lib = _lib.load()
    B, N, na = 2, 300, 37
    code = _lib.SSQ_F32 if rdt == np.float32 else _lib.SSQ_F64
    X = np.stack([signal(N, sd) for sd in (21, 22)]).astype(rdt)
    kw = dict(scales=_log(GMW, na, 8), fs=FS, order=order, n_iter=4, get_tau=True, get_targets=True)
    mn = C.c_int64(0)
    assert lib.ssq_tmssq_cwt_workspace_bytes(code, B, N, na, order, C.byref(mn)) > 0
    P, M = c2.p2up(N)[0], 2 if order == 1 else 5
    ref = up.tmssq_cwt(X, GMW, **kw)
    for limit in (mn.value + 15 * 32 * M * P, mn.value):
        out = up.tmssq_cwt(X, GMW, work_limit_bytes=limit, **kw)
        for k in range(6):
            assert np.array_equal(ref[k], out[k]), (limit, k)


@pytest.mark.parametrize("rdt", RDTS, ids=RDT_IDS)
def test_degenerate_inputs(rdt):
    sc = _log(GMW, 20, 4)
    nu = up.tssq_cwt_row_freqs(GMW, sc)
    kw = dict(scales=sc, n_iter=4, get_tau=True, get_targets=True)
    Tx, Wx, _, _, tau, mm = up.tmssq_cwt(np.zeros(200, dtype=rdt), GMW, **kw)
    assert not Tx.any() and not Wx.any() and np.isposinf(tau).all() and (mm == -1).all()
    Tx, Wx, _, _, tau, mm = up.tmssq_cwt(np.full(200, 3.0, dtype=rdt), GMW, **kw)
    assert np.isfinite(Tx.view(rdt)).all() and not np.isnan(tau).any()
    assert np.array_equal(mm, walk(one_step_targets_dt1(tau), 4))
    worst, row, clean = scatter_check(Tx, Wx, mm, nu)
    assert worst <= 1 and row <= 1 and clean
    # N = 2, na = 2: P = 4, the two scales whose peaks sit on its bins 2 and 1
    sc2 = _log(GMW, 2, 1)
    Tx, Wx, _, _, tau, mm = up.tmssq_cwt(np.array([3.0, -1.0], dtype=rdt), GMW, scales=sc2, padtype="zero", n_iter=4,
                                         get_tau=True, get_targets=True)
    assert Tx.shape == (2, 2) and np.isfinite(Tx.view(rdt)).all() and Tx.any() and (mm >= 0).all() and (mm < 2).all()
    assert np.array_equal(mm, walk(one_step_targets_dt1(tau), 4))
    worst, row, clean = scatter_check(Tx, Wx, mm, up.tssq_cwt_row_freqs(GMW, sc2))
    assert worst <= 1 and row <= 1 and clean
    Tx, Wx, _, _, tau, mm = up.tmssq_cwt(signal(200, 2).astype(rdt), GMW, gamma=1e6, **kw)
    assert np.abs(Wx).max() < 1e6 and not Tx.any() and np.isposinf(tau).all() and (mm == -1).all()


def one_step_targets_dt1(tau):
    """`one_step_targets` of a call without `fs` (dt = 1)."""
    return np.where(np.isposinf(tau), -1, time_targets(tau, 1.0))
