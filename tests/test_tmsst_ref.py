"""The numpy model of the time-reassigned multisynchrosqueezed STFT (tests/helpers/tmsst_ref.py) against the facts it is
built on: the walk on maps written by hand, n_iter = 1 is `tsst_ref`, the per-row marginal identity, and the
concentration table of DESIGN 4.21.  CPU only."""
import functools

import numpy as np
import pytest

from tests.helpers import tmsst_ref as m
from tests.helpers import tsst_ref as m1
from tests.test_gpu_tsst import signal, window

N, NFFT, SIGMA = 1024, 256, 10.0
# the share of the rows' energy in their largest cell, by order and n_iter
TABLE = {2: {1: 0.7225, 2: 0.9435, 4: 0.9729, 8: 0.9741, 32: 0.9744},
         1: {1: 0.1837, 2: 0.3132, 4: 0.5266, 8: 0.6313, 32: 0.6800}}


def table_window():
    return np.exp(-0.5 * ((np.arange(NFFT) - NFFT // 2) / SIGMA) ** 2)


@functools.lru_cache(maxsize=None)
def table_share(order, n_iter):
    x, _ = m.delay_signal(N)
    return m.top_cell_share(m.tmsst_ref(x, table_window(), NFFT, order=order, n_iter=n_iter)[3])


def test_walk_on_maps_written_by_hand():
    n = 9
    ident = np.arange(n)[None, :]
    none = np.full((2, n), -1)
    shift = np.minimum(np.arange(n) + 1, n - 1)[None, :]
    for it in (1, 2, 7, 64):
        assert np.array_equal(m.walk(ident, it), ident)
        assert np.array_equal(m.walk(none, it), none)
        assert np.array_equal(m.walk(shift, it), np.minimum(np.arange(n) + it, n - 1)[None, :])
    cyc = np.arange(8) ^ 1                                    # 2i <-> 2i + 1
    assert np.array_equal(m.walk(cyc, 1), cyc) and np.array_equal(m.walk(cyc, 2), np.arange(8))
    assert np.array_equal(m.walk(cyc, 64), np.arange(8)) and np.array_equal(m.walk(cyc, 63), cyc)
    hole = shift[0].copy()
    hole[5] = -1                                              # chains stop ON frame 5; frame 5 itself goes nowhere
    assert np.array_equal(m.walk(hole, 64), [5, 5, 5, 5, 5, -1, 8, 8, 8])
    assert np.array_equal(m.walk(hole, 2), [2, 3, 4, 5, 5, -1, 8, 8, 8])
    both = np.stack([np.stack([hole, shift[0]]), np.stack([cyc.tolist() + [8], ident[0]])])       # [2, 2, 9]: rows apart
    out = m.walk(both, 3)
    assert out.dtype == both.dtype and np.array_equal(out[0, 0], m.walk(hole, 3)) and np.array_equal(out[1, 1], ident[0])


@pytest.mark.parametrize("order", [1, 2])
def test_one_step_is_tsst_ref(order):
    x = signal(1500, 3)
    a = m.tmsst_ref(x, window(64), 64, hop_len=3, fs=250.0, padtype="zero", order=order, n_iter=1)
    b = m1.tsst_ref(x, window(64), 64, hop_len=3, fs=250.0, padtype="zero", order=order)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("hop,pad,modulated,n_iter", [(1, "reflect", True, 4), (3, "zero", False, 7), (64, "wrap", True, 64)])
def test_marginal_identity(order, hop, pad, modulated, n_iter):
    """Per row, sum_m' Tx[k, m'] e^(-2 pi i k m' hop / n) = sum_(kept m) V[k, m] e^(-2 pi i k m hop / n): the rotation takes
    the total displacement, so the steps telescope.  Bound: 16 eps sum_m |V[k, m]| (DESIGN 4.13's)."""
    n = 256
    V, tau, tgt, Tx = m.tmsst_ref(signal(N, 1), window(n), n, hop_len=hop, padtype=pad, modulated=modulated, order=order,
                                  n_iter=n_iter)
    k = np.arange(n // 2 + 1)[:, None]
    ph = np.exp(-2j * np.pi * ((k * np.arange(V.shape[1])[None, :] * hop) % n) / n)
    err = np.abs((Tx * ph).sum(1) - (np.where(tgt >= 0, V, 0) * ph).sum(1))
    tol = 16 * np.finfo(np.float64).eps * np.abs(V).sum(1)
    print("marginal identity, worst row: %.3g of its tolerance" % (err / tol).max())
    assert (err <= tol).all()


@pytest.mark.parametrize("order", [1, 2])
def test_concentration_table(order):
    got = {it: table_share(order, it) for it in TABLE[order]}
    print("order %d: %s" % (order, "  ".join("%d: %.4f" % kv for kv in got.items())))
    for it, want in TABLE[order].items():
        assert abs(got[it] - want) < 5e-5, (order, it, got[it])


def test_more_steps_concentrate_more():
    assert table_share(2, 4) > table_share(2, 1)
    assert table_share(2, 4) - table_share(2, 1) > 0.2          # 0.7225 -> 0.9729


def test_a_walk_leaves_the_window():
    """The largest total displacement on the table's signal: 348 frames at n_iter 4, 480 at 32, with H = 128."""
    x, _ = m.delay_signal(N)
    for it, far in ((1, 128), (4, 348), (32, 480)):
        tgt = m.tmsst_ref(x, table_window(), NFFT, order=2, n_iter=it)[2]
        kk, mm = np.nonzero(tgt >= 0)
        assert np.abs(tgt[kk, mm] - mm).max() == far
