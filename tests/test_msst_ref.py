"""CPU tests of the numpy model of the multisynchrosqueezed STFT (tests/helpers/msst_ref.py): what the
definition promises, on the model alone.  No GPU, no library."""
import functools

import numpy as np
import pytest

from tests.helpers import msst_ref as r
from tests.helpers import sst2_ref as m2

N, NFFT = 1024, 256


@functools.lru_cache(maxsize=None)
def fm():
    """The sinusoidal FM of DESIGN 4.17 (fi = 0.25 + 0.15 sin(2 pi 3 t / N) cycles/sample) and its Gaussian window."""
    x, _ = r.fm_signal(N)
    win = m2.gauss_window(NFFT, 24)
    x.setflags(write=False)
    win.setflags(write=False)
    return x, win


@functools.lru_cache(maxsize=None)
def model(order, n_iter):
    x, win = fm()
    out = r.mssq_stft_ref(x, win, NFFT, order=order, n_iter=n_iter)
    for a in out:
        a.setflags(write=False)
    return out


def test_walk_by_hand():
    m = np.array([[1], [2], [2], [-1], [3], [6], [5]])          # 0 -> 1 -> 2 = 2; 3: no map; 4 -> 3 stops; 5 <-> 6
    assert r.walk(m, 1)[:, 0].tolist() == [1, 2, 2, -1, 3, 6, 5]
    assert r.walk(m, 2)[:, 0].tolist() == [2, 2, 2, -1, 3, 5, 6]
    assert r.walk(m, 3)[:, 0].tolist() == [2, 2, 2, -1, 3, 6, 5]
    m3 = np.random.default_rng(0).integers(-1, 7, size=(3, 7, 5))
    w3 = r.walk(m3, 5)
    for b in range(3):
        assert np.array_equal(w3[b], r.walk(m3[b], 5))


@pytest.mark.parametrize("kw", [dict(), dict(flipud=True), dict(squeezing="lebesgue", hop_len=3, padtype="wrap")])
def test_one_step_of_order_two_is_the_second_order_transform(kw):
    x, win = fm()
    V, w2, kk, Tx = m2.sst2_ref(x, win, NFFT, **kw)
    Vm, wm, bm, Txm = r.mssq_stft_ref(x, win, NFFT, order=2, n_iter=1, **kw)
    assert np.array_equal(Vm, V) and np.array_equal(wm, w2) and np.array_equal(bm, kk)
    assert np.array_equal(Txm.view(np.float64), Tx.view(np.float64))


@pytest.mark.parametrize("order", [1, 2])
def test_every_column_keeps_its_sum(order):
    """sum_k Tx[k, j] = dw sum_(kept k) Sx[k, j] whatever the walk does, up to the order of the additions: within
    4 eps dw sum|V| per column."""
    V = model(order, 1)[0]
    dw = 0.5 / (NFFT // 2)
    tol = 4 * np.finfo(np.float64).eps * dw * np.abs(V).sum(0)
    base = model(order, 1)[3].sum(0)
    for n_iter in (1, 2, 4, 32):
        err = np.abs(model(order, n_iter)[3].sum(0) - base)
        print("order %d n_iter %d: worst column %.3g of its tolerance" % (order, n_iter, (err / tol).max()))
        assert (err <= tol).all()


@pytest.mark.parametrize("order", [1, 2])
def test_a_map_at_its_fixed_point_stays(order):
    """A chain that has ended by 32 steps -- on a bin that maps to itself or has no map -- does not move with more steps;
    what still moves then is on a cycle (off the ridge the FM signal's maps hold cycles between weak bins: 4 % of the
    chains of order 1 and 14 % of order 2, which carry no visible energy), and the map made of the ended chains alone is
    a fixed point of the walk."""
    _, w, _, _ = model(order, 1)
    m, _ = r.bins_of(w, NFFT // 2 + 1, 1.0, np.float64)
    at32 = r.walk(m, 32)
    cols = np.broadcast_to(np.arange(m.shape[1]), m.shape)
    nxt = np.where(at32 >= 0, m[np.maximum(at32, 0), cols], -1)
    ended = (at32 < 0) | (nxt == at32) | (nxt == -1)
    print("order %d: %d of %d chains still turn after 32 steps" % (order, (~ended).sum(), (at32 >= 0).sum()))
    assert ended.sum() > 0.5 * ended.size
    for more in (1, 2, 32):
        assert np.array_equal(r.walk(m, 32 + more)[ended], at32[ended])
    settled = np.where(ended, at32, -1)
    idem = np.where(settled >= 0, settled, -1)
    idem[settled[settled >= 0], cols[settled >= 0]] = settled[settled >= 0]        # every end bin maps to itself
    for n_iter in (2, 3, 64):
        assert np.array_equal(r.walk(idem, n_iter), idem)


def test_more_steps_concentrate_the_fm_signal():
    """Top-cell shares of the model: order 2 0.82 / 0.96 at n_iter 1 / 4, order 1 0.23 / 0.40."""
    s = {(o, n): r.top_cell_share(model(o, n)[3], NFFT) for o in (1, 2) for n in (1, 4)}
    print("top-cell share:", {k: round(v, 4) for k, v in s.items()})
    assert s[2, 4] >= s[2, 1] + 0.1
    assert s[1, 4] > s[1, 1]
