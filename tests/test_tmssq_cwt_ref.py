"""The numpy model of the time-reassigned multisynchrosqueezed CWT (tests/helpers/tmssq_cwt_ref.py) against the facts it
is built on: n_iter = 1 is `tssq_cwt_ref`, the per-row marginal identity, the concentration table of DESIGN 4.22, and the
fact the walk kernel's design rests on -- a coefficient's target may lie a whole row away.  CPU only."""
import functools

import numpy as np
import pytest

from tests.helpers import tmssq_cwt_ref as m
from tests.helpers import tssq_cwt_ref as m1

N = 1024
GMW = ("gmw", 3.0, 60.0)
SCALES = m.table_scales(GMW)                                  # 160 log scales at nv 32 from wc / pi
NU = m1.row_freqs(GMW, SCALES)
ITERS = (1, 2, 4, 8, 32)
# the share of the rows' energy (0.06 < nu < 0.40) in their largest cell, by n_iter.  The committed helper's
# figures; the entry 0.97785 sits on a rounding boundary of the fourth digit and is pinned to five.
TABLE = {
    ("clean", 2): (0.7942, 0.9608, 0.9792, 0.9778, 0.97785),
    ("clean", 1): (0.4926, 0.7716, 0.8096, 0.7662, 0.7551),
    ("noise", 2): (0.6083, 0.8750, 0.9119, 0.9068, 0.9052),
}


def table_signal(kind):
    x, _ = m.delay_signal(N, 512.0, 150.0, 4)
    if kind == "noise":
        x = x + 0.3 * x.std() * np.random.default_rng(0).standard_normal(N)
    return x


@functools.lru_cache(maxsize=None)
def one_step(kind, order):
    """(W, tau, t1) of the one-step model on the table's signal; computed once, read-only."""
    W, tau, t1, _ = m1.tssq_cwt_ref(table_signal(kind), GMW, SCALES, order=order, squeeze=False)
    for a in (W, tau, t1):
        a.setflags(write=False)
    return W, tau, t1


@functools.lru_cache(maxsize=None)
def table_share(kind, order, n_iter):
    W, _, t1 = one_step(kind, order)
    re, im, _, _ = m1.scatter(W, m.walk(t1, n_iter), NU)
    return m.top_cell_share(re.astype(np.float64) + 1j * im.astype(np.float64), NU)


@pytest.mark.parametrize("kind,order", list(TABLE))
def test_concentration_table(kind, order):
    got = [table_share(kind, order, it) for it in ITERS]
    print("%s order %d: %s" % (kind, order, "  ".join("%d: %.6f" % kv for kv in zip(ITERS, got))))
    for it, g, want in zip(ITERS, got, TABLE[kind, order]):
        assert abs(g - want) <= 5e-5, (kind, order, it, g)


def test_more_steps_concentrate_more():
    assert table_share("clean", 2, 1) < table_share("clean", 2, 2) < table_share("clean", 2, 4)
    assert table_share("clean", 2, 4) - table_share("clean", 2, 1) > 0.15            # 0.7942 -> 0.9792
    assert table_share("noise", 2, 4) - table_share("noise", 2, 1) > 0.25            # 0.6083 -> 0.9119


@pytest.mark.parametrize("order", [1, 2])
def test_one_step_is_tssq_cwt_ref(order):
    x = table_signal("noise")[:300]
    sc = SCALES[::8]
    for rdt in (np.float64, np.float32):
        a = m.tmssq_cwt_ref(x, GMW, sc, dt=0.5, padtype="zero", order=order, n_iter=1, rdt=rdt)
        b = m1.tssq_cwt_ref(x, GMW, sc, dt=0.5, padtype="zero", order=order, rdt=rdt)
        for u, v in zip(a, b):
            assert u.dtype == v.dtype and np.array_equal(u, v)


@pytest.mark.parametrize("order", [1, 2])
def test_marginal_identity(order):
    """sum_m' Tx[i, m'] e^{-2 pi i nu_i m'} = sum over the kept j of Wx[i, j] e^{-2 pi i nu_i j} per row at n_iter 4: the
    rotation takes the total displacement, so the steps telescope.  The bound is tests/test_tssq_cwt_ref.py's:
    1e-12 max|W|."""
    for kind in ("clean", "noise"):
        W, tau, mm, Tx = m.tmssq_cwt_ref(table_signal(kind), GMW, SCALES, order=order, n_iter=4)
        a, b = m1.marginal(Tx, NU), m1.marginal(W, NU, mm >= 0)
        err = np.hypot((a[0] - b[0]).astype(np.float64), (a[1] - b[1]).astype(np.float64))
        print("order %d %-5s worst row %.3g of max|W|" % (order, kind, err.max() / np.abs(W).max()))
        assert err.max() <= 1e-12 * np.abs(W).max()
        assert np.array_equal(mm == -1, np.isposinf(tau))


def test_a_target_lies_a_whole_row_away():
    """What the walk kernel is designed around: tssq_cwt clamps to +-N, not to a window.  On the table's signal the
    largest displacement is 1006 of 1024 columns after one step and 1023 after four, half of the kept bins move more than
    64 columns and a tenth more than 256, and 65 % of them end elsewhere than their one-step target at n_iter 4."""
    _, _, t1 = one_step("clean", 2)
    i, j = np.nonzero(t1 >= 0)
    d1 = np.abs(t1[i, j] - j)
    mm = m.walk(t1, 4)
    d4 = np.abs(mm[i, j] - j)
    print("n_iter 1: max %d, > 64: %.3f, > 256: %.3f;  n_iter 4: max %d, moved on: %.3f"
          % (d1.max(), (d1 > 64).mean(), (d1 > 256).mean(), d4.max(), (mm[i, j] != t1[i, j]).mean()))
    assert d1.max() > 1000 and d4.max() > 1000
    assert (d1 > 64).mean() > 0.45 and (d1 > 256).mean() > 0.08
    assert (mm[i, j] != t1[i, j]).mean() > 0.6
