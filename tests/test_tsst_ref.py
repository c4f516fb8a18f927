"""The numpy model of the time-reassigned synchrosqueezed STFT (tests/helpers/tsst_ref.py) against the facts it is built
on: an impulse's bins all name the impulse's own column, the marginal identity that stands in for an inverse, the
concentration of impulses (both orders) and of a fast chirp (second order only), and the rotation factor.  CPU only."""
import numpy as np
import pytest

from tests.helpers import sst2_ref as s
from tests.helpers import tsst_ref as m

N, NFFT, SIGMA = 1024, 256, 12
IMPULSES = (300, 500, 517, 800)


def impulse_share(P):
    """Share of the energy P = |.|^2 on the impulses' own columns."""
    return P[:, list(IMPULSES)].sum() / P.sum()


def chirp_share(P, n=NFFT, f0=0.05, f1=0.45, inside=0.05):
    """Share of the rows' energy on the column where the chirp crosses the row, rows at least `inside` inside the band."""
    k = np.arange(n // 2 + 1)
    rows = k[(k / n >= f0 + inside) & (k / n <= f1 - inside)]
    cols = np.rint((rows / n - f0) / ((f1 - f0) / N)).astype(int)
    return P[rows, cols].sum() / P[rows].sum()


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("arith", ["fft", "dft"])
def test_an_isolated_impulse_sends_every_kept_bin_to_its_own_column(order, arith):
    n, t0 = 128, 333
    V, tau, tgt, Tx, d = m.tsst_ref(m.impulses(700, [t0]), s.gauss_window(n, n / 10.0), n, order=order, arith=arith,
                                    details=True)
    keep = d["keep"]
    u0 = t0 - np.arange(V.shape[1])[None, :]
    err = np.abs(d["offset"] - u0)[keep].max()
    print("kept %d bins, worst |offset - u0| %.3g" % (keep.sum(), err))
    assert keep.sum() >= 65 * 100 and err <= 1e-9
    assert (tgt[keep] == t0).all()
    g = s.gauss_window(n, n / 10.0)
    assert np.allclose(np.abs(Tx[:, t0]), g.sum(), rtol=1e-12)          # the rotation aligns every contribution
    assert not np.delete(Tx, t0, axis=1).any()


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("hop,pad,modulated", [(1, "reflect", True), (3, "zero", False), (64, "wrap", True)])
def test_marginal_identity(order, hop, pad, modulated):
    n = 256
    x, _ = s.chirp(N, 0.05, 0.45)
    x = x + m.impulses(N, IMPULSES, 8.0)
    V, tau, tgt, Tx, d = m.tsst_ref(x, s.gauss_window(n, SIGMA), n, hop_len=hop, padtype=pad, modulated=modulated,
                                    order=order, details=True)
    k = np.arange(n // 2 + 1)[:, None]
    ph = np.exp(-2j * np.pi * ((k * np.arange(V.shape[1])[None, :] * hop) % n) / n)
    err = np.abs((Tx * ph).sum(1) - (np.where(d["keep"], V, 0) * ph).sum(1)).max() / np.abs(V).max()
    print("marginal identity: %.3g of max|Sx|" % err)
    assert err <= 1e-12


def test_concentrates_impulses_in_both_orders():
    x = m.impulses(N, IMPULSES)
    win = s.gauss_window(NFFT, SIGMA)
    out1, out2 = m.tsst_ref(x, win, NFFT, order=1), m.tsst_ref(x, win, NFFT, order=2)
    s1, s2, s0 = (impulse_share(np.abs(a) ** 2) for a in (out1[3], out2[3], out1[0]))
    print("impulse share: order 1 %.3f, order 2 %.3f, STFT %.3f" % (s1, s2, s0))
    assert s1 >= 0.85 and s2 >= 0.85 and s0 <= 0.10


def test_second_order_concentrates_a_fast_chirp_where_first_order_does_not():
    x, _ = s.chirp(N, 0.05, 0.45)
    win = s.gauss_window(NFFT, SIGMA)
    s1 = chirp_share(np.abs(m.tsst_ref(x, win, NFFT, order=1)[3]) ** 2)
    s2 = chirp_share(np.abs(m.tsst_ref(x, win, NFFT, order=2)[3]) ** 2)
    print("chirp share: order 1 %.3f, order 2 %.3f" % (s1, s2))
    assert s2 >= 0.95 and s1 <= 0.10


def test_rotation_factor_by_hand():
    # k = 3, from frame 10 to frame 12 at hop 5, n = 16: (3 * (10 - 12) * 5) mod 16 = (-30) mod 16 = 2 -> exp(-2 pi i 2/16)
    z = m.rotation(3, 10, 12, 5, 16)
    assert abs(z - (np.sqrt(0.5) - 1j * np.sqrt(0.5))) <= 1e-15
    # and it is what aligns one impulse's coefficients: frame m sees exp(-2 pi i k (t0 - m hop) / n) (modulated)
    k, t0, mm, hop, n = 5, 40, 37, 1, 32
    assert abs(np.exp(-2j * np.pi * k * (t0 - mm * hop) / n) * m.rotation(k, mm, t0, hop, n) - 1) <= 1e-14
    assert m.rotation(7, 4, 4, 3, 64) == 1
