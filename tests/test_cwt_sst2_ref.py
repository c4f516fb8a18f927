"""CPU tests of the definition of the second-order synchrosqueezed CWT on its numpy model,
tests/helpers/cwt_sst2_ref.py: the operator is exact on a linear chirp, with or without a Gaussian envelope, where the
first-order one is biased; and it puts a fast chirp's energy on the chirp's own bin."""
import numpy as np
import pytest

from tests.helpers import cwt_sst2_ref as m

GMW = ("gmw", 3.0, 60.0)


def _scales(nv, count):
    """s0 2^(k / nv), s0 = wc / pi: the peak frequency of scale k is 0.5 2^(-k / nv) cycles/sample."""
    return m.gmw_wc(3.0, 60.0) / np.pi * 2.0 ** (np.arange(count) / nv)


@pytest.mark.parametrize("sigma", [None, 150.0], ids=["constant", "gaussian"])
def test_second_order_is_exact_on_a_linear_chirp(sigma):
    """Chirp 0.05 -> 0.25 cycles/sample, N = 1024, GMW(3, 60), nv = 16 (80 scales: peak frequencies 0.5 ... 0.016), on
    columns N/5 .. 4N/5 and bins with |W| >= 0.3 max|W|.  Measured: second order 4.4e-15 (constant amplitude) and
    3e-15 (Gaussian envelope, sigma = 150), first order 4.9e-3 and 1.7e-3."""
    N = 1024
    x, fi = m.chirp(N, 0.05, 0.25, sigma)
    s = _scales(16, 80)
    W, w2, _, _, d = m.cwt_sst2_ref(x, GMW, s, m.log_freqs(N, len(s)), details=True)
    c = np.arange(N // 5, 4 * N // 5)
    big = (np.abs(W) >= 0.3 * np.abs(W).max())[:, c]
    e2 = np.abs(w2[:, c] - fi[c])[big].max()
    e1 = np.abs(d["w1"][:, c] - fi[c])[big].max()
    print("sigma %s: second order %.3g, first order %.3g (%d bins)" % (sigma, e2, e1, big.sum()))
    assert big.sum() > 1000
    assert d["use2"][:, c][big].all()
    assert e2 <= 1e-12
    assert e1 >= 1e-3


def test_dft_arithmetic_agrees_with_fft():
    N = 200
    x, _ = m.chirp(N, 0.05, 0.3)
    s = _scales(4, 20)
    f = m.log_freqs(N, len(s))
    a = m.cwt_sst2_ref(x, GMW, s, f, padtype="symmetric")
    b = m.cwt_sst2_ref(x, GMW, s, f, padtype="symmetric", arith="dft")
    assert np.abs(a[0] - b[0]).max() <= 1e-13 * np.abs(a[0]).max()
    assert np.array_equal(np.isinf(a[1]), np.isinf(b[1]))
    # (w2 is a quotient of differences of products: where D is small the two arithmetics differ by far more than an
    # ulp -- the GPU tests take their tolerance from that difference, nothing is asserted on it here)
    big = np.abs(a[0]) >= 1e-2 * np.abs(a[0]).max()
    print("w2: fft against dft %.3g on %d strong bins" % (np.abs(a[1] - b[1])[big].max(), big.sum()))


def test_second_order_concentrates_a_fast_chirp():
    """Chirp 0.02 -> 0.45 cycles/sample, N = 512, GMW(3, 60), scales s0 2^(k/32) (s0 = wc / pi, k < 180), 'maximal' log
    frequencies: the share of |Tx|^2 on the chirp's own bin, over columns N/5 .. 4N/5.  Measured: second order 0.9993,
    first order 0.8224."""
    N = 512
    x, fi = m.chirp(N, 0.02, 0.45)
    s = _scales(32, 180)
    f = m.log_freqs(N, len(s))
    W, w2, _, Tx2, d = m.cwt_sst2_ref(x, GMW, s, f, details=True)
    own, _ = m.bin_positions(fi, f, "log")
    # the first-order map: the same scatter under w1
    b1, _ = m.bin_positions(d["w1"], f, "log")
    Tx1 = np.zeros_like(Tx2)
    cols = np.arange(N)
    keep = np.isfinite(w2)
    for i in range(len(s)):
        k = keep[i]
        Tx1[b1[i, k], cols[k]] += W[i, k]
    c = np.arange(N // 5, 4 * N // 5)

    def share(Tx):
        E = np.abs(Tx) ** 2
        return E[own[c], c].sum() / E[:, c].sum()
    s2, s1 = share(Tx2), share(Tx1)
    print("own-bin share: second order %.4f, first order %.4f" % (s2, s1))
    assert s2 >= 0.99
    assert s1 <= 0.9
