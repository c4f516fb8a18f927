"""The numpy model of the second-order synchrosqueezed STFT (tests/helpers/sst2_ref.py) against the facts it is built
on: it recovers a linear chirp's instantaneous frequency where the first-order operator is biased, falls back to the
first-order operator on a tone, survives an all-zero signal and conserves the row sum.  No GPU."""
import numpy as np
import pytest

from tests.helpers import sst2_ref as m


@pytest.mark.parametrize("arith", ["fft", "dft"])
def test_linear_chirp_instantaneous_frequency(arith):
    """sigma = 8, n_fft = 128, N = 1024, a sweep 0.15 -> 0.35 cycles/sample (the band keeps the real signal's mirror
    image, which no order removes, 0.3 cycles/sample = 15 window bandwidths away): |Re w2 - phi'(t)| < 1e-6 on bins
    with |V| >= 1e-3 max, away from the padded ends; the first-order error there is ~1e-3."""
    N, n = 1024, 128
    x, fi = m.chirp(N, 0.15, 0.35)
    V, w2, kk, Tx, d = m.sst2_ref(x, m.gauss_window(n, 8), n, arith=arith, details=True)
    cols = slice(n, N - n)
    big = (np.abs(V) >= 1e-3 * np.abs(V).max())[:, cols]
    e2 = np.abs(d["re_w2"] - fi[None, :])[:, cols][big].max()
    e1 = np.abs(d["re_w1"] - fi[None, :])[:, cols][big].max()
    print("second order %.3g, first order %.3g cycles/sample" % (e2, e1))
    assert e2 < 1e-6
    assert e1 > 1e-4
    assert d["use2"][:, cols][big].all()
    # the reported frequency is fs |Re w2| on kept bins
    assert np.array_equal(w2[:, cols][big], np.abs(d["re_w2"])[:, cols][big])


def test_pure_tone_is_first_order():
    """The numerator of q vanishes for a tone: w2 == w1 within 1e-9 on bins with |V| >= 1e-3 max.  (sigma = n_fft / 16 as
    in the chirp test: the window's truncation step, e^-32, stays far below those bins, and so does the mirror image of
    the real tone at 0.25 cycles/sample, 8 window bandwidths from the nearest of them.)"""
    N, n = 512, 64
    x = np.cos(2 * np.pi * 0.25 * np.arange(N) + 0.3)
    V, w2, kk, Tx, d = m.sst2_ref(x, m.gauss_window(n, 4), n, details=True)
    cols = slice(n, N - n)
    big = (np.abs(V) >= 1e-3 * np.abs(V).max())[:, cols]
    assert big.sum() > 1000 and d["use2"][:, cols][big].all()
    assert np.abs(d["re_w2"] - d["re_w1"])[:, cols][big].max() < 1e-9
    assert np.abs(d["re_w1"][:, cols][big] - 0.25).max() < 1e-9


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_all_zero_input(dtype):
    V, w2, kk, Tx = m.sst2_ref(np.zeros(200), m.gauss_window(32, 4), 32, hop_len=3, dtype=dtype)
    assert Tx.dtype == dtype and not np.isnan(Tx.view(Tx.real.dtype)).any() and not Tx.any()
    assert np.isinf(w2).all() and (kk == -1).all()


@pytest.mark.parametrize("flipud,modulated,padtype", [(False, True, "reflect"), (True, False, "wrap")])
def test_row_sum_is_conserved(flipud, modulated, padtype):
    """Tx.sum(0) == dw * sum of the kept V: every kept bin lands in exactly one row."""
    rng = np.random.default_rng(3)
    N, n = 300, 32
    x = m.chirp(N, 0.1, 0.3)[0] + 0.1 * rng.standard_normal(N)
    V, w2, kk, Tx, d = m.sst2_ref(x, m.gauss_window(n, 5), n, hop_len=2, fs=2.0, padtype=padtype, modulated=modulated,
                                  flipud=flipud, details=True)
    want = (d["dw"] * np.where(d["keep"], V, 0)).sum(0)
    assert np.abs(Tx.sum(0) - want).max() <= 1e-12 * np.abs(V).sum(0).max()
    assert kk.min() >= -1 and kk.max() <= n // 2
    assert np.array_equal(kk == -1, ~d["keep"])


def test_the_two_arithmetics_agree_to_rounding():
    """'fft' and 'dft' differ by rounding alone (their difference is what the GPU tolerances are taken from), and V is
    upstream's STFT: np.fft.rfft of the rotated, windowed frames."""
    N, n, hop = 400, 64, 3
    x = m.chirp(N, 0.05, 0.4)[0]
    win = m.gauss_window(n, 7)
    a = m.sst2_ref(x, win, n, hop_len=hop, arith="fft")
    b = m.sst2_ref(x, win, n, hop_len=hop, arith="dft")
    assert np.abs(a[0] - b[0]).max() <= 1e-12 * np.abs(a[0]).max()
    big = np.abs(a[0]) >= 1e-2 * np.abs(a[0]).max()
    assert np.abs(a[1] - b[1])[big].max() < 1e-10
    xp = np.pad(x, [n // 2, n - 1 - n // 2], mode="reflect")
    fr = np.stack([xp[i * hop:i * hop + n] for i in range((N - 1) // hop + 1)], axis=1)
    S = np.fft.rfft(np.fft.ifftshift(fr * win[:, None], axes=0), axis=0)
    assert np.array_equal(a[0], S)
