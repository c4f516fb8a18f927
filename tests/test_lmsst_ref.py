"""CPU tests of the numpy model of the local maximum synchrosqueezing transforms (tests/helpers/lmsst_ref.py) and of the
two default-`delta` functions (`upstream.lmsst_default_delta`, `upstream.lmssq_cwt_default_delta`): numpy on the host."""
import numpy as np
import pytest

from ssqueeze_rs_amd import upstream as up
from tests.helpers import lmsst_ref as r
from tests.helpers import msst_ref as ms
from tests.helpers import sst2_ref as m2


@pytest.mark.parametrize("R,n", [(2, 3), (9, 5), (33, 4)])
def test_model_equals_the_triple_loop_on_random_maps(R, n):
    rng = np.random.default_rng(R)
    A = rng.random((R, n))
    Aq = np.round(A * 4) / 4                                   # many exact ties
    for delta in sorted({1, 2, R // 2, R - 1} - {0}):
        for M in (A, Aq):
            assert np.array_equal(r.rows_of(M, delta), r.rows_brute(M, delta)), (R, delta)
    B = rng.random((3, R, n))
    got = r.rows_of(B, 1)
    for b in range(3):
        assert np.array_equal(got[b], r.rows_brute(B[b], 1))


def test_model_on_maps_built_by_hand():
    R = 9
    col = lambda v: np.asarray(v, dtype=np.float64)[:, None]    # noqa: E731
    # a plateau of equal values: the lowest row of the window wins
    plateau = col([0, 1, 5, 5, 5, 5, 1, 0, 0])
    assert r.rows_of(plateau, 1)[:, 0].tolist() == [1, 2, 2, 2, 3, 4, 5, 6, 7]
    assert r.rows_of(plateau, 2)[:, 0].tolist() == [2, 2, 2, 2, 2, 3, 4, 5, 6]
    # a maximum on the first and on the last row
    first = col([9, 1, 2, 1, 0, 0, 0, 0, 0])
    assert r.rows_of(first, 2)[:, 0].tolist() == [0, 0, 0, 2, 2, 3, 4, 5, 6]
    last = col([0, 0, 0, 0, 0, 0, 1, 2, 9])
    assert r.rows_of(last, 2)[:, 0].tolist() == [0, 0, 0, 1, 6, 7, 8, 8, 8]
    # delta >= R - 1: the window is the column, every row names the column's first largest row
    rng = np.random.default_rng(3)
    A = rng.random((R, 6))
    A[4, 2] = A[:, 2].max() + 1
    A[7, 2] = A[4, 2]                                           # a tie: the lower row
    for delta in (R - 1, R, 50):
        m = r.rows_of(A, delta)
        assert (m == A.argmax(0)[None, :]).all() and m[0, 2] == 4
    # R = 2
    two = np.array([[1.0, 2.0, 3.0], [2.0, 2.0, 1.0]])
    assert r.rows_of(two, 1).tolist() == [[1, 0, 0], [1, 0, 0]]
    assert np.array_equal(r.rows_of(two, 1), r.rows_brute(two, 1))
    # a NaN is never strictly greater and nothing is strictly greater than it: it wins only from the window's first row
    nan = col([1.0, np.nan, 3.0, 0.0])
    assert r.rows_of(nan, 1)[:, 0].tolist() == [0, 2, 1, 2]
    assert np.array_equal(r.rows_of(nan, 1), r.rows_brute(nan, 1))


def test_energy_is_numpys_own_arithmetic():
    rng = np.random.default_rng(5)
    Z = (rng.standard_normal(1000) + 1j * rng.standard_normal(1000))
    assert np.array_equal(r.energy(Z), Z.real * Z.real + Z.imag * Z.imag)
    Z32 = Z.astype(np.complex64)
    A = r.energy(Z32)
    assert A.dtype == np.float64
    assert np.array_equal(A, Z32.real.astype(np.float64) ** 2 + Z32.imag.astype(np.float64) ** 2)   # exact in fp64


@pytest.mark.parametrize("kw", [dict(), dict(flipud=True), dict(squeezing="lebesgue"), dict(dtype=np.complex64)])
def test_column_sums_are_those_of_the_one_step_scatter(kw):
    """A coefficient moves along frequency only: every column of Tx sums to what `msst_ref.scatter` leaves under one-step
    bins with the same kept cells (any bins do; the identity map is taken), up to the order of the additions."""
    N, n = 300, 32
    x = np.random.default_rng(2).standard_normal(N)
    win = m2.gauss_window(n, 4)
    V, bins, Tx = r.lmssq_stft_ref(x, win, n, hop_len=3, delta=3, **kw)
    F = n // 2 + 1
    rdt = np.float32 if V.dtype == np.complex64 else np.float64
    dw = rdt(np.linspace(0, .5, F)[1])
    one_step = np.where(bins >= 0, np.arange(F)[:, None], -1)
    ref = ms.scatter(V, one_step, dw, kw.get("squeezing", "sum"))
    tol = 8 * np.finfo(rdt).eps * float(dw) * np.abs(V).sum(0)
    assert (np.abs(Tx.sum(0) - ref.sum(0)) <= tol + 1e-300).all()
    assert ((bins >= -1) & (bins < F)).all()
    kept = bins >= 0
    tgt = F - 1 - bins if kw.get("flipud") else bins
    cols = np.broadcast_to(np.arange(V.shape[1]), V.shape)
    assert kept[tgt[kept], cols[kept]].all()                    # a kept k always has a kept target


def test_default_delta_of_a_window():
    g = m2.gauss_window(256, 24)
    G = np.abs(np.fft.rfft(g))
    d = up.lmsst_default_delta(g, 256)
    assert d == r.default_delta_stft(g, 256) == 7
    assert G[d] <= 1e-3 * G[0] < G[d - 1]                       # the 60 dB point of a Gaussian's lobe
    # a Hann of 32 samples sized to n_fft = 64: the lobe ends at its first null, bin 2 n_fft / win_len = 4
    h = np.hanning(33)[:32]
    d = up.lmsst_default_delta(h, 64)
    Gh = np.abs(np.fft.rfft(np.pad(h, [16, 16])))
    assert d == r.default_delta_stft(h, 64) == 4
    assert Gh[d] <= 1e-3 * Gh[0] or Gh[d + 1] >= Gh[d]
    # a window with no lobe end inside the rows (a single sample: a flat spectrum ends at once, G[2] >= G[1])
    one = np.zeros(16)
    one[8] = 1.0
    assert up.lmsst_default_delta(one, 16) == 1
    # a monotone spectrum that never falls 60 dB: F - 1
    slow = m2.gauss_window(16, 0.45)
    Gs = np.abs(np.fft.rfft(slow))
    assert (np.diff(Gs) < 0).all() and Gs[-2] > 1e-3 * Gs[0]
    assert up.lmsst_default_delta(slow, 16) == 8
    # the cap
    wide = m2.gauss_window(4096, 0.6)
    assert up.lmsst_default_delta(wide, 4096) <= 256
    with pytest.raises(ValueError):
        up.lmsst_default_delta("hann", 64)


def test_default_delta_of_a_wavelet():
    s = 4.0 * 2 ** (np.arange(48) / 16.0)
    d = up.lmssq_cwt_default_delta("gmw", s)
    # restated: the GMW (gamma 3, beta 60) at scale ratio q is q^beta exp(-(beta / gamma)(q^gamma - 1)) of its peak
    q = s / s[24]
    R = q ** 60.0 * np.exp(-(60.0 / 3.0) * (q ** 3.0 - 1.0))
    want = next(k for k in range(1, 48) if all(R[i] <= 1e-3 for i in (24 - k, 24 + k) if 0 <= i < 48))
    assert d == want and 1 <= d <= 47
    assert R[24 - d] <= 1e-3 and R[24 + d] <= 1e-3 and (R[24 - d + 1] > 1e-3 or R[24 + d - 1] > 1e-3)
    # finer scales: more rows under the response
    assert up.lmssq_cwt_default_delta("gmw", 4.0 * 2 ** (np.arange(96) / 32.0)) in (2 * d - 1, 2 * d, 2 * d + 1)
    # a narrower wavelet: fewer
    assert up.lmssq_cwt_default_delta(("gmw", {"beta": 240}), s) < d
    # two rows: the only delta there is; the cap
    assert up.lmssq_cwt_default_delta("gmw", np.array([4.0, 4.1])) == 1
    assert up.lmssq_cwt_default_delta("morlet", 4.0 * 2 ** (np.arange(2049) / 1024.0)) <= 256
    with pytest.raises(ValueError):
        up.lmssq_cwt_default_delta("gmw", np.array([4.0]))
