"""CPU tests of tests/helpers/cwt_scatter_check.py: a NumPy model of the fp32 reassignment (phase transform in fp32, the
oracle's bin rule, run-by-run accumulation in fp32) meets every bound of the checker, and each kind of kernel error the
checker exists for makes it fail: an element in the wrong row, a run flushed twice, a stray write into an empty cell, a
dropped last term, a cell that is not a number, w computed from its neighbour's dWx, a keep mask off its threshold."""
import numpy as np
import pytest

from oracle import ssq_oracle as o
from tests.helpers import cwt_scatter_check as chk


def _model(lebesgue=False, gamma=1e-3):
    N, na = 3000, 24
    x = o.synth_signal(N, 5, np.float32)
    x[1000:1400] = 0.0
    scales = 2.0 ** (np.arange(4, 4 + na) / 4.0)
    Wx_o, _, dWx_o = o.cwt(x.astype(np.float64), "morlet", scales=scales, derivative=True)
    Wx, dWx = Wx_o.astype(np.complex64), dWx_o.astype(np.complex64)
    f = o.cwt_ssq_freqs(na, 1.0 / scales[-1], 1.0 / scales[0], "log")
    A, B, Cc, D = dWx.real, dWx.imag, Wx.real, Wx.imag      # float32 throughout
    with np.errstate(all="ignore"):
        w = np.abs((B * Cc - A * D) / ((Cc * Cc + D * D) * np.float32(2.0 * np.pi)))
    w = np.where(np.abs(Wx.astype(np.complex128)) < float(np.float32(gamma)), np.float32(np.inf), w).astype(np.float32)
    b, valid, _ = o.cwt_bins(w.astype(np.float64), f)
    k = np.where(valid, na - 1 - b, -1)
    Tx = np.zeros((na, N), dtype=np.complex64)
    leb = np.float32(1.0 / na)
    for i in range(na):                                     # ascending rows, one fp32 addition per term
        m = k[i] >= 0
        Tx[k[i][m], np.flatnonzero(m)] += (leb if lebesgue else Wx[i][m])
    return Tx, Wx, dWx, w, k, f, gamma


@pytest.mark.parametrize("lebesgue", [False, True])
def test_numpy_model_meets_every_bound(lebesgue):
    Tx, Wx, dWx, w, k, f, gamma = _model(lebesgue)
    rows = chk.assert_scatter_cells(Tx, Wx, k, lebesgue, np.float32)
    assert rows.shape == (Tx.shape[0],) and rows.max() <= 1.0
    assert (k < 0).any() and (k >= 0).any()
    assert chk.assert_bins_follow_w(k, w, f, True, np.float32) <= 1e-5
    exempt, wr = chk.assert_w_follows_wx(w, Wx, dWx, gamma, np.float32)
    assert exempt <= 1e-5 and 0.0 < wr.max() <= 1.0


def test_scatter_errors_are_caught():
    Tx, Wx, dWx, w, k, f, gamma = _model()
    i, j = np.argwhere(k >= 0)[len(k) // 2 * 700]
    row = k[i, j]
    other = row + 1 if row + 1 < Tx.shape[0] else row - 1
    bad = Tx.copy()                                         # one element in the neighbouring row
    bad[row, j] -= Wx[i, j]
    bad[other, j] += Wx[i, j]
    with pytest.raises(AssertionError):
        chk.assert_scatter_cells(bad, Wx, k, False, np.float32)
    bad = Tx.copy()                                         # a run added twice
    bad[row, j] += Wx[i, j]
    with pytest.raises(AssertionError):
        chk.assert_scatter_cells(bad, Wx, k, False, np.float32)
    empty = np.ones(Tx.shape, dtype=bool)
    for r in range(k.shape[0]):
        m = k[r] >= 0
        empty[k[r][m], np.flatnonzero(m)] = False
    e = np.argwhere(empty)[0]
    bad = Tx.copy()                                         # a stray write of the smallest fp32 number
    bad[e[0], e[1]] = np.float32(1e-45)
    with pytest.raises(AssertionError):
        chk.assert_scatter_cells(bad, Wx, k, False, np.float32)
    for cell in ((e[0], e[1]), (row, j)):                   # not a number, in an empty cell and in a summed one
        for v in (np.nan, complex(0.0, np.nan), np.inf):
            bad = Tx.copy()
            bad[cell] = v
            with pytest.raises(AssertionError):
                chk.assert_scatter_cells(bad, Wx, k, False, np.float32)
            with pytest.raises(AssertionError):
                chk.assert_scatter_cells(bad, Wx, k, True, np.float32)
    bad = Tx.copy()                                         # the last term of a cell dropped
    bad[row, j] = Tx[row, j] - Wx[i, j]
    with pytest.raises(AssertionError):
        chk.assert_scatter_cells(bad, Wx, k, False, np.float32)


def test_phase_and_keep_errors_are_caught():
    Tx, Wx, dWx, w, k, f, gamma = _model()
    with pytest.raises(AssertionError):                     # w of column j from dWx of column j + 1
        chk.assert_w_follows_wx(w, Wx, np.roll(dWx, 1, axis=1), gamma, np.float32)
    with pytest.raises(AssertionError):                     # Wx and dWx swapped
        chk.assert_w_follows_wx(w, dWx, Wx, gamma, np.float32)
    w2 = w.copy()                                           # a kept element marked as dropped
    i, j = np.argwhere(np.isfinite(w))[0]
    w2[i, j] = np.inf
    with pytest.raises(AssertionError):
        chk.assert_w_follows_wx(w2, Wx, dWx, gamma, np.float32)
    k2 = k.copy()                                           # a bin one row off
    k2[i, j] = k2[i, j] + 1 if k2[i, j] >= 0 else 0
    with pytest.raises(AssertionError):
        chk.assert_bins_follow_w(k2, w, f, True, np.float32)
    with pytest.raises(AssertionError):                     # a row of Wx against the neighbouring row of the oracle
        chk.assert_rows_follow_oracle(Wx, dWx, np.roll(Wx, 1, axis=0).astype(np.complex128),
                                      dWx.astype(np.complex128))


def test_fp64_sums_are_held_to_the_fp64_bound():
    """fp64 results: the reference sum runs in long double, so the bound's slack belongs to the code under test: sums
    in fp64 pass, the same sums rounded to fp32 do not, nor does a NaN cell."""
    Tx32, Wx32, dWx, w, k, f, gamma = _model()
    Wx = Wx32.astype(np.complex128) * (1.0 + 2.0 ** -30)    # terms that need all of fp64
    na, N = k.shape
    Tx = np.zeros((na, N), dtype=np.complex128)
    for i in range(na):
        m = k[i] >= 0
        Tx[k[i][m], np.flatnonzero(m)] += Wx[i][m]
    assert chk.assert_scatter_cells(Tx, Wx, k, False, np.float64).max() <= 1.0
    with pytest.raises(AssertionError):
        chk.assert_scatter_cells(Tx.astype(np.complex64).astype(np.complex128), Wx, k, False, np.float64)
    Tx[0, 0] = np.nan
    with pytest.raises(AssertionError):
        chk.assert_scatter_cells(Tx, Wx, k, False, np.float64)
