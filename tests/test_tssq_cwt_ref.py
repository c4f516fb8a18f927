"""CPU checks of the numpy model of the time-reassigned synchrosqueezed CWT (tests/helpers/tssq_cwt_ref.py):
the facts the definition rests on, and the concentration table DESIGN 4.16 quotes.  No GPU, no library."""
import functools

import numpy as np
import pytest

from tests.helpers import cwt_sst2_ref as c2
from tests.helpers import tssq_cwt_ref as m
from tests.helpers.tsst_ref import impulses

N = 512
GMW = ("gmw", 3.0, 60.0)
MORLET = ("morlet", 13.4)
SCALES = 2.0 * 2.0 ** (np.arange(180) / 32)               # 180 log scales at nv 32 from 2
FIT = 96                                                  # scales 2 ... 15.7: the wavelet fits the padding
T0 = 200                                                  # the impulse
F0, F1 = 0.02, 0.45                                       # the chirp, cycles/sample over the N samples


def energy(A):
    return A.real.astype(np.float64) ** 2 + A.imag.astype(np.float64) ** 2


def chirp_rows(wavelet):
    """(rows with 0.07 < nu < 0.40, the column where the chirp crosses each of them)."""
    nu = m.row_freqs(wavelet, SCALES)
    rows = np.nonzero((nu > 0.07) & (nu < 0.40))[0]
    return rows, np.rint((nu[rows] - F0) * N / (F1 - F0)).astype(np.int64)


def column_share(A, col):
    """The share of the energy of A [na, N] on column `col`."""
    e = energy(A)
    return float(e[:, col].sum() / e.sum())


def ridge_share(A, rows, cols, reach=0):
    """The share of the energy of the rows `rows` of A within +-reach columns of `cols`."""
    e = energy(A)[rows]
    r = np.arange(len(rows))
    return float(sum(e[r, cols + k].sum() for k in range(-reach, reach + 1)) / e.sum())


def table_shares(transform):
    """DESIGN 4.16's table from `transform(x, wavelet, padtype, order) -> (Tx, Wx)` [180, 512]: a dict of shares."""
    out = {}
    imp = impulses(N, [T0])
    for pad in ("zero", "reflect"):
        for order in (1, 2):
            Tx, Wx = transform(imp, GMW, pad, order)
            out["impulse", pad, order] = column_share(Tx, T0)
        out["impulse", pad, "W"] = column_share(Wx, T0)
    x = c2.chirp(N, F0, F1)[0]
    for wavelet in (GMW, MORLET):
        rows, cols = chirp_rows(wavelet)
        for order in (1, 2):
            Tx, Wx = transform(x, wavelet, "reflect", order)
            out["chirp", wavelet[0], order, 0] = ridge_share(Tx, rows, cols)
            out["chirp", wavelet[0], order, 1] = ridge_share(Tx, rows, cols, 1)
        out["chirp", wavelet[0], "W", 1] = ridge_share(Wx, rows, cols, 1)
    return out


# DESIGN 4.16's table, to four digits (the model of exactly this definition, np.fft)
TABLE = {
    ("impulse", "zero", 1): 0.9977, ("impulse", "zero", 2): 0.9978, ("impulse", "zero", "W"): 0.0296,
    ("impulse", "reflect", 1): 0.9829, ("impulse", "reflect", 2): 0.9718, ("impulse", "reflect", "W"): 0.0293,
    ("chirp", "gmw", 1, 0): 0.2178, ("chirp", "gmw", 2, 0): 0.9985,
    ("chirp", "gmw", 1, 1): 0.5387, ("chirp", "gmw", 2, 1): 0.9996, ("chirp", "gmw", "W", 1): 0.0790,
    ("chirp", "morlet", 1, 0): 0.1517, ("chirp", "morlet", 2, 0): 0.9985,
}


def _model(x, wavelet, pad, order):
    W, _, _, Tx = m.tssq_cwt_ref(x, wavelet, SCALES, padtype=pad, order=order)
    return Tx, W


@functools.lru_cache(maxsize=None)
def model_table():
    return table_shares(_model)


def test_concentration_table():
    got = model_table()
    assert len(chirp_rows(GMW)[0]) == 53 and len(chirp_rows(MORLET)[0]) == 80
    for key, want in TABLE.items():
        print("%-32s model %.5f   table %.4f" % (key, got[key], want))
        assert abs(got[key] - want) <= 5e-5, key


def test_order_2_beats_order_1_on_the_chirp():
    got = model_table()
    for wv in ("gmw", "morlet"):
        assert got["chirp", wv, 2, 0] > got["chirp", wv, 1, 0] + 0.5
        assert got["chirp", wv, 2, 1] > got["chirp", wv, 1, 1] + 0.4
        assert got["chirp", wv, 1, 1] > got["chirp", wv, "W", 1]


def test_impulse_names_its_own_column():
    """W(b) = k(b - t0) and Wt(b) = (t0 - b) k(b - t0): j + Re(Wt/W) = t0 at every scale whose wavelet fits the padding.
    Order 1's tau on the isolated zero-padded impulse names the impulse's column on every bin with |W| >= 1e-6 max."""
    W, tau, mm, _ = m.tssq_cwt_ref(impulses(N, [T0]), GMW, SCALES[:FIT], padtype="zero", order=1, squeeze=False)
    big = np.abs(W) >= 1e-6 * np.abs(W).max()
    assert big.sum() > 20000
    assert (mm[big] == T0).all()
    assert (np.rint(np.arange(N)[None, :] + tau)[big] == T0).all()


@pytest.mark.parametrize("order", [1, 2])
def test_marginal_identity(order):
    """sum_m' Tx[i, m'] e^{-2 pi i nu_i m'} = sum over the kept j of Wx[i, j] e^{-2 pi i nu_i j}, per row: every moved
    coefficient carries exactly the phase that its new column takes back.  The model's Tx is rounded once to complex128,
    so a row may be off by N roundings of cells no larger than the row's sum of |W|; measured worst row 1.5e-15 ... 3.7e-15
    of max|W|."""
    nu = m.row_freqs(GMW, SCALES)
    for x, pad in ((c2.chirp(N, F0, F1)[0], "reflect"), (impulses(N, [T0]), "zero"),
                   (c2.chirp(N, F0, F1)[0] + impulses(N, [128, 256, 384], 8.0), "symmetric")):
        W, tau, mm, Tx = m.tssq_cwt_ref(x, GMW, SCALES, padtype=pad, order=order)
        a, b = m.marginal(Tx, nu), m.marginal(W, nu, mm >= 0)
        err = np.hypot((a[0] - b[0]).astype(np.float64), (a[1] - b[1]).astype(np.float64))
        print("order %d %-9s worst row %.3g of max|W|" % (order, pad, err.max() / np.abs(W).max()))
        assert err.max() <= 1e-12 * np.abs(W).max()
        assert np.array_equal(mm == -1, np.isposinf(tau))


@pytest.mark.parametrize("wavelet", [GMW, MORLET], ids=["gmw", "morlet"])
def test_d2_is_the_crossing_time_of_a_gaussian_chirp(wavelet):
    """x(t) = exp(-(t - tc)^2 / (2 s^2)) cos(w0 t + k t^2 / 2): with u = t - tc the analytic part is
    exp(-A u^2 / 2 + i w1 u), A = 1 / s^2 - i k, w1 = w0 + k tc, whose spectrum is exp(-(w - w1)^2 / (2 A) - i w tc): its
    logarithm is quadratic in w, the model d2 is derived for, and its group delay at w is tc + (w - w1) Im(1 / A).
    j + d2 equals that at w = 2 pi nu_i, on every strong bin (|W| >= 1e-2 max), within the model's 'fft'-against-'dft'
    disagreement there.  The signal is the table's chirp (0.02 -> 0.45 cycles/sample over 512 samples) under an envelope of
    40 samples, on every other of the scales 2 ... 15.7; measured: GMW 8.1e-10 sample against a disagreement of 1.2e-9,
    Morlet 2.4e-9 against 3.7e-9, where the first-order offset is wrong by 50 and 86 samples."""
    n, s = N, 40.0
    f0, f1 = F0, F1
    k = 2 * np.pi * (f1 - f0) / n
    t = np.arange(n, dtype=np.float64)
    x = np.exp(-0.5 * ((t - n / 2) / s) ** 2) * np.cos(2 * np.pi * f0 * t + 0.5 * k * t * t)
    sc = SCALES[0:FIT:2]
    nu = m.row_freqs(wavelet, sc)
    outs = [m.tssq_cwt_ref(x, wavelet, sc, padtype="zero", order=2, squeeze=False, arith=a, details=True)
            for a in ("fft", "dft")]
    (W, _, _, _, d), (_, _, _, _, dd) = outs
    big = np.abs(W) >= 1e-2 * np.abs(W).max()
    assert big.sum() > 1000 and d["use2"][big].all()
    w1 = 2 * np.pi * f0 + k * (n / 2)
    A = 1 / s ** 2 - 1j * k
    want = n / 2 + (2 * np.pi * nu[:, None] - w1) * (1 / A).imag
    got = t[None, :] + d["d2"]
    self_err = np.abs(d["d2"] - dd["d2"])[big].max()
    err = np.abs(got - want)[big].max()
    print("d2 against the analytic crossing time: %.3g samples; fft against dft: %.3g" % (err, self_err))
    assert err <= self_err
    # the first-order offset is biased: it names the envelope's centre of gravity under the wavelet, not the crossing
    assert np.abs(t[None, :] + d["d1"] - want)[big].max() > 10
