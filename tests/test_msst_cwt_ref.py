"""CPU tests of the numpy model of the multisynchrosqueezed CWT (tests/helpers/msst_cwt_ref.py): the table of
the design note, the invariants of the definition, and the bin -> row table rho."""
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import upstream as up
from tests.helpers import cwt_sst2_ref as m
from tests.helpers import msst_cwt_ref as r

ITERS = (1, 2, 4, 32)
# (order, grid, noise) -> the top-cell share at n_iter 1, 2, 4, 32, at the digits the model prints
TABLE = {
    (2, "peak", 0.0): (0.9455, 0.9949, 0.9980, 0.9981),
    (2, "maximal", 0.0): (0.9676, 0.9965, 0.9970, 0.9970),
    (1, "peak", 0.0): (0.6680, 0.7936, 0.8031, 0.8120),
    (1, "maximal", 0.0): (0.7140, 0.7849, 0.7998, 0.8028),
    (2, "peak", 0.3): (0.8181, 0.9167, 0.9230, 0.9214),
}


@functools.lru_cache(maxsize=None)
def run(order, grid, noise, n_iter):
    x, scales, f_asc, rc = r.fm_case(grid, noise)
    out = r.mssq_cwt_ref(x, r.FM_WAVELET, scales, f_asc, "log", None, rc, order=order, n_iter=n_iter)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("key", list(TABLE), ids=["o%d-%s-noise%g" % k for k in TABLE])
def test_model_table(key):
    shares = [r.top_cell_share(run(*key, n)[5]) for n in ITERS]
    print(key, " ".join("%.4f" % s for s in shares))
    assert shares[2] > shares[0]                                   # the share rises from n_iter 1 to 4
    assert ["%.4f" % s for s in shares] == ["%.4f" % s for s in TABLE[key]]


@pytest.mark.parametrize("key", list(TABLE), ids=["o%d-%s-noise%g" % k for k in TABLE])
def test_weighted_column_sums_are_unchanged_by_the_walk(key):
    """A coefficient keeps its own row weight wherever it lands: each column of Tx sums to the column's kept W rc.  Both
    sides add the same na terms in different orders: (na - 1) eps sum|terms| bounds either, so 2 na eps sum|W rc|."""
    _, _, _, rc = r.fm_case(key[1], key[2])
    eps = np.finfo(np.float64).eps
    for n in ITERS:
        W, w, b, rows, w_n, Tx = run(*key, n)
        terms = np.where(b >= 0, W * rc[:, None], 0)
        tol = 2 * len(W) * eps * np.abs(terms).sum(0)
        err = np.abs(Tx.sum(0) - terms.sum(0))
        print(n, "worst column: %.3g of its bound, %.3g of sum|terms|" % ((err / tol).max(), (err / np.abs(terms).sum(0)).max()))
        assert (err <= tol).all()
        assert np.array_equal(rows >= 0, b >= 0) and np.array_equal(np.isinf(w_n), b < 0)


@pytest.mark.parametrize("flipud", [False, True])
def test_one_step_is_the_second_order_model(flipud):
    x, scales, f_asc, rc = r.fm_case("maximal")
    W, w, b, rows, w_n, Tx = r.mssq_cwt_ref(x, r.FM_WAVELET, scales, f_asc, "log", None, rc, order=2, n_iter=1, flipud=flipud)
    W2, w2, b2, Tx2 = m.cwt_sst2_ref(x, r.FM_WAVELET, scales, f_asc, "log", None, rc, flipud=flipud)
    na = len(scales)
    assert np.array_equal(W, W2) and np.array_equal(w, w2) and np.array_equal(w_n, w2) and np.array_equal(Tx, Tx2)
    assert np.array_equal(np.where(b >= 0, na - 1 - b, -1) if flipud else b, b2)
    assert np.array_equal(rows, np.where(b >= 0, np.arange(na)[:, None], -1))


def test_the_walk_by_hand():
    """Three rows, two columns, rho the reversal: column 0 chains 0 -> row 1 -> row 2 (a fixed point), column 1 points at
    a row without a map."""
    rho = np.array([2, 1, 0])
    b = np.array([[1, 2], [0, -1], [0, 1]])          # row 0 -> bin 1 = row 1; row 1 -> bin 0 = row 2; row 2 -> bin 0 = row 2
    assert np.array_equal(r.walk_rows(b, rho, 1), [[0, 0], [1, -1], [2, 2]])
    assert np.array_equal(r.walk_rows(b, rho, 2), [[1, 0], [2, -1], [2, 2]])     # (column 1: row 0 -> bin 2 = row 0; row 2 -> row 1: no map)
    assert np.array_equal(r.walk_rows(b, rho, 3), [[2, 0], [2, -1], [2, 2]])
    assert np.array_equal(r.walk_rows(b, rho, 64), r.walk_rows(b, rho, 3))
    assert np.array_equal(r.walk_rows(np.stack([b, b]), rho, 3)[1], r.walk_rows(b, rho, 3))
    w = np.array([[1.0, 2.0], [3.0, np.inf], [5.0, 6.0]])
    assert np.array_equal(r.gather(w, r.walk_rows(b, rho, 3)), [[5.0, 2.0], [5.0, np.inf], [5.0, 6.0]])


# ---------------------------------------------------------------------------------------------------------------- rho
GMW = ("gmw", {"gamma": 3.0, "beta": 60.0})


def test_rho_is_the_reversal_on_a_peak_log_grid():
    x, scales, f_asc, rc = r.fm_case("peak")
    na = len(scales)
    assert np.array_equal(r.row_of_bin(r.row_freqs(r.FM_WAVELET, scales), f_asc), na - 1 - np.arange(na))
    # the library's own 'peak' grid (discrete peaks on the padded grid) is the reversal too, at any sampling rate
    for fs in (None, 1.0, 250.0):
        dt = 1.0 if fs is None else 1 / fs
        wcode, p0, p1 = up._wavelet(GMW)
        f_lib = up._cwt_freq_grid(scales, None, None, "peak", r.FM_N, wcode, p0, p1, dt)[2]
        rho = up.mssq_cwt_row_of_bin(GMW, scales, f_lib, fs)
        assert rho.dtype == np.int32 and np.array_equal(rho, na - 1 - np.arange(na))
        assert np.array_equal(rho, r.row_of_bin(r.row_freqs(r.FM_WAVELET, scales) / dt, f_lib))


def test_rho_on_a_maximal_grid_is_many_to_one_and_monotone():
    x, scales, f_asc, rc = r.fm_case("maximal")
    rho = r.row_of_bin(r.row_freqs(r.FM_WAVELET, scales), f_asc)
    assert (np.diff(rho) <= 0).all() and rho[0] == len(scales) - 1 and rho[-1] == 0
    assert len(np.unique(rho)) < len(rho)
    assert np.array_equal(up.mssq_cwt_row_of_bin(GMW, scales, f_asc), rho)
    lin = np.linspace(f_asc[0], f_asc[-1], len(f_asc))                   # log distance on a 'linear' grid too
    assert np.array_equal(up.mssq_cwt_row_of_bin(GMW, scales, lin), r.row_of_bin(r.row_freqs(r.FM_WAVELET, scales), lin))


def test_rho_takes_the_lowest_row_on_a_tie_and_the_lowest_frequency_for_no_frequency():
    nu = np.array([0.4, 0.1, 0.1, 0.025])                                # rows 1 and 2 coincide; 0.2 is midway in log2
    f = np.array([-1.0, 0.0, 0.1, 0.2])
    assert np.array_equal(r.row_of_bin(nu, f), [3, 3, 1, 0])
    assert abs(np.log2(0.4) - np.log2(0.2)) == abs(np.log2(0.1) - np.log2(0.2))         # (the tie is exact)
    wc = m.gmw_wc(3.0, 60.0)
    rho = up.mssq_cwt_row_of_bin(GMW, wc / (2 * np.pi * nu), f)
    nu_lib = up.tssq_cwt_row_freqs(GMW, wc / (2 * np.pi * nu))
    assert np.array_equal(rho, r.row_of_bin(nu_lib, f)) and rho[0] == rho[1] == 3 and rho[2] == 1
    with pytest.raises(ValueError):
        up.mssq_cwt_row_of_bin(GMW, np.ones(4), np.ones(3))
    with pytest.raises(ValueError):
        up.mssq_cwt_row_of_bin(GMW, np.ones(4), np.array([1.0, 2.0, np.nan, 3.0]))
