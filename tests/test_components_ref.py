"""CPU tests of the component inversion (`upstream.issq_cwt` / `issq_stft` with `cc`, `cw`): the NumPy restatement
tests/helpers/components_ref.py on hand-made cases, the argument errors the mirror raises before any GPU work, and
the two C-ABI entry points."""
import ctypes as C

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.helpers import components_ref as cr

F = 6


def _powers(N=1):
    """Tx whose column sums name their rows: Re Tx[r] = 10**r (and an imaginary part that must not count)."""
    re = (10.0 ** np.arange(F))[:, None] * np.ones((1, N))
    return (re + 1j * 7.0).astype(np.complex128)


def _rows(*rows):
    return float(sum(10.0 ** r for r in rows))


def _slice_sum(col, lo, hi):
    return float(np.sum(col[slice(lo, hi + 1)]))


@pytest.mark.parametrize("cc, cw, comps, rem", [
    ([2, 3], [1, 1], [(1, 2, 3), (2, 3, 4)], (0, 5)),          # overlapping bands: rows 2, 3 count twice
    ([-1, 2], [3, 0], [(), (2,)], (0, 1, 3, 4, 5)),            # cc == -1: no band; cw = 0: one row
    ([-5], [2], [(0,)], (1, 2, 3, 4, 5)),                      # other negatives clip: row 0
    ([-1], [0], [()], (0, 1, 2, 3, 4, 5)),
    ([F + 4], [1], [()], tuple(range(F))),                     # cc >= F: lo = hi = F, an empty slice
    ([F], [1], [(5,)], (0, 1, 2, 3, 4)),                       # hi clipped at F, cut at F - 1
    ([3], [-1], [()], tuple(range(F))),                        # negative cw: lo > hi
    ([0], [100], [tuple(range(F))], ()),
])
def test_restatement_on_hand_made_bands(cc, cw, comps, rem):
    Tx = _powers()
    x = cr.invert_components(Tx, np.array([cc]), np.array([cw]))
    assert x.shape == (len(cc) + 1, 1) and x.dtype == np.float64
    for k, rows in enumerate(comps):
        assert x[k, 0] == _rows(*rows)
    assert x[-1, 0] == _rows(*rem)


def test_restatement_truncates_float_curves():
    x = cr.invert_components(_powers(2), np.array([2.9, -1.5]), np.array([1.7, 0.2]))   # 1-D: one curve
    assert x.shape == (2, 2)
    assert x[0, 0] == _rows(1, 2, 3)                            # (2, 1): rows 1 .. 3
    assert x[0, 1] == 0.0                                       # -1.5 -> -1: no curve
    assert x[1, 1] == _rows(*range(F))


def test_restatement_matches_python_slices_on_random_curves():
    rng = np.random.default_rng(3)
    Fr, N, K = 9, 50, 4
    Tx = rng.standard_normal((Fr, N)) + 1j * rng.standard_normal((Fr, N))
    cc = rng.integers(-3, Fr + 3, size=(N, K))
    cc[rng.random((N, K)) < 0.2] = -1
    cw = rng.integers(-1, 4, size=(N, K))
    x = cr.invert_components(Tx, cc, cw)
    for m in range(N):
        col = Tx[:, m].real
        left = np.ones(Fr, dtype=bool)
        for k in range(K):
            lo, hi = int(np.clip(cc[m, k] - cw[m, k], 0, Fr)), int(np.clip(cc[m, k] + cw[m, k], 0, Fr))
            if cc[m, k] == -1:
                lo, hi = 1, 0
            assert x[k, m] == pytest.approx(_slice_sum(col, lo, hi), abs=1e-12)
            left[slice(lo, hi + 1)] = False
        assert x[K, m] == pytest.approx(float(np.sum(col[left])), abs=1e-12)


def test_disjoint_bands_add_up_to_the_full_column_sum():
    rng = np.random.default_rng(5)
    Fr, N = 40, 64
    Tx = rng.standard_normal((Fr, N)) + 1j * rng.standard_normal((Fr, N))
    cc = np.stack([rng.integers(3, 10, N), rng.integers(20, 30, N)], axis=1)
    cw = np.full_like(cc, 3)
    x = cr.invert_components(Tx, cc, cw)
    assert np.abs(x.sum(axis=0) - Tx.real.sum(axis=0)).max() <= 1e-12 * np.abs(Tx.real).sum(axis=0).max()


def test_restatement_sums_the_remainder_in_the_dtype_of_tx():
    Tx = np.array([[1.0 + 0j], [2.0 ** -30], [1.0]], dtype=np.complex64)
    x = cr.invert_components(Tx, np.array([0]), np.array([0]))
    assert x[1, 0] == np.float32(2.0 ** -30) + np.float32(1.0)      # fp32 sum of the uncovered rows


# ---- argument errors the mirror raises before it looks for a GPU ----------------------------------------------------
def _tx(F_=8, N=5, dt=np.complex64):
    return np.zeros((F_, N), dtype=dt)


@pytest.mark.parametrize("fn", ["cwt", "stft"])
@pytest.mark.parametrize("Tx, cc, cw, err", [
    (_tx(), np.zeros(5), None, ValueError),                      # only one of cc / cw
    (_tx(), None, np.zeros(5), ValueError),
    (_tx(), np.zeros(4), np.zeros(4), ValueError),               # one row per column of Tx
    (_tx(), np.zeros((5, 3)), np.zeros((5, 2)), ValueError),     # cw needs K columns
    (_tx(), np.zeros((5, 0)), np.zeros((5, 0)), ValueError),     # no component
    (_tx(), np.zeros((5, 2)), np.zeros((3, 2)), ValueError),     # cw rows neither N nor 1
    (_tx(), np.zeros((1, 5, 2)), np.zeros((1, 5, 2)), ValueError),
    (_tx(), np.zeros(()), np.zeros(()), ValueError),
    (np.zeros((2, 8, 5), np.complex64), np.zeros((5, 1)), np.zeros((5, 1)), ValueError),   # batched: [B, N(, K)]
    (np.zeros((8, 5)), np.zeros(5), np.zeros(5), TypeError),     # Tx must be complex
    (np.zeros((2, 2, 8, 5), np.complex64), np.zeros(5), np.zeros(5), TypeError),
])
def test_argument_errors_come_before_the_gpu(fn, Tx, cc, cw, err):
    with pytest.raises(err):
        if fn == "cwt":
            up.issq_cwt(Tx, "gmw", cc=cc, cw=cw)
        else:
            up.issq_stft(Tx, np.hanning(2 * (Tx.shape[-2] - 1)) + 0.1, cc=cc, cw=cw)


def test_issq_stft_checks_its_own_arguments_first():
    with pytest.raises(ValueError, match="modulated"):
        up.issq_stft(_tx(), np.hanning(14), cc=np.zeros(4), cw=None, modulated=False)
    with pytest.raises(ValueError, match="hop_len"):
        up.issq_stft(_tx(), np.hanning(14), cc=np.zeros(4), cw=None, hop_len=2)


# ---- the C-ABI -------------------------------------------------------------------------------------------------------
NEW = ("ssq_issq_components_exec", "ssq_issq_components_host")


def test_new_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib._SIGNATURES and name in _lib.header_symbols()
        assert hasattr(lib, name)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_host_entry_rejects_bad_arguments_with_last_error():
    lib = _lib.load()
    T = np.zeros((4, 3), dtype=np.complex128)
    cc = np.zeros((3, 2), dtype=np.int64)
    cw = np.zeros((3, 2), dtype=np.int64)
    x = np.zeros((3, 3))
    cases = [
        ((_lib.SSQ_F64, _vp(T), 1, 4, 3, _vp(cc), _vp(cw), 0, 0, 1.0, _vp(x)), b"n_comp"),
        ((_lib.SSQ_F64, _vp(T), 1, 0, 3, _vp(cc), _vp(cw), 0, 2, 1.0, _vp(x)), b"rows"),
        ((_lib.SSQ_F64, _vp(T), 0, 4, 3, _vp(cc), _vp(cw), 0, 2, 1.0, _vp(x)), b"batch"),
        ((_lib.SSQ_F64, _vp(T), 1, 4, 0, _vp(cc), _vp(cw), 0, 2, 1.0, _vp(x)), b"cols"),
        ((7, _vp(T), 1, 4, 3, _vp(cc), _vp(cw), 0, 2, 1.0, _vp(x)), b"dtype"),
        ((_lib.SSQ_F64, None, 1, 4, 3, _vp(cc), _vp(cw), 0, 2, 1.0, _vp(x)), b"NULL"),
        ((_lib.SSQ_F64, _vp(T), 1, 4, 3, _vp(cc), None, 1 << 31, 2, 1.0, _vp(x)), b"cw_const"),
    ]
    for args, msg in cases:
        assert lib.ssq_issq_components_host(*args) != 0
        assert msg in lib.ssq_last_error()
    for arr, name in ((cc, b"cc"), (cw, b"cw")):
        for v in (1 << 31, -(1 << 31) - 1):
            arr[1, 1] = v
            assert lib.ssq_issq_components_host(_lib.SSQ_F64, _vp(T), 1, 4, 3, _vp(cc), _vp(cw), 0, 2, 1.0,
                                                _vp(x)) != 0
            assert b"|" + name + b"|" in lib.ssq_last_error()
        arr[1, 1] = 0
