"""CPU checks of the ridge-extraction restatement (tests/helpers/ridge_oracle.py) on hand-checked cases of upstream's
quirks (old/ssqueezepy/ridge_extraction.py), and of `upstream.extract_ridges`' argument errors, which come before any
GPU call."""
import numpy as np
import pytest

from tests.helpers import ridge_oracle as ro


def test_upstream_test_basic():
    """old/tests/ridge_extraction_test.py:17-26."""
    m = np.array([[1, 4, 4], [2, 2, 2], [5, 5, 4]])
    idx, f, e = ro.extract_ridges(m, np.exp([1, 2, 3]), penalty=2.0, get_params=True)
    assert np.array_equal(idx, [[2], [2], [2]])
    assert f.dtype == np.float32 and e.dtype == np.float32          # int input: float32 parameters (:113-114)
    assert np.array_equal(e[:, 0], [25, 25, 16])


def test_band_slice_wraps_when_ridge_is_below_bw():
    """energy[int(r - bw):int(r + bw), t] = 0 (:143): r = 1, bw = 2 gives energy[-1:3] -- empty, so the second ridge
    is the first again; r = 3, bw = 2 zeroes rows 1..4 and leaves row 5."""
    F, N = 8, 10                                     # N > F: no modulo (:164-165) in the way
    Tf = np.full((F, N), 0.1)
    Tf[1] = 10.0
    idx = ro.extract_ridges(Tf, np.arange(1, F + 1), n_ridges=2, bw=2, transform="stft")
    assert np.array_equal(idx[:, 0], [1] * N) and np.array_equal(idx[:, 1], [1] * N)
    Tf = np.full((F, N), 0.1)
    Tf[3], Tf[5], Tf[6] = 10.0, 5.0, 1.0
    idx = ro.extract_ridges(Tf, np.arange(1, F + 1), n_ridges=2, bw=2, transform="stft")
    assert np.array_equal(idx[:, 0], [3] * N) and np.array_equal(idx[:, 1], [5] * N)


def test_all_zero_column_starts_a_nan_chain():
    """0 / 0 = NaN cost (:133); np.amin propagates it, so every later column is NaN; argmin then returns the first
    NaN (row 0) and the backward test never matches a NaN, keeping the forward index."""
    rng = np.random.default_rng(0)
    Tf = rng.standard_normal((6, 7)) + 1j * rng.standard_normal((6, 7))
    Tf[:, 3] = 0
    scales = np.exp(np.arange(6) / 4)
    idx, costs = ro.extract_ridges(Tf, scales, return_costs=True)
    cost = costs[0]
    assert np.isnan(cost[:, 3]).all() and not np.isnan(np.delete(cost, 3, axis=1)).any()
    P = ro.penalty_matrix(ro.metric(scales, np.float64), 2.0, np.float64)
    pen, fwd = ro.forward(cost, P)
    assert np.isnan(pen[:, 3:]).all() and not np.isnan(pen[:, :3]).any()
    assert np.array_equal(fwd[3:], [0] * 4)
    assert np.array_equal(idx[3:, 0], [0] * 4)


def test_forward_index_is_reduced_modulo_n_when_f_exceeds_n():
    """unravel_index(argmin(pen, axis=0), (F, N))[1] (:164-165) = argmin mod N."""
    F, N = 7, 2
    cost = np.ones((F, N))
    cost[5, :] = -1.0                                # argmin row 5 in both columns -> 5 mod 2 = 1
    P = np.zeros((F, F))
    pen, fwd = ro.forward(cost, P)
    assert np.array_equal(fwd, [1, 1])


def test_ties_first_index_forward_last_match_backward():
    """argmin takes the first of equal minima; the serial backward loop overwrites, so the LAST row within eps wins."""
    F, N = 5, 4
    cost = np.zeros((F, N), dtype=np.float32)
    P = np.zeros((F, F), dtype=np.float32)
    pen, fwd = ro.forward(cost, P)
    assert np.array_equal(fwd, [0] * N)
    ridge = ro.backward(cost, P, pen, fwd, np.float32(ro.EPS32))
    assert np.array_equal(ridge, [F - 1] * (N - 1) + [0])


def test_backward_keeps_forward_index_when_nothing_matches():
    cost = np.zeros((3, 2))
    P = np.zeros((3, 3))
    pen = np.array([[0.0, 5.0], [0.0, 5.0], [0.0, 5.0]])       # val = 5 matches no pen[f, 0] + P = 0
    assert np.array_equal(ro.backward(cost, P, pen, np.array([2, 1]), ro.EPS64), [2, 1])


def test_mixed_dtype_case_is_fp64_cost_with_fp32_penalty():
    """float64 real Tf: energy and DP in fp64, P and eps float32 values (:113-121)."""
    Tf = np.random.default_rng(1).standard_normal((4, 5))
    assert ro.param_dtype(Tf) == np.float32
    P = ro.penalty_matrix(ro.metric(np.exp(np.arange(4) / 3), np.float32), 2.0, np.float32)
    assert P.dtype == np.float32
    energy = np.abs(Tf) ** 2
    cost = -np.log(energy / energy.max(axis=0) + np.float32(ro.EPS32))
    assert cost.dtype == np.float64
    pen, _ = ro.forward(cost, P)
    assert pen.dtype == np.float64


@pytest.mark.parametrize("kw, shape", [
    (dict(scales=np.exp(np.arange(5))), (4, 8)),            # len(scales) != F
    (dict(scales=np.exp(np.arange(4)), n_ridges=0), (4, 8)),
    (dict(scales=np.exp(np.arange(4)), bw=-1), (4, 8)),
    (dict(scales=np.exp(np.arange(4)).reshape(2, 2)), (4, 8)),
    (dict(scales=np.exp(np.arange(4))), (8,)),               # Tf must be 2-D or 3-D
])
def test_extract_ridges_argument_errors_come_before_the_gpu(monkeypatch, kw, shape):
    from ssqueeze_rs_amd import _lib
    from ssqueeze_rs_amd import upstream as up

    def no_gpu():
        raise AssertionError("the GPU was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    with pytest.raises(ValueError):
        up.extract_ridges(np.ones(shape, dtype=np.complex64), **kw)
