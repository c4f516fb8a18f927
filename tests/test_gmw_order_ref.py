"""CPU checks of the higher-order GMW pieces: the restated order-k wavelet (tests/helpers/gmw_order_ref.py) against an
independent construction from generalized Laguerre polynomials (Olhede & Walden 2002), and the host coefficients the
mirror hands to the library (`upstream.gmw_k_constants`, `upstream.gmw_order_coefficients`)."""
import math
import warnings

import numpy as np
import pytest

from oracle import upstream_oracle as u
from tests.helpers import gmw_order_ref as g

PAIRS = [(3.0, 60.0), (4.0, 80.0), (3.0, 6.0)]


def _grid(gamma, beta):
    wc = u.morsefreq(gamma, beta)
    return np.concatenate([[-1.0, 0.0], np.linspace(1e-3, 3 * wc, 801)])


def _laguerre_gmw(w, gamma, beta, k):
    """2 sqrt(G(r) G(k+1) / G(k+r)) L_k^{(r-1)}(2 w^gamma) * envelope, the bandpass-normalised order-k GMW."""
    from scipy.special import genlaguerre
    r = (2 * beta + 1) / gamma
    norm = 2 * math.sqrt(math.exp(math.lgamma(r) + math.lgamma(k + 1) - math.lgamma(k + r)))
    wc = u.morsefreq(gamma, beta)
    w = np.asarray(w, dtype=np.float64)
    out = np.zeros_like(w)
    p = w > 0
    env = np.exp(-beta * np.log(wc) + wc ** gamma + beta * np.log(w[p]) - w[p] ** gamma)
    out[p] = norm * genlaguerre(k, r - 1)(2 * w[p] ** gamma) * env
    return out


@pytest.mark.parametrize("gamma,beta", PAIRS)
@pytest.mark.parametrize("k", range(5))
def test_gmw_l1_k_equals_the_laguerre_construction(gamma, beta, k):
    """1e-12 relative to the sum of the absolute polynomial terms: upstream's power-basis sum cancels (terms up to ~1e3
    times the result at k = 4, beta = 60), and its lgamma-based constants carry ~1e-14, so near the peak the value itself
    is only good to ~2e-10 (checked against a 50-digit Laguerre evaluation).  Plain relative 1e-12 holds up to k = 2."""
    w = _grid(gamma, beta)
    a = g.gmw_l1_k(w, gamma, beta, k)
    b = _laguerre_gmw(w, gamma, beta, k)
    kc = g.gmw_k_constants(gamma, beta, k)
    wp = np.maximum(w, 0)
    absterms = sum(abs(kc[m]) * (2 * wp ** gamma) ** m for m in range(k + 1)) * np.abs(g.gmw_l1_k(w, gamma, beta, 0)) / 2
    assert np.abs(a - b).max() <= 1e-12 * absterms.max()
    if k <= 2:
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    assert a[0] == 0.0 and a[1] == 0.0


@pytest.mark.parametrize("gamma,beta", PAIRS)
def test_order_zero_is_the_order_zero_wavelet(gamma, beta):
    w = _grid(gamma, beta)
    b = u.gmw_l1(w, gamma, beta)
    assert np.abs(g.gmw_l1_k(w, gamma, beta, 0) - b).max() <= 1e-14 * np.abs(b).max()
    assert np.array_equal(g.gmw_k_constants(gamma, beta, 0), [2.0])


@pytest.mark.parametrize("gamma,beta", PAIRS)
def test_mirror_constants_equal_the_restatement(gamma, beta):
    from ssqueeze_rs_amd import upstream as up
    for k in range(up.GMW_MAX_ORDER + 1):
        a, b = up.gmw_k_constants(gamma, beta, k), g.gmw_k_constants(gamma, beta, k)
        assert a.shape == (k + 1,) and np.abs(a - b).max() <= 1e-13 * np.abs(b).max()
    assert np.array_equal(up.gmw_k_constants(gamma, beta, 0), [2.0])


@pytest.mark.parametrize("gamma,beta", PAIRS)
@pytest.mark.parametrize("orders", [(0, 1, 2), range(3), (1, 4), (2, 2, 0, 3)])
def test_averaged_polynomial_is_the_mean_of_the_order_wavelets(gamma, beta, orders):
    """the linearity the single-table averaged transform rests on: one polynomial whose psih is the per-order mean."""
    from ssqueeze_rs_amd import upstream as up
    w = _grid(gamma, beta)
    poly = up.gmw_order_coefficients(gamma, beta, orders)
    assert poly.shape == (1, max(orders) + 1)
    wc = u.morsefreq(gamma, beta)
    y = 2 * np.maximum(w, 0) ** gamma
    with np.errstate(divide="ignore"):
        env = np.where(w > 0, np.exp(-beta * np.log(wc) + wc ** gamma + beta * np.log(np.maximum(w, 0)) -
                                     np.maximum(w, 0) ** gamma), 0.0)
    mine = np.polynomial.polynomial.polyval(y, poly[0]) * env
    ref = np.mean([g.gmw_l1_k(w, gamma, beta, k) for k in orders], axis=0)
    assert np.abs(mine - ref).max() <= 1e-12 * np.abs(ref).max()
    per = up.gmw_order_coefficients(gamma, beta, orders, average=False)
    assert per.shape == (len(orders), max(orders) + 1)
    for i, k in enumerate(orders):
        assert np.array_equal(per[i, :k + 1], up.gmw_k_constants(gamma, beta, k)) and not per[i, k + 1:].any()


def test_restated_per_order_average_equals_the_averaged_wavelet_transform():
    """cwt_higher_order's mean of K outputs (the restatement) equals one transform with the mean wavelet (linearity)."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal(300)
    sc = 2 ** (np.arange(8, 40) / 8)
    Wm, dWm = g.cwt_higher_order(x, sc, 3.0, 20.0, (0, 1, 2), derivative=True, fs=2.0)
    fn = lambda w: np.mean([g.gmw_l1_k(w, 3.0, 20.0, k) for k in range(3)], axis=0)     # noqa: E731
    W1, dW1 = g.cwt_psih(x, fn, sc, fs=2.0, derivative=True)
    assert np.abs(Wm - W1).max() <= 1e-13 * np.abs(W1).max()
    assert np.abs(dWm - dW1).max() <= 1e-13 * np.abs(dW1).max()
    lst = g.cwt_higher_order(x, sc, 3.0, 20.0, (0, 1, 2), average=False)
    assert isinstance(lst, list) and len(lst) == 3 and lst[0].shape == (len(sc), 300)


def test_order_argument_rules_without_a_gpu():
    """the option checks run before any device work: upstream's return-shape rules and the ValueErrors."""
    from ssqueeze_rs_amd import upstream as up
    assert up._order_args(0, None, "gmw") is None
    assert up._order_args(2, None, "gmw") == ((2,), False)
    assert up._order_args((0, 1, 2), None, "gmw") == ((0, 1, 2), True)
    assert up._order_args(range(3), False, "gmw") == ((0, 1, 2), False)
    assert up._order_args([1, 2], None, "gmw") == ((1, 2), True)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert up._order_args((2,), True, "gmw") == ((2,), False)
    assert len(rec) == 1
    for bad in (dict(order=1, wavelet="morlet"), dict(order=(0, 1), wavelet=("morlet", {"mu": 13.4})),
                dict(order=-1, wavelet="gmw"), dict(order=(0, -2), wavelet="gmw"),
                dict(order=up.GMW_MAX_ORDER + 1, wavelet="gmw"), dict(order=1.5, wavelet="gmw")):
        with pytest.raises(ValueError):
            up._order_args(bad["order"], None, bad["wavelet"])
    with pytest.raises(ValueError):
        up._order_args(1, None, "gmw", l1_norm=False)
    with pytest.raises(ValueError):
        up._wavelet(("gmw", {"order": 1}))


def test_gmwk_entry_points_reject_bad_arguments_with_an_error_code():
    """argument checks of ssq_cwt_host_gmwk / ssq_ssq_cwt_host_gmwk / ssq_cwt_plan_create_gmwk come before any device
    work: a non-zero status and ssq_last_error, never a crash."""
    import ctypes as C
    from ssqueeze_rs_amd import _lib
    lib = _lib.load()
    x = np.zeros(64)
    sc = 2.0 ** (np.arange(8, 24) / 8)
    W = np.zeros((2, 16, 64), dtype=np.complex128)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None                 # noqa: E731
    ok = np.array([2.0, -1.0])
    cases = [(ok, 2, 1, 1, None), (None, 2, 1, 1, "NULL"), (np.zeros(18), 18, 1, 1, "n_coeffs"),
             (ok, 0, 1, 1, "n_coeffs"), (ok, 2, 0, 1, "n_groups"), (ok, 2, 1, 0, "UPSTREAM"),
             (np.array([2.0, np.nan]), 2, 1, 1, "finite")]
    for coeffs, n, groups, variant, msg in cases[1:]:
        rc = lib.ssq_cwt_host_gmwk(1, ptr(x), 1, 64, 3.0, 60.0, ptr(coeffs), n, groups, ptr(sc), len(sc), 1.0, 1, 0, 0,
                                   variant, ptr(W), None)
        assert rc != 0 and msg in lib.ssq_last_error().decode(), msg
        plan = C.c_void_p()
        rc = lib.ssq_cwt_plan_create_gmwk(C.byref(plan), 1, 64, 3.0, 60.0, ptr(coeffs), n, groups, ptr(sc), len(sc), 1.0,
                                          0, variant)
        assert rc != 0 and msg in lib.ssq_last_error().decode() and not plan.value
    big = np.ones(2 * 20000)
    rc = lib.ssq_cwt_host_gmwk(1, ptr(x), 1, 64, 3.0, 60.0, ptr(big), 2, 20000, ptr(sc), 2, 1.0, 1, 0, 0, 1, ptr(W), None)
    assert rc != 0 and "32767" in lib.ssq_last_error().decode()
    f = np.linspace(0.1, 0.4, len(sc))
    rc = lib.ssq_ssq_cwt_host_gmwk(1, ptr(x), 1, 64, 3.0, 60.0, ptr(np.ones(4)), 2, 2, ptr(sc), len(sc), 1.0, 8, ptr(f),
                                   0, 0, 0, -1.0, 1, ptr(W), None, None, None)
    assert rc != 0 and "n_groups" in lib.ssq_last_error().decode()
