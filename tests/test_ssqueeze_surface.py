"""CPU tests of `upstream.ssqueeze`, `phase_cwt` and `phase_stft`: upstream's signatures (ssqueezing.py:13-16,
_ssq_cwt.py:420, _ssq_stft.py:200), the refused options raising ValueError before any GPU work, and the NumPy
restatement tests/helpers/ssqueeze_ref.py on hand-computed cases."""
import inspect

import numpy as np
import pytest

from ssqueeze_rs_amd import upstream as up
from tests.helpers import ssqueeze_ref as ref


def _sig(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


E = inspect.Parameter.empty


def test_signatures_match_upstream():
    assert _sig(up.ssqueeze) == [
        ("Wx", E), ("w", None), ("ssq_freqs", None), ("scales", None), ("Sfs", None), ("fs", None), ("t", None),
        ("squeezing", "sum"), ("maprange", "maximal"), ("wavelet", None), ("gamma", None), ("was_padded", True),
        ("flipud", False), ("dWx", None), ("transform", "cwt")]
    assert _sig(up.phase_cwt) == [("Wx", E), ("dWx", E), ("difftype", "trig"), ("gamma", None), ("parallel", None)]
    assert _sig(up.phase_stft) == [("Sx", E), ("dSx", E), ("Sfs", E), ("gamma", None), ("parallel", None)]


@pytest.fixture
def no_gpu(monkeypatch):
    def refuse():
        raise AssertionError("GPU touched before the argument check")
    monkeypatch.setattr(up._lib, "require_gpu", refuse)


def _maps(F=8, N=16, dtype=np.complex128):
    rng = np.random.default_rng(0)
    Wx = (rng.standard_normal((F, N)) + 1j * rng.standard_normal((F, N))).astype(dtype)
    dWx = (rng.standard_normal((F, N)) + 1j * rng.standard_normal((F, N))).astype(dtype)
    return Wx, dWx


S8 = 2.0 ** (np.arange(8) / 4 + 1)


@pytest.mark.parametrize("kw, word", [
    (dict(maprange="energy"), "maprange"),
    (dict(maprange=(0.1, 0.4)), "maprange"),
    (dict(maprange="nope"), "maprange"),
    (dict(squeezing="lebesgue", w=None), "squeezing"),
    (dict(squeezing="abs", w=None), "squeezing"),
    (dict(squeezing=lambda x: x, w=None), "squeezing"),
    (dict(squeezing="bogus"), "squeezing"),
    (dict(transform="stft", ssq_freqs=None), "ssq_freqs"),
    (dict(transform="stft", ssq_freqs="linear"), "ssq_freqs"),
    (dict(transform="stft", ssq_freqs=np.linspace(0, .5, 8), w=None, Sfs=None), "Sfs"),
    (dict(transform="stft", ssq_freqs=np.linspace(.1, .5, 8), w=None, Sfs=np.linspace(0, .5, 8)), "Sfs[0]"),
    (dict(transform="fft"), "transform"),
    (dict(scales=None), "scales"),
    (dict(ssq_freqs="log-piecewise", maprange="maximal"), "log-piecewise"),
    (dict(maprange="peak", ssq_freqs="log", wavelet=None), "wavelet"),
    (dict(w="negative"), "negatives"),
    (dict(w=None, dWx=None), "dWx"),
])
def test_refused_options_raise_before_the_gpu(no_gpu, kw, word):
    Wx, dWx = _maps()
    args = dict(w=np.abs(Wx.real), scales=S8, dWx=dWx)
    args.update(kw)
    if isinstance(args["w"], str):
        args["w"] = -np.abs(Wx.real)
    with pytest.raises(ValueError, match=word.replace("[", r"\[")):
        up.ssqueeze(Wx, **args)


def test_phase_refusals(no_gpu):
    Wx, dWx = _maps()
    with pytest.raises(ValueError, match="difftype"):
        up.phase_cwt(Wx, dWx, difftype="phase")
    with pytest.raises(ValueError, match="dWx"):
        up.phase_cwt(Wx, dWx[:4])
    with pytest.raises(ValueError, match="Sfs"):
        up.phase_stft(Wx, dWx, np.linspace(0, .5, 5))
    with pytest.raises(TypeError):
        up.phase_cwt(Wx.real, dWx)


# ---- the restatement on hand-computed cases
def test_restatement_linear_ties_round_half_to_even_and_clamp():
    f = np.array([0.0, 1.0, 2.0, 3.0])
    # w = 0.5 -> bin 0, 1.5 -> 2, 2.5 -> 2, -> 9 clamps to 3, 0.49 -> 0
    w = np.array([[0.5], [1.5], [2.5], [9.0]])
    Wx = np.array([[1.0], [10.0], [100.0], [1000.0]], dtype=np.complex128)
    Tx = ref.indexed_sum(Wx, w, f, 1.0, False, False)
    np.testing.assert_array_equal(Tx[:, 0], [1, 0, 110, 1000])
    Tf = ref.indexed_sum(Wx, w, f, 1.0, False, True)                 # flipud: k -> 3 - k
    np.testing.assert_array_equal(Tf[:, 0], [1000, 110, 0, 1])


def test_restatement_skips_inf_and_weights_rows():
    f = np.array([1.0, 2.0, 4.0, 8.0])                               # log2: 0, 1, 2, 3
    w = np.array([[2.0, np.inf], [np.inf, 8.0], [4.0, 1.0], [2.0 ** 0.25, 2.0 ** 2.25]])
    Wx = np.ones((4, 2), dtype=np.complex128) * (1 + 2j)
    c = np.array([1.0, 2.0, 3.0, 4.0])
    Tx = ref.indexed_sum(Wx, w, f, c, True, False)
    # col 0: row0 -> bin 1 (x1), row2 -> bin 2 (x3), row3 log2 = .25 -> bin 0 (x4); col 1: row1 -> 3 (x2),
    # row2 -> 0 (x3), row3 log2 = 2.25 -> 2 (x4)
    np.testing.assert_array_equal(Tx[:, 0], np.array([4, 1, 3, 0]) * (1 + 2j))
    np.testing.assert_array_equal(Tx[:, 1], np.array([3, 0, 4, 2]) * (1 + 2j))


def test_restatement_fast_path_keeps_strictly_above_gamma():
    Wx = np.array([[1.0 + 0j], [0.5 + 0j]])
    dWx = np.array([[2j * np.pi * 1.0], [2j * np.pi * 0.5 * 2.0]])   # w = 1 and 2
    f = np.array([1.0, 2.0])
    T_eq = ref.ssqueeze_fast(Wx, dWx, f, 1.0, False, False, gamma=0.5)   # |Wx| == gamma on row 1: dropped
    np.testing.assert_array_equal(T_eq[:, 0], [1, 0])
    w = ref.phase_cwt(Wx, dWx, gamma=0.5)                                 # the phase function keeps it
    np.testing.assert_allclose(w[:, 0], [1, 2])
    np.testing.assert_array_equal(ref.indexed_sum(Wx, w, f, 1.0, False, False)[:, 0], [1, 0.5])
    assert np.isinf(ref.phase_cwt(Wx, dWx, gamma=0.6)[1, 0])


def test_restatement_log_piecewise_two_segments():
    # two exponential segments: ratio 2 below the transition, 2**(1/4) above it
    f = np.hstack([2.0 ** np.arange(4), 8 * 2.0 ** (np.arange(1, 9) / 4)])
    idx = ref.transition_idx(f)
    assert idx == 4
    p = ref.bin_params(f, True)
    assert p[0] == "pw" and p[2] == 3.0 and p[5] == 3 and p[4] == .25 and p[3] == 1.0
    wl = np.array([0.4, 0.6, 1.5, 2.5, 3.0, 3.1, 3.13, 3.2, 5.0, 9.0])
    k = ref.bins(2.0 ** wl[:, None], p, len(f) - 1, False)[:, 0]
    # log2 w <= vlmin1 = 3: first segment, rint(log2 w); above: 3 + rint((log2 w - 3) / .25), clamped at 11
    expect = [0, 1, 2, 2, 3, 3, 4, 4, 11, 11]
    np.testing.assert_array_equal(k, expect)
    kf = ref.bins(2.0 ** wl[:, None], p, len(f) - 1, True)[:, 0]
    np.testing.assert_array_equal(kf, 11 - np.array(expect))


def test_restatement_squeezing_modes():
    Wx = np.array([[3 + 4j, 1j], [1 + 0j, -2 + 0j]])
    w = np.array([[1.0, 1.0], [0.0, np.inf]])
    f = np.array([0.0, 1.0])
    assert ref.ssqueeze(Wx, w, f, 1.0, "linear", "abs").dtype == np.float64
    np.testing.assert_array_equal(ref.ssqueeze(Wx, w, f, 1.0, "linear", "abs"), [[1, 0], [5, 1]])
    np.testing.assert_array_equal(ref.ssqueeze(Wx, w, f, 2.0, "linear", "lebesgue"), [[1, 0], [1, 1]])
    np.testing.assert_array_equal(ref.ssqueeze(Wx, w, f, 1.0, "linear", lambda x: x * 2), [[2, 0], [6 + 8j, 2j]])
