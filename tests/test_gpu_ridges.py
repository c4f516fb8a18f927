"""GPU ridge extraction (`upstream.extract_ridges`, ridge.hip) against the numba-free restatement
tests/helpers/ridge_oracle.py: the forward DP bitwise, the costs to a few ulp, the ridges exactly."""
import ctypes as C

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.helpers import ridge_oracle as ro

pytestmark = pytest.mark.gpu

MODES = {   # name -> (cost dtype, parameter dtype, eps)
    "fp32": (np.float32, np.float32, ro.EPS32),
    "fp64": (np.float64, np.float64, ro.EPS64),
    "mixed": (np.float64, np.float32, ro.EPS32),
}


def _code(dt):
    return _lib.SSQ_F64 if dt == np.float64 else _lib.SSQ_F32


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _track_gpu(cost, m, penalty, cdt, pdt):
    """ssq_ridge_track_host on cost [B][F][N] -> (pen [B][F][N], ridge [B][N])."""
    cost = np.ascontiguousarray(cost, dtype=cdt)
    B, F, N = cost.shape
    pen = np.empty_like(cost)
    ridge = np.empty((B, N), dtype=np.int64)
    m = np.ascontiguousarray(m, dtype=pdt)
    rc = _lib.load().ssq_ridge_track_host(_code(cdt), _code(pdt), _vp(cost), B, F, N, _vp(m),
                                          float(pdt(penalty)), _vp(ridge), _vp(pen))
    _lib.check(rc)
    return pen, ridge


def _same_bits(a, b):
    """NaN exactly where the other has NaN (payloads differ between hosts), every other value bitwise."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint8), b[~nb].view(np.uint8))


def _costs(kind, F, N, cdt, rng):
    c = rng.standard_normal((F, N)).astype(cdt) ** 2 * cdt(3)
    if kind == "nan":
        c[:, N // 2] = np.nan
    elif kind == "const":
        c[:, 1::3] = cdt(0.5)
    return c


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind, F, N", [("random", 37, 60), ("random", 256, 40), ("nan", 20, 30),
                                        ("const", 16, 50), ("random", 300, 5)])
def test_dp_is_exact(mode, kind, F, N):
    cdt, pdt, eps = MODES[mode]
    rng = np.random.default_rng(F * 1000 + N)
    cost = _costs(kind, F, N, cdt, rng)
    m = ro.metric(np.exp(np.linspace(0, 3, F)), pdt)
    P = ro.penalty_matrix(m, 2.0, pdt)
    pen_o, ridge_o = ro.track(cost, P, pdt(eps))
    pen, ridge = _track_gpu(cost[None], m, 2.0, cdt, pdt)
    assert _same_bits(pen[0], pen_o)
    assert np.array_equal(ridge[0], ridge_o)


def test_dp_is_exact_when_the_column_exceeds_lds():
    """F = 7000 fp64: the previous column (2 x 56 KB) plus the metric do not fit in LDS; F > N exercises mod N."""
    cdt = pdt = np.float64
    rng = np.random.default_rng(7)
    F, N = 7000, 3
    cost = _costs("random", F, N, cdt, rng)
    m = ro.metric(np.linspace(1, 2, F), pdt, transform="stft")
    P = ro.penalty_matrix(m, 0.5, pdt)
    pen_o, ridge_o = ro.track(cost, P, pdt(ro.EPS64))
    pen, ridge = _track_gpu(cost[None], m, 0.5, cdt, pdt)
    assert _same_bits(pen[0], pen_o)
    assert np.array_equal(ridge[0], ridge_o)


def _extract_host(Tf, scales, penalty, n_ridges, bw, transform="cwt"):
    """ssq_extract_ridges_host with cost_out -> (idx, ridge_f, ridge_e, costs [n_ridges][F][N])."""
    cplx = np.iscomplexobj(Tf)
    cdt = np.float64 if Tf.dtype in (np.complex128, np.float64) else np.float32
    pdt = ro.param_dtype(Tf)
    F, N = Tf.shape
    m = ro.metric(scales, pdt, transform)
    s = np.ascontiguousarray(np.asarray(scales, dtype=pdt).reshape(-1))
    idx = np.empty((N, n_ridges), dtype=np.int64)
    rf, re = np.empty((N, n_ridges), dtype=pdt), np.empty((N, n_ridges), dtype=pdt)
    costs = np.empty((n_ridges, F, N), dtype=cdt)
    Tc = np.ascontiguousarray(Tf)
    rc = _lib.load().ssq_extract_ridges_host(_code(cdt), _code(pdt), int(cplx), _vp(Tc), 1, F, N, _vp(m), _vp(s),
                                             float(pdt(penalty)), n_ridges, float(bw), _vp(idx), _vp(rf), _vp(re),
                                             _vp(costs))
    _lib.check(rc)
    return idx, rf, re, costs, m, pdt


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128, np.float32, np.float64])
def test_costs_within_ulps_and_dp_on_them_reproduces_the_ridges(dtype):
    rng = np.random.default_rng(3)
    F, N = 48, 200
    Tf = rng.standard_normal((F, N)) + (1j * rng.standard_normal((F, N)) if np.dtype(dtype).kind == "c" else 0)
    Tf = Tf.astype(dtype)
    Tf[:, 17] = 0                                                  # an all-zero column: NaN cost from there on
    scales = np.exp(np.linspace(0.5, 4, F))
    idx, rf, re, costs, m, pdt = _extract_host(Tf, scales, 2.0, 3, 4)
    (_, _, _), costs_o = ro.extract_ridges(Tf, scales, 2.0, n_ridges=3, bw=4, get_params=True, return_costs=True)
    P = ro.penalty_matrix(m, 2.0, pdt)
    eps = pdt(ro.EPS64 if Tf.dtype == np.complex128 else ro.EPS32)
    # the first ridge's cost is the oracle's; later ones follow the GPU's own bands, so compare the first only
    c0, o0 = costs[0], costs_o[0]
    assert np.array_equal(np.isnan(c0), np.isnan(o0))
    ok = ~np.isnan(o0)
    # cost = -log(q + eps) with q = e / emax in [0, 1]: an ulp of q near the column max is an absolute error of
    # one ulp of 1 in the cost, so ulps are counted at max(|cost|, 1)
    assert np.all(np.abs(c0[ok] - o0[ok]) <= 8 * np.spacing(np.maximum(np.abs(o0[ok]), 1).astype(c0.dtype)))
    for i in range(3):
        _, r = ro.track(costs[i], P, eps)
        assert np.array_equal(idx[:, i], r), i


def _oracle_match(Tf, scales, **kw):
    got = up.extract_ridges(Tf, scales, **kw)
    ref = ro.extract_ridges(Tf, scales, **kw)
    if kw.get("get_params"):
        assert np.array_equal(got[0], ref[0])
        assert got[1].dtype == ref[1].dtype and np.array_equal(got[1], ref[1])
        assert got[2].dtype == ref[2].dtype
        assert np.allclose(got[2], ref[2], rtol=1e-12 if ref[2].dtype == np.float64 else 1e-6, atol=0)
    else:
        assert got.dtype == np.int64 and np.array_equal(got, ref)
    return got


def _chirp_tone(N=512):
    t = np.arange(N)
    f_chirp = 0.04 + 0.12 * t / N                                # cycles / sample
    x = np.cos(2 * np.pi * np.cumsum(f_chirp)) + 0.8 * np.cos(2 * np.pi * 0.35 * t)
    return x, f_chirp


@pytest.mark.parametrize("n_ridges", [1, 2, 3])
def test_end_to_end_cwt(n_ridges):
    x, _ = _chirp_tone()
    scales = 2 ** (np.arange(8, 8 + 5 * 8) / 8)
    Tx, Wx, ssq_freqs, sc = up.ssq_cwt(x, "gmw", scales=scales)
    assert Tx.dtype == np.complex128
    _oracle_match(Wx, sc, n_ridges=n_ridges, bw=4, get_params=True)
    _oracle_match(Tx, ssq_freqs, n_ridges=n_ridges, bw=2, get_params=n_ridges == 2)


@pytest.mark.parametrize("n_ridges", [1, 2, 3])
def test_end_to_end_stft(n_ridges):
    from scipy.signal.windows import dpss
    x, _ = _chirp_tone()
    win = dpss(128, 16, sym=False)
    Tx, Sx, ssq_freqs, Sfs = up.ssq_stft(x, win, n_fft=128)
    _oracle_match(Sx, Sfs, n_ridges=n_ridges, bw=4, transform="stft", get_params=True)
    _oracle_match(Tx, ssq_freqs, n_ridges=n_ridges, bw=2, transform="stft")


def test_ridges_follow_a_chirp_and_a_tone():
    N = 1024
    x, f_chirp = _chirp_tone(N)
    Tx, _, ssq_freqs, _ = up.ssq_stft(x, np.hanning(256), n_fft=256)
    F = Tx.shape[0]
    df = ssq_freqs[1] - ssq_freqs[0]
    idx = up.extract_ridges(Tx, ssq_freqs, penalty=2.0, n_ridges=2, bw=F // 16, transform="stft")
    want = [np.round(f_chirp / df), np.full(N, np.round(0.35 / df))]
    interior = slice(N // 16, N - N // 16)
    for w in want:
        near = np.min(np.abs(idx[interior] - w[interior, None]), axis=1) <= 2
        assert near.mean() >= 0.95, near.mean()


def test_batch_equals_the_per_signal_loop():
    rng = np.random.default_rng(11)
    B, F, N = 5, 40, 120
    Tb = (rng.standard_normal((B, F, N)) + 1j * rng.standard_normal((B, F, N))).astype(np.complex64)
    scales = np.exp(np.linspace(0, 3, F))
    idx, rf, re = up.extract_ridges(Tb, scales, n_ridges=2, bw=3, get_params=True)
    assert idx.shape == (B, N, 2) and rf.shape == (B, N, 2) and re.dtype == np.float32
    for b in range(B):
        i1, f1, e1 = up.extract_ridges(Tb[b], scales, n_ridges=2, bw=3, get_params=True)
        assert np.array_equal(idx[b], i1) and np.array_equal(rf[b], f1) and np.array_equal(re[b], e1)


def test_upstream_test_basic_on_the_gpu():
    """old/tests/ridge_extraction_test.py:17-26, integer input."""
    m = np.array([[1, 4, 4], [2, 2, 2], [5, 5, 4]])
    idx, f, e = up.extract_ridges(m, np.exp([1, 2, 3]), penalty=2.0, get_params=True)
    assert np.array_equal(idx, [[2], [2], [2]])
    assert np.array_equal(e[:, 0], [25, 25, 16]) and e.dtype == np.float32
    assert np.array_equal(f[:, 0], np.exp([3, 3, 3]).astype(np.float32))
    idx2 = up.extract_ridges(m, np.exp([1, 2, 3])[:, None], penalty=2.0, parallel=False)
    assert np.array_equal(idx2, [[2], [2], [2]])


def test_shape_errors_reach_ssq_last_error():
    lib = _lib.load()
    z = np.zeros((1, 4), dtype=np.float32)
    m = np.zeros(1, dtype=np.float32)
    r = np.zeros(4, dtype=np.int64)
    assert lib.ssq_ridge_track_host(_lib.SSQ_F32, _lib.SSQ_F32, _vp(z), 1, 40000, 1, _vp(m), 2.0, _vp(r), None) != 0
    assert b"n_freqs" in lib.ssq_last_error()
    assert lib.ssq_ridge_track_host(_lib.SSQ_F32, _lib.SSQ_F32, _vp(z), 1, 4, 0, _vp(m), 2.0, _vp(r), None) != 0
    assert b"n_time" in lib.ssq_last_error()
