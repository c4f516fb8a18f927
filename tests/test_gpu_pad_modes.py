"""GPU parity of padtype 'symmetric', 'replicate' and 'wrap' in the upstream mirror (`ssqueeze_rs_amd.upstream`).

The kernels fetch padded samples through one index map (csrc/pad_index.h); the reference is the numba-free restatement
oracle/upstream_oracle.py with its `padsignal` patched (pytest's monkeypatch, inside each test) by the five-mode
restatement tests/helpers/pad_ref.py.  Padding changes which sample is loaded, not the arithmetic, so every tolerance
is the one tests/test_gpu_upstream.py uses for 'reflect' / 'zero' on the same path: fp64 1e-11 of the maximum and the
bin-parity rule of `_check_ssq_stft` / `_check_ssq_cwt` (Tx <= 1e-10 after re-accumulating the oracle with the kernel's
own bins); fp32 2e-6 (STFT) and 5e-6 (CWT) of the maximum, the STFT's Tx by the column sums of
`test_float32_mode_and_batches`.  The one bound that file has no figure for is the fp32 column sum of the CWT's Tx: a
column of Tx is `const` times the sum of the kept rows of Wx, so it carries at most `na` times the 5e-6 of Wx.

The signal is a ramp plus a tone: its two ends differ by 3, so a loader that fell back to 'reflect' or 'zero' misses by
orders of magnitude, not at the tolerance.

Routing (csrc/api_stft.hip, csrc/api_cwt.hip): upstream-variant plans run the unfused STFT kernels (stft_generic.hip,
direct sums up to n_fft 128 and the packed device FFT beyond) and the CWT's naive / tile / two-step kernels.  The fused
STFT kernels and the `cwt_os` time tiles are reference-variant only, at every N, and reference-variant plans know two
pad codes; `test_upstream_plans_stay_off_the_fused_and_time_tile_kernels` asks the plans, at the smallest N at which a
reference-variant plan launches time tiles."""
import ctypes as C

import numpy as np
import pytest

from oracle import upstream_oracle as u
from ssqueeze_rs_amd import upstream as up
from ssqueeze_rs_amd import _lib
from tests.helpers import pad_ref
from tests.test_gpu_upstream import _check_ssq_stft

pytestmark = pytest.mark.gpu

MODES = ("symmetric", "replicate", "wrap")
DTYPES = (np.float64, np.float32)
# (N, n_fft, hop).  Every shape runs stft_generic.hip, the only STFT kernels an upstream plan launches: n_fft 121, 64 and
# 16 by its direct sums (n_fft <= 128), n_fft 1024 and 1000 by its packed frames through the device FFT (a power of two
# and Bluestein).  They are the shapes at which a reference-variant plan would pick the fused, any-length and generic
# kernels.  N = 5 under n_fft = 16 pads wider than the signal: 'wrap' and 'symmetric' go round more than once.
STFT_SHAPES = ((3000, 1024, 256), (700, 64, 2), (3000, 1000, 250), (600, 121, 3), (5, 16, 1))


def _ramp_tone(N, dtype=np.float64):
    return (np.linspace(-1, 2, N) + 0.3 * np.sin(2 * np.pi * 0.07 * np.arange(N))).astype(dtype)


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _scales(nv, octaves=9):                                  # tests/test_gpu_upstream.py::_scales for the GMW
    j0 = int(np.ceil(np.log2(20 ** (1 / 3) / np.pi) * nv))
    return 2 ** (np.arange(j0, j0 + octaves * nv) / nv)


@pytest.fixture
def oracle(monkeypatch):
    monkeypatch.setattr(u, "padsignal", pad_ref.padsignal)
    return u


# ------------------------------------------------------------------------------------------------------- STFT ----
@pytest.mark.parametrize("N,n_fft,hop", STFT_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_stft_with_derivative(oracle, mode, dtype, N, n_fft, hop):
    x = _ramp_tone(N, dtype)
    win = np.hanning(n_fft + 2)[1:-1]
    Sx, dSx = up.stft(x, win, n_fft=n_fft, hop_len=hop, fs=3.0, padtype=mode, derivative=True)
    So, dSo = oracle.stft(x.astype(np.float64), win, n_fft=n_fft, hop_len=hop, fs=3.0, padtype=mode, derivative=True)
    assert Sx.shape == So.shape and Sx.dtype == (np.complex128 if dtype == np.float64 else np.complex64)
    tol = 1e-11 if dtype == np.float64 else 2e-6
    print(mode, dtype.__name__, (N, n_fft, hop), "Sx", _rel(Sx, So), "dSx", _rel(dSx, dSo))
    assert _rel(Sx, So) <= tol and _rel(dSx, dSo) <= tol
    # and the mode is the one asked for: far from what 'reflect' gives at the same shape
    assert _rel(Sx, oracle.stft(x.astype(np.float64), win, n_fft=n_fft, hop_len=hop, fs=3.0)) > 1e-3


@pytest.mark.parametrize("N,n_fft,hop", STFT_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_ssq_stft(oracle, mode, dtype, N, n_fft, hop):
    x = _ramp_tone(N, dtype)
    win = np.hanning(n_fft + 2)[1:-1]
    if dtype == np.float64:
        _check_ssq_stft(x, win, n_fft=n_fft, hop_len=hop, padtype=mode)     # (reads `u.padsignal`: the patched one)
        return
    # fp32: the figures of tests/test_gpu_upstream.py::test_float32_mode_and_batches
    Tx, Sx, f, Sfs = up.ssq_stft(x, win, n_fft=n_fft, hop_len=hop, padtype=mode)
    To, So, *_ = oracle.ssq_stft(x.astype(np.float64), win, n_fft=n_fft, hop_len=hop, padtype=mode, gamma=10 * u.EPS32)
    assert Tx.shape == To.shape and Tx.dtype == np.complex64 and f.dtype == np.float32
    print(mode, (N, n_fft, hop), "Sx", _rel(Sx, So), "Tx sums", np.abs(Tx.sum(0) - To.sum(0)).max(),
          1e-4 * np.abs(So).max() * (Sfs[1] - Sfs[0]) * Tx.shape[0])
    assert np.abs(Sx - So).max() <= 2e-6 * np.abs(So).max()
    assert np.abs(Tx.sum(0) - To.sum(0)).max() <= 1e-4 * np.abs(So).max() * (Sfs[1] - Sfs[0]) * Tx.shape[0]


# -------------------------------------------------------------------------------------------------------- CWT ----
# N = 1000: the tile kernels (padded length 2048); N = 5: the naive path (padded length 8).  The CWT pads to p2up(N),
# never by more than the signal on a side, so no CWT shape goes round twice: the STFT's N = 5 and the CPU grid of
# tests/test_pad_index.py cover that.
CWT_SHAPES = ((1000, _scales(8)), (5, 2.0 ** (np.arange(8, 24) / 8)))


@pytest.mark.parametrize("N,sc", CWT_SHAPES, ids=["N1000", "N5"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_cwt_with_derivative(oracle, mode, dtype, N, sc):
    x = _ramp_tone(N, dtype)
    tol = 1e-11 if dtype == np.float64 else 5e-6
    for rpadded in (False, True):
        Wx, s, dWx = up.cwt(x, "gmw", scales=sc, fs=10.0, derivative=True, padtype=mode, rpadded=rpadded)
        Wo, so, dWo = oracle.cwt(x.astype(np.float64), "gmw", scales=sc, fs=10.0, derivative=True, padtype=mode,
                                 rpadded=rpadded)
        assert Wx.shape == Wo.shape == (len(sc), pad_ref.p2up(N)[0] if rpadded else N)
        print(mode, dtype.__name__, N, rpadded, "Wx", _rel(Wx, Wo), "dWx", _rel(dWx, dWo))
        assert _rel(Wx, Wo) <= tol and _rel(dWx, dWo) <= tol
    assert _rel(Wx, oracle.cwt(x.astype(np.float64), "gmw", scales=sc, fs=10.0, rpadded=True)[0]) > 1e-3


@pytest.mark.parametrize("N,sc", ((1000, _scales(16)), CWT_SHAPES[1]), ids=["N1000", "N5"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_ssq_cwt(oracle, mode, dtype, N, sc):
    """fp64: tests/test_gpu_upstream.py::test_ssq_cwt_matches_upstream_restatement; fp32: Wx at 5e-6 and the column sums
    of Tx at `na` times that (module docstring)."""
    x = _ramp_tone(N, dtype)
    fs = 10.0
    na = len(sc)
    if dtype == np.float32:
        Tx, Wx, f, s = up.ssq_cwt(x, "gmw", scales=sc, fs=fs, padtype=mode)
        To, Wo, fo, so, im = oracle.ssq_cwt(x.astype(np.float64), "gmw", scales=sc, fs=fs, padtype=mode,
                                            gamma=10 * u.EPS32, return_intermediates=True)
        wmax = np.abs(Wo).max()
        print(mode, N, "Wx", _rel(Wx, Wo), "Tx sums", np.abs(Tx.sum(0) - To.sum(0)).max(), 5e-6 * wmax * im["const"] * na)
        assert Tx.shape == To.shape and Tx.dtype == np.complex64
        assert np.abs(Wx - Wo).max() <= 5e-6 * wmax
        assert np.abs(Tx.sum(0) - To.sum(0)).max() <= 5e-6 * wmax * im["const"] * na
        return
    Tx, Wx, f, s, w, dWx = up.ssq_cwt(x, "gmw", scales=sc, fs=fs, padtype=mode, get_w=True, get_dWx=True)
    To, Wo, fo, so, im = oracle.ssq_cwt(x, "gmw", scales=sc, fs=fs, padtype=mode, return_intermediates=True)
    assert Tx.shape == To.shape and np.allclose(f, fo, rtol=1e-14, atol=0)
    wmax = np.abs(Wo).max()
    assert np.abs(Wx - Wo).max() <= 1e-11 * wmax and np.abs(dWx - im["dWx"]).max() <= 1e-11 * np.abs(im["dWx"]).max()
    keep_g, keep_o = np.isfinite(w), im["k"] >= 0
    assert np.abs(Wo[keep_g != keep_o]).max(initial=0.0) <= 1e-6 * wmax + 1e-12
    fa = im["freqs_ascending"]
    with np.errstate(all="ignore"):
        v = (np.log2(w) - np.log2(fa[0])) / (np.log2(fa[1]) - np.log2(fa[0]))
        k_own = na - 1 - np.minimum(np.rint(np.maximum(np.where(keep_g, v, 0.0), 0)), na - 1).astype(np.int64)
    Tre = np.zeros_like(To)
    cols = np.arange(Tx.shape[1])
    for i in range(na):
        m = keep_g[i]
        np.add.at(Tre, (k_own[i, m], cols[m]), Wo[i, m] * im["const"])
    assert np.abs(Tx - Tre).max() <= 1e-10 * max(np.abs(Tre).max(), 1e-300)
    both = keep_o & keep_g & (np.abs(Wo) > 1e-6 * wmax)
    mism = both & (k_own != im["k"])
    if mism.any():
        vv = v[mism]
        assert (np.abs(np.abs(vv - np.floor(vv)) - 0.5) < 1e-6).all()
    assert mism.mean() <= 1e-3


def test_cwt_higher_order_and_the_rs_switch_take_the_modes(oracle):
    """`cwt_higher_order`, `cwt(order=(k,))` and `_rs.*(..., _upstream=True)` forward `padtype` to the same plans; the
    higher-order reference (tests/helpers/gmw_order_ref.py) pads through the oracle's patched `padsignal`."""
    from ssqueeze_rs_amd import _rs
    from tests.helpers import gmw_order_ref as g
    x = _ramp_tone(1000)
    sc = _scales(8)
    for mode in MODES:
        W2o = g.cwt_higher_order(x, sc, 3.0, 60.0, 2, padtype=mode)
        assert _rel(up.cwt_higher_order(x, "gmw", order=2, scales=sc, padtype=mode)[0], W2o) <= 1e-11
        assert _rel(up.cwt(x, "gmw", scales=sc, order=(2,), padtype=mode)[0], W2o) <= 1e-11
        assert _rel(W2o, g.cwt_higher_order(x, sc, 3.0, 60.0, 2)) > 1e-3
        Wr, sr, _ = _rs.cwt(x, "gmw", nv=8, padtype=mode, _upstream=True)
        assert _rel(Wr, oracle.cwt(x, "gmw", scales=sr, padtype=mode)[0]) <= 1e-11
        win = np.hanning(256)
        Sr, _ = _rs.stft(x, 256, 64, win, mode, _upstream=True)
        assert _rel(Sr, oracle.stft(x, win, n_fft=256, hop_len=64, padtype=mode)) <= 1e-11
    with pytest.raises(ValueError):
        up.stft(x, np.hanning(64), n_fft=64, padtype="constant")
    with pytest.raises(ValueError):
        up.ssq_cwt(x, "gmw", scales=sc, padtype="periodic")


# ------------------------------------------------------------------------------------------ unchanged behaviour ----
def test_reflect_and_zero_are_unchanged_bytes():
    """'reflect' is the default argument; 'zero' gives one signal the same bytes alone and inside a batch of three."""
    for dtype in DTYPES:
        x = _ramp_tone(3000, dtype)
        xb = np.stack([x, x[::-1], 0.5 * x])
        win = np.hanning(256)
        sc = _scales(8).astype(dtype)
        a = up.ssq_stft(x, win, n_fft=256, hop_len=16, padtype="reflect")
        b = up.ssq_stft(x, win, n_fft=256, hop_len=16)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        a = up.ssq_cwt(x[:1000], "gmw", scales=sc, padtype="reflect")
        b = up.ssq_cwt(x[:1000], "gmw", scales=sc)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        one = up.ssq_stft(x, win, n_fft=256, hop_len=16, padtype="zero")
        three = up.ssq_stft(xb, win, n_fft=256, hop_len=16, padtype="zero")
        assert one[0].tobytes() == three[0][0].tobytes() and one[1].tobytes() == three[1][0].tobytes()
        one = up.ssq_cwt(x[:1000], "gmw", scales=sc, padtype="zero")
        three = up.ssq_cwt(np.ascontiguousarray(xb[:, :1000]), "gmw", scales=sc, padtype="zero")
        assert one[0].tobytes() == three[0][0].tobytes() and one[1].tobytes() == three[1][0].tobytes()
        # and the batched call takes the new modes signal by signal
        for mode in MODES:
            one = up.ssq_stft(xb[1], win, n_fft=256, hop_len=16, padtype=mode)
            three = up.ssq_stft(xb, win, n_fft=256, hop_len=16, padtype=mode)
            assert one[0].tobytes() == three[0][1].tobytes()
            one = up.cwt(xb[2, :1000], "gmw", scales=sc, padtype=mode)
            three = up.cwt(np.ascontiguousarray(xb[:, :1000]), "gmw", scales=sc, padtype=mode)
            assert one[0].tobytes() == three[0][2].tobytes()


def test_upstream_plans_stay_off_the_fused_and_time_tile_kernels():
    """The fused STFT kernels and the `cwt_os` families are reference-variant only (csrc/api_stft.hip: `force_generic`;
    csrc/api_cwt.hip: `!ups`), and a reference-variant plan knows two pad codes, so no call launches one of them with a
    new mode: no N makes an upstream call launch a time tile.  Asked of the plans themselves, at shapes where a
    reference-variant plan does take those kernels: n_fft = 1024, and N = 262 144 = 64 * kOsL, fp32, 24 ascending
    Morlet scales in [4, 30], the smallest N at which time tiles are launched.  If this fails, the loaders of those
    kernels meet the new modes and need the parity checks of this file."""
    lib = _lib.load()
    vp = C.c_void_p
    N = 64 * 4096
    win = np.hanning(1024)
    sc = 2.0 ** (np.arange(16, 40) / 8)
    for variant, fused, tiled in ((0, 1, True), (up.VARIANT_UPSTREAM, 0, False)):
        for code in ((0, 1) if variant == 0 else range(5)):
            plan = vp()
            _lib.check(lib.ssq_stft_plan_create_v(C.byref(plan), _lib.SSQ_F32, N, win.ctypes.data_as(vp), 1024, 256, 1.0,
                                                  code, 0, -1.0, 0, variant))
            assert lib.ssq_stft_plan_is_fused(plan) == fused, (variant, code)
            _lib.check(lib.ssq_stft_plan_destroy(plan))
            plan = vp()
            _lib.check(lib.ssq_cwt_plan_create_v(C.byref(plan), _lib.SSQ_F32, N, _lib.WAVELET["morlet"], 13.4, 0.0,
                                                 sc.ctypes.data_as(vp), len(sc), 1.0, code, variant))
            assert (lib.ssq_cwt_plan_tiled_rows(plan) > 0) == tiled, (variant, code)
            _lib.check(lib.ssq_cwt_plan_destroy(plan))
