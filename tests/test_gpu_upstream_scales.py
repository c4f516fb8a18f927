"""The upstream CWT family on 'log-piecewise' and 'linear' scale arrays (`ssqueeze_rs_amd.upstream`), on the GPU.

Checked against the NumPy restatements oracle/upstream_oracle.py (the transform, scale by scale) and
tests/helpers/scales_ref.py (row weights, frequencies, the two-segment bin rule; ssqueezing.py:122-133, :247-283,
algos.py:356-370, :860-897), and against upstream's own reconstruction thresholds
(old/tests/reconstruction_test.py:65-87, :111-124).  Tolerances as tests/test_gpu_upstream.py: fp64 Wx <= 1e-11 max,
Tx <= 1e-10 after re-accumulating with the kernel's own w; fp32 Wx <= 5e-6 max, Tx by column sums."""
import numpy as np
import pytest

from oracle import upstream_oracle as u
from ssqueeze_rs_amd import upstream as up
from tests.helpers import scales_ref as ref

pytestmark = pytest.mark.gpu

GMW8 = ("gmw", {"beta": 8})


def _t(a, b, n):
    return np.linspace(a, b, n, endpoint=False)


def echirp(N):                                             # reconstruction_test.py:33-35
    t = _t(0, 10, N)
    return np.cos(2 * np.pi * 3 * np.exp(t / 3)), t


def lchirp(N):                                             # :37-39
    t = _t(0, 10, N)
    return np.cos(np.pi * t ** 2), t


def _freqs(N, freqs):                                      # :42-45
    x = np.concatenate([np.cos(2 * np.pi * f * _t(i, i + 1, N // len(freqs))) for i, f in enumerate(freqs)])
    return x, _t(0, len(x) / N, len(x))


def fast_transitions(N):
    return _freqs(N, np.array([N / 100, N / 200, N / 3, N / 20, N / 3 - 1, N / 50, N / 4, N / 150]) / 8)


def low_freqs(N):
    return _freqs(N, [.3, .3, 1, 1, 2, 2])


def high_freqs(N):
    return _freqs(N, np.array([N / 2, N / 2 - 1, N / 4, N / 3]) / 4)


def mad_rms(x, xrec):                                      # :26-29
    return np.mean(np.abs(x - xrec)) / np.sqrt(np.mean(x ** 2))


def _grid(kind, N, wavelet):
    s = up.process_scales(kind, N, wavelet).reshape(-1)
    assert up.infer_scaletype(s)[0] == kind.split(":")[0]
    return s


def _make_ssq_freqs(M):                                    # old/tests/fft_test.py:236-246 ('log-piecewise')
    sf = np.logspace(0, np.log10(M), 2 * M)
    return np.hstack([sf[:M // 2], sf[M // 2 + 3 - 1::3]])


# ------------------------------------------------------------------------------------------------------- cwt ----
@pytest.mark.parametrize("kind,N", [("log-piecewise", 2048), ("linear", 512)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_cwt_on_piecewise_and_linear_scales(kind, N, dtype):
    s = _grid(kind, N, GMW8)
    rng = np.random.default_rng(N)
    xb = rng.standard_normal((3, N)).astype(dtype)
    Wx, sc, dWx = up.cwt(xb, GMW8, scales=s, derivative=True)
    assert Wx.shape == (3, len(s), N) and sc.dtype == dtype and np.array_equal(sc, s.astype(dtype))
    tol = 1e-11 if dtype == np.float64 else 5e-6
    for b in (0, 2):
        Wo, _, dWo = u.cwt(xb[b].astype(np.float64), GMW8, scales=s, derivative=True)
        assert np.abs(Wx[b] - Wo).max() <= tol * np.abs(Wo).max()
        assert np.abs(dWx[b] - dWo).max() <= tol * np.abs(dWo).max()
    W1, _ = up.cwt_higher_order(xb[1], GMW8, order=1, scales=s)          # order 1 on the same grid
    W1o, _ = up.cwt(xb[1], GMW8, scales=s, order=(1,))
    assert np.array_equal(W1, W1o)
    with pytest.raises(Exception, match="differs"):                      # the nv check stays 'log'-only
        up.ssq_cwt(xb[0], GMW8, scales=2 ** (np.arange(20, 60) / 16), nv=32)
    assert np.array_equal(up.ssq_cwt(xb[0], GMW8, scales=s, nv=7)[1], up.ssq_cwt(xb[0], GMW8, scales=s)[1])


# --------------------------------------------------------------------------------------------------- ssq_cwt ----
def _check_ssq(x, s, kind, f_kind, Tx, Wx, f, w, dWx, squeezing, flipud, fp64, f_idx=None):
    """Re-squeeze the GPU's own Wx / dWx with the restatement: bins from the kernel's own w (fp64: Tx equal; fp32: column
    sums, the bins themselves: test_ssq_cwt_kernel_bins); bins from NumPy's w may differ only at rounding ties.  f_idx:
    the transition of log-piecewise frequencies found in their own dtype (default: on f)."""
    na = len(s)
    f_asc = f[::-1].astype(np.float64)
    const = ref.row_const(s, kind)
    Wx64, dW64 = Wx.astype(np.complex128), dWx.astype(np.complex128)
    keep = np.isfinite(w)
    k_own = ref.bins(np.where(keep, w.astype(np.float64), 1.0), f_asc, f_kind, f_idx)
    if flipud:
        k_own = na - 1 - k_own
    Wv = np.ones(Wx.shape) / na if squeezing == "lebesgue" else Wx64
    Tre = np.zeros((na, Wx.shape[1]), dtype=np.complex128)
    cols = np.arange(Wx.shape[1])
    for i in range(na):
        m = keep[i]
        np.add.at(Tre, (k_own[i, m], cols[m]), Wv[i, m] * const[i])
    if fp64:
        assert np.abs(Tx - Tre).max() <= 1e-10 * max(np.abs(Tre).max(), 1e-300)
        T2, k2 = ref.squeeze(Wx64, dW64, f_asc, f_kind, const, squeezing, flipud, idx=f_idx)
        mism = keep & (k2 >= 0) & (k2 != k_own)
        assert mism.mean() <= 1e-3
    else:
        scale = (np.abs(Wv) * const[:, None]).sum(0).max()
        assert np.abs(Tx.sum(0) - Tre.sum(0)).max() <= 1e-5 * scale
    return Tre


@pytest.mark.parametrize("kind,N", [("log-piecewise", 2048), ("linear", 512)])
@pytest.mark.parametrize("kw", [dict(), dict(squeezing="lebesgue", flipud=False), dict(ssq_freqs="log"),
                                dict(ssq_freqs="linear"), dict(ssq_freqs="piecewise-array"),
                                dict(ssq_freqs="piecewise-array-f32"), dict(order=(0, 1))])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ssq_cwt_on_piecewise_and_linear_scales(kind, N, kw, dtype):
    kw = dict(kw)
    x, ts = echirp(N)
    fs = 1 / (ts[1] - ts[0])
    s = _grid(kind, N, GMW8)
    na = len(s)
    if str(kw.get("ssq_freqs")).startswith("piecewise-array"):
        sq = _make_ssq_freqs(na + na % 2)[:na] * (fs / 2 / na)              # (odd M gives M - 1 entries)
        kw["ssq_freqs"] = sq.astype(np.float32) if kw["ssq_freqs"].endswith("f32") else sq
    Tx, Wx, f, sc, w, dWx = up.ssq_cwt(x.astype(dtype), GMW8, scales=s, fs=fs, get_w=True, get_dWx=True, **kw)
    assert Tx.shape == (na, N) and f.dtype == dtype and np.array_equal(sc, s.astype(dtype))
    sq = kw.get("ssq_freqs")
    f_idx = None
    if isinstance(sq, np.ndarray):
        f_kind = "log-piecewise"
        f_idx = up.logscale_transition_idx(sq)             # in sq's own dtype (float32: float32 thresholds)
        assert f_idx is not None
        assert np.array_equal(f, sq[::-1].astype(dtype))
    else:
        f_kind = sq or kind
        if f_kind == "log-piecewise":
            fo = ref.piecewise_freqs(s, N, GMW8, dt=1 / fs)
            assert np.allclose(f[::-1], fo, rtol=1e-12 if dtype == np.float64 else 1e-6)
            assert up.logscale_transition_idx(fo) == na - up.logscale_transition_idx(s)
    if "order" not in kw:
        Wo, _, dWo = u.cwt(x, GMW8, scales=s, fs=fs, derivative=True)
        tol = 1e-11 if dtype == np.float64 else 5e-6
        assert np.abs(Wx - Wo).max() <= tol * np.abs(Wo).max()
    _check_ssq(x, s, kind, f_kind, Tx, Wx, f, w, dWx, kw.get("squeezing", "sum"), kw.get("flipud", True),
               dtype == np.float64, f_idx)


def _kernel_wk(x, wavelet, s_in, fs, ssq_freqs=None, flipud=True):
    """ssq_cwt through its C entry point with the (w, k) hook -> (Tx, w, k, f_asc, f_kind, f_idx): the kernel's own
    bins, which `ssq_cwt` does not return.  The arguments are prepared as `upstream.ssq_cwt` prepares them."""
    from ssqueeze_rs_amd import _lib
    from ssqueeze_rs_amd._rs import _call, _ptr
    code = _lib.SSQ_F32 if x.dtype == np.float32 else _lib.SSQ_F64
    xa = np.ascontiguousarray(x[None])
    N, dt = len(x), 1 / fs
    wcode, p0, p1 = up._wavelet(wavelet)
    s, kind, nv, s_own = up._scales(s_in)
    const = up._row_const(s, kind, nv)
    if ssq_freqs is None:
        f_kind = kind
        f = f_own = np.ascontiguousarray(up._ssq_freqs(s, N, wcode, p0, p1, dt, "peak", kind, s_own))
    else:
        f_own = ssq_freqs
        f = np.ascontiguousarray(ssq_freqs, dtype=np.float64)
        f_kind = up.infer_scaletype(f_own)[0]
    f_idx = up.logscale_transition_idx(f_own) if f_kind == "log-piecewise" else 0
    cdt = np.complex64 if code == _lib.SSQ_F32 else np.complex128
    Tx, wk = np.zeros((1, len(s), N), cdt), np.zeros((1, len(s), N), cdt)
    variant = up.VARIANT_UPSTREAM | (up.VARIANT_FLIPUD if flipud else 0)
    _call(_lib.load().ssq_ssq_cwt_host_rows(code, _ptr(xa), 1, N, wcode, p0, p1, _ptr(s), len(s), dt, _ptr(const),
                                            _ptr(f), up.FREQS[f_kind], f_idx, _lib.PAD["reflect"], 0, -1.0, variant,
                                            _ptr(Tx), None, None, _ptr(wk)))
    return Tx[0], wk[0].real, wk[0].imag.astype(np.int64), f, f_kind, f_idx


@pytest.mark.parametrize("case", ["piecewise", "piecewise-f32-scales", "piecewise-f32-freqs", "linear"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ssq_cwt_kernel_bins(case, dtype):
    """The kernel's own bin of every element (the (w, k) hook) against the restated rule on the kernel's own w
    (algos.py:860-897): equal, or one row apart where w sits on a rounding tie (fp32: within the fp32 evaluation of
    log2 w and the quotient)."""
    N = 2048
    x, ts = echirp(N)
    x = x.astype(dtype)
    fs = 1 / (ts[1] - ts[0])
    s = _grid("linear" if case == "linear" else "log-piecewise", N, GMW8)
    if case == "linear":
        s = s[:400]
    sq = None
    if case == "piecewise-f32-scales":
        s = s.astype(np.float32)
    if case == "piecewise-f32-freqs":
        sq = (_make_ssq_freqs(len(s) + len(s) % 2)[:len(s)] * (fs / 2 / len(s))).astype(np.float32)
        assert up.logscale_transition_idx(sq.astype(np.float64)) is None    # only float32's thresholds see it
    Tx, w, k, f, f_kind, f_idx = _kernel_wk(x, GMW8, s, fs, sq)
    T_pub = up.ssq_cwt(x, GMW8, scales=s, fs=fs, ssq_freqs=sq)[0]
    assert np.array_equal(Tx, T_pub)                                         # the helper is ssq_cwt's call
    assert f_kind == ("linear" if case == "linear" else "log-piecewise")
    na = len(s)
    keep = np.isfinite(w)
    assert np.array_equal(keep, k >= 0) and keep.mean() > 0.5
    kr, v = ref.bins(np.where(keep, w.astype(np.float64), 1.0), f, f_kind, f_idx or None, return_v=True)
    kr = na - 1 - kr                                                         # flipud
    mism = keep & (kr != k)
    tie = np.abs(np.abs(v - np.floor(v)) - 0.5) < (2e-3 if dtype == np.float32 else 1e-9)
    assert np.all(np.abs(kr - k)[mism] <= 1) and np.all(tie[mism])
    assert mism.mean() <= 1e-3
    if f_kind == "log-piecewise":                                            # both segments are used
        rows = na - 1 - k[keep]
        assert (rows >= f_idx).any() and (rows < f_idx - 1).any()


def test_float32_scales_through_the_whole_chain():
    """A float32 log-piecewise grid, as `ssq_cwt` returns it for float32 input, goes back into `cwt`, `ssq_cwt` and
    `icwt` (upstream's chain, reconstruction_test.py:111-124, in float32)."""
    x, ts = echirp(1024)
    x32 = x.astype(np.float32)
    s = up.process_scales("log-piecewise", len(x), "gmw").reshape(-1)
    Tx, Wx, f, sc = up.ssq_cwt(x32, "gmw", scales=s, t=ts)
    assert sc.dtype == np.float32 and up.infer_scaletype(sc)[0] == "log-piecewise"
    assert mad_rms(x, up.issq_cwt(Tx, "gmw")) < .02
    assert mad_rms(x, up.icwt(Wx, "gmw", scales=sc)) < .02
    W2, s2 = up.cwt(x32, "gmw", scales=sc)
    assert np.abs(W2 - Wx).max() <= 1e-5 * np.abs(Wx).max()
    T2, _, f2, _ = up.ssq_cwt(x32, "gmw", scales=sc, t=ts)
    assert np.allclose(f2, f, rtol=1e-6)
    assert np.abs(T2.sum(0) - Tx.sum(0)).max() <= 1e-4 * np.abs(Tx.sum(0)).max()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ssq_cwt_piecewise_two_step_plan(dtype):
    """N = 2^16 (padded 2^17: the two-step plan), maximal preset.  A kernel trace of this configuration showed the large
    scales on the band-limited inverse (cwt_tile_kernel mode 6, CWT_INV_Z) beside the two-step modes."""
    N = 2 ** 16
    rng = np.random.default_rng(3)
    x = (np.cos(2 * np.pi * 0.001 * np.arange(N) ** 1.3 / 30) + 0.3 * rng.standard_normal(N)).astype(dtype)
    s = _grid("log-piecewise", N, "gmw")
    Tx, Wx, f, sc, w, dWx = up.ssq_cwt(x, "gmw", scales=s, get_w=True, get_dWx=True)
    cols = slice(None) if dtype == np.float64 else slice(0, N, 7)
    Wo, _ = u.cwt(x.astype(np.float64), "gmw", scales=s)
    tol = 1e-11 if dtype == np.float64 else 5e-6
    assert np.abs(Wx - Wo).max() <= tol * np.abs(Wo).max()
    _check_ssq(x, s, "log-piecewise", "log-piecewise", Tx[:, cols], Wx[:, cols], f, w[:, cols], dWx[:, cols], "sum",
               True, dtype == np.float64)


def test_ssq_cwt_piecewise_rejects_maximal_maprange():
    x = np.zeros(2048)
    s = _grid("log-piecewise", 2048, "gmw")
    with pytest.raises(ValueError):
        up.ssq_cwt(x, "gmw", scales=s, maprange="maximal")                 # ssqueezing.py:181-184
    with pytest.raises(ValueError):
        up.ssq_cwt(x, "gmw", scales=2 ** (np.arange(20, 120) / 16), ssq_freqs="log-piecewise", maprange="maximal")
    Tx, _, f, _ = up.ssq_cwt(x, "gmw", scales=s, maprange="maximal", ssq_freqs="log")
    assert Tx.shape == (len(s), 2048) and np.allclose(f[[0, -1]], [0.5, 1 / 2048])


# ------------------------------------------------------------------------------------------------ inverses ----
def test_reconstruction_ssq_cwt_thresholds():
    """reconstruction_test.py:65-87: issq_cwt(ssq_cwt(x)) within mad_rms 0.1 on 'log', 'log-piecewise', 'linear' (the
    low-frequency signal on ':maximal' bounds, without 'linear')."""
    for fn in (echirp, lchirp, fast_transitions, low_freqs, high_freqs):
        x, ts = fn(2048)
        for kind in ("log", "log-piecewise", "linear"):
            spec = kind
            if fn.__name__ == "low_freqs":
                if kind == "linear":
                    continue
                spec = f"{kind}:maximal"
            s = up.process_scales(spec, len(x), GMW8).reshape(-1)
            Tx, *_ = up.ssq_cwt(x, GMW8, scales=s, nv=32, t=ts)
            err = mad_rms(x, up.issq_cwt(Tx, GMW8))
            assert err < .1, (err, fn.__name__, spec)


def test_reconstruction_log_piecewise():
    """reconstruction_test.py:111-124: ssq_cwt + issq_cwt and icwt on 'log-piecewise', both < 0.02 on echirp(1024)."""
    x, ts = echirp(1024)
    s = up.process_scales("log-piecewise", len(x), "gmw").reshape(-1)
    Tx, Wx, f, sc = up.ssq_cwt(x, "gmw", scales=s, t=ts)
    assert mad_rms(x, up.issq_cwt(Tx, "gmw")) < .02
    assert mad_rms(x, up.icwt(Wx, "gmw", scales=sc)) < .02
    # the inverse itself: the two segments' one-integral sums (_cwt.py:418-448)
    idx = up.logscale_transition_idx(s)
    adm = u.adm_ssq("gmw")
    want = sum((2 / adm) * np.log(2 ** (1 / up.infer_scaletype(p)[1])) * Wx[r].real.sum(0)
               for r, p in ((slice(0, idx), s[:idx]), (slice(idx, None), s[idx:])))
    assert np.abs(up.icwt(Wx, "gmw", scales=sc) - want).max() <= 1e-12 * np.abs(x).max()


def test_icwt_linear():
    x, ts = lchirp(1024)
    s = up.process_scales("linear", len(x), GMW8).reshape(-1)
    Wx, _ = up.cwt(x, GMW8, scales=s, t=ts)
    adm = u.adm_ssq(GMW8)
    for l1, p in ((True, 1.0), (False, 1.5)):
        W = Wx if l1 else up.cwt(x, GMW8, scales=s, t=ts, l1_norm=False)[0]
        want = (2 / adm) * np.pi / 4 * (W.real / s[:, None] ** p).sum(0) + 0.5
        assert np.abs(up.icwt(W, GMW8, scales=s, l1_norm=l1, x_mean=0.5) - want).max() <= 1e-12 * np.abs(want).max()


# ---------------------------------------------------------------------------------------------------- ridges ----
def test_extract_ridges_on_log_piecewise_tx():
    x, ts = echirp(2048)
    s = up.process_scales("log-piecewise", len(x), "gmw").reshape(-1)
    Tx, _, f, sc = up.ssq_cwt(x, "gmw", scales=s, t=ts)
    ridge = up.extract_ridges(Tx, sc, penalty=2.0, n_ridges=1, bw=4)
    assert ridge.shape == (len(x), 1) and ridge.min() >= 0 and ridge.max() < len(s)
