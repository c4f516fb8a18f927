"""`upstream.ssqueeze`, `phase_cwt` and `phase_stft` on the GPU, against the fused `ssq_cwt` / `ssq_stft` (their
get_w output and Tx) and the NumPy restatement tests/helpers/ssqueeze_ref.py.  Tolerances as tests/test_gpu_upstream.py:
fp64 w <= 1e-12 relative, Tx <= 1e-10 relative where the bins agree; fp32 by column sums (invariant under a bin
flip) and a bounded share of cells at half-bin ties."""
import numpy as np
import pytest

from ssqueeze_rs_amd import upstream as up
from tests.helpers import ssqueeze_ref as ref

pytestmark = pytest.mark.gpu

GMW8 = ("gmw", {"beta": 8})
EPS = {np.float32: float(np.finfo(np.float32).eps), np.float64: float(np.finfo(np.float64).eps)}


def echirp(N):                                             # reconstruction_test.py:33-35
    t = np.linspace(0, 10, N, endpoint=False)
    return np.cos(2 * np.pi * 3 * np.exp(t / 3)), t


def _grid(kind, N):
    if kind == "log":
        wc = 20 ** (1 / 3)
        j0 = int(np.ceil(np.log2(wc / np.pi) * 16))
        return 2 ** (np.arange(j0, j0 + 7 * 16) / 16)
    return up.process_scales(kind, N, GMW8).reshape(-1)


def _cwt(kind, N, dtype, batch=None):
    x, ts = echirp(N)
    fs = 1 / (ts[1] - ts[0])
    if batch:
        x = np.stack([x * (1 + 0.25 * b) + 0.1 * b for b in range(batch)])
    s = _grid(kind, N)
    Wx, sc, dWx = up.cwt(x.astype(dtype), GMW8, scales=s, fs=fs, derivative=True)
    return x.astype(dtype), fs, s, Wx, dWx


def _close_tx(T, R, dtype, cells=1e-3):
    """T against R: fp64 elementwise; fp32 by column sums plus a bounded share of differing cells (half-bin ties)."""
    scale = max(np.abs(R).max(), 1e-300)
    if dtype == np.float64:
        assert np.abs(T - R).max() <= 1e-10 * scale
        return
    assert np.abs(T.sum(-2) - R.sum(-2)).max() <= 1e-4 * scale * np.sqrt(R.shape[-2])
    assert (np.abs(T - R) > 1e-4 * scale).mean() <= cells


def _check_w(w, W, dW, wf, wr, g, dtype, scale=0.0):
    """w (this kernel) against wr (the restatement, on the same W, dW) and wf (the fused get_w, computed from the fused
    path's own W, dW, which agree with these to rounding of their largest values): inf on the same cells, against wf
    but where |W| is within that rounding of gamma; finite values within 1e-12 (fp32 1e-4) of |w| plus the rounding
    of the cancellation in B C - A D (an fma or not) and of Sfs - q, and against wf plus the effect of a W, dW
    perturbed by a few ulps of their maxima on Im(dW / W) / 2 pi."""
    fin = np.isfinite(w)
    assert np.array_equal(fin, np.isfinite(wr))
    e = EPS[dtype]
    tol = 1e-12 if dtype == np.float64 else 1e-4
    mag = np.abs(W).astype(np.float64)
    pert, pert_d = 8 * e * mag.max(), 8 * e * np.abs(dW).max()
    sure = np.abs(mag - g) > pert + 4 * e * g
    assert np.array_equal(fin[sure], np.isfinite(wf)[sure])
    with np.errstate(all="ignore"):
        cond = (np.abs(dW.imag * W.real) + np.abs(dW.real * W.imag)) / (mag ** 2 * 2 * np.pi)
        moved = (pert * np.abs(dW) / mag ** 2 + pert_d / mag) / (2 * np.pi)
    slack = 8 * e * (cond + scale)
    assert np.all(np.abs(w[fin] - wr[fin]) <= tol * np.abs(wr[fin]) + slack[fin])
    both = fin & np.isfinite(wf)
    assert np.all(np.abs(w[both] - wf[both]) <= tol * np.abs(wf[both]) + slack[both] + moved[both])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["log", "log-piecewise", "linear"])
def test_phase_cwt_equals_the_fused_w_and_the_restatement(kind, dtype):
    x, fs, s, Wx, dWx = _cwt(kind, 1024, dtype)
    g = 10 * EPS[dtype]
    w = up.phase_cwt(Wx, dWx, gamma=g)
    assert w.dtype == dtype and w.shape == Wx.shape
    *_, wf = up.ssq_cwt(x, GMW8, scales=s, fs=fs, get_w=True)
    _check_w(w, Wx, dWx, wf, ref.phase_cwt(Wx, dWx, g), g, dtype)
    # upstream's own default gamma for phase_cwt: sqrt(eps) (_ssq_cwt.py:488-489)
    w0 = up.phase_cwt(Wx, dWx)
    assert np.array_equal(np.isinf(w0), np.abs(Wx) < np.sqrt(EPS[dtype]))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_phase_stft_equals_the_fused_w_and_the_restatement(dtype):
    x, _ = echirp(2048)
    win = np.hanning(256)
    Tx, Sx, f, Sfs, w_f, dSx = up.ssq_stft(x.astype(dtype), win, n_fft=256, hop_len=1, get_w=True, get_dWx=True)
    w = up.phase_stft(Sx, dSx, Sfs)
    assert w.dtype == dtype and w.shape == Sx.shape
    g = 10 * EPS[dtype]
    # the fused get_w comes from an Sx transformed together with dSx (one packed FFT per frame), the returned Sx from a
    # transform of its own: the two differ in the last bits of the largest values, hence `moved` in _check_w
    _check_w(w, Sx, dSx, w_f, ref.phase_stft(Sx, dSx, Sfs, g), g, dtype, scale=float(Sfs[-1]))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["log", "log-piecewise", "linear"])
def test_ssqueeze_from_dwx_reproduces_ssq_cwt(kind, dtype):
    x, fs, s, Wx, dWx = _cwt(kind, 1024, dtype)
    Tf, _, ff, _ = up.ssq_cwt(x, GMW8, scales=s, fs=fs, maprange="peak", flipud=True)
    Tx, f = up.ssqueeze(Wx, None, dWx=dWx, scales=s, fs=fs, ssq_freqs=kind, maprange="peak", wavelet=GMW8,
                        flipud=True)
    assert Tx.dtype == Wx.dtype and Tx.shape == Wx.shape
    np.testing.assert_allclose(f, ff, rtol=1e-6 if dtype == np.float32 else 1e-14)
    _close_tx(Tx, Tf, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ssqueeze_from_dsx_reproduces_ssq_stft(dtype):
    x, _ = echirp(2048)
    win = np.hanning(256)
    for flipud in (False, True):
        Tf, Sx, f, Sfs, dSx = up.ssq_stft(x.astype(dtype), win, n_fft=256, get_dWx=True, flipud=flipud)
        Tx, fo = up.ssqueeze(Sx, None, ssq_freqs=Sfs, Sfs=Sfs, dWx=dSx, transform="stft", flipud=flipud)
        assert np.array_equal(fo, Sfs[::-1] if flipud else Sfs)
        _close_tx(Tx, Tf, dtype)


def _settle(kind, s, N, fs, ssq):
    """The frequencies, frequency type and row weights upstream's ssqueeze settles on (ssqueezing.py:122-194)."""
    st, nv = up.infer_scaletype(s)
    c = ref.row_const(s, st, nv)
    f = up._ssq_freqs(s, N, *up._wavelet(GMW8), 1 / fs, "peak", ssq, s) if isinstance(ssq, str) else ssq
    return np.asarray(f), c, (ssq if isinstance(ssq, str) else up.infer_scaletype(ssq)[0])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["log", "log-piecewise", "linear"])
@pytest.mark.parametrize("squeezing", ["sum", "lebesgue", "abs", "fn"])
def test_ssqueeze_from_w_matches_the_restatement(kind, squeezing, dtype):
    N = 1024
    x, fs, s, Wx, dWx = _cwt(kind, N, dtype)
    w = up.phase_cwt(Wx, dWx, gamma=10 * EPS[dtype])
    sq = (lambda a: a * a) if squeezing == "fn" else squeezing
    f, c, st = _settle(kind, s, N, fs, kind)
    for flipud in (False, True):
        Tx, fo = up.ssqueeze(Wx, w, ssq_freqs=kind, scales=s, fs=fs, squeezing=sq, maprange="peak", wavelet=GMW8,
                             flipud=flipud)
        R = ref.ssqueeze(Wx.astype(np.complex128), w.astype(np.float64), f, c, st, sq, flipud)
        assert Tx.shape == Wx.shape
        assert (Tx.dtype == dtype) if squeezing == "abs" else (Tx.dtype == Wx.dtype)
        assert np.allclose(fo, f[::-1], rtol=1e-14)
        _close_tx(Tx, R, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ssqueeze_from_w_on_an_edited_wx_and_array_freqs(dtype):
    N = 1024
    x, fs, s, Wx, dWx = _cwt("log-piecewise", N, dtype)
    w = up.phase_cwt(Wx, dWx, gamma=10 * EPS[dtype])
    We = Wx.copy()
    We[::3] = 0                                                   # a masked transform
    f, c, st = _settle("log-piecewise", s, N, fs, "log-piecewise")
    for freqs in (f, f.astype(np.float32), np.linspace(f[0], f[-1], len(f))):
        Tx, fo = up.ssqueeze(We, w, ssq_freqs=freqs, scales=s, fs=fs, flipud=True)
        ft = up.infer_scaletype(freqs)[0]
        R = ref.ssqueeze(We.astype(np.complex128), w.astype(np.float64), freqs, c, ft, "sum", True)
        assert np.array_equal(fo, freqs[::-1])
        # float32 frequencies: upstream takes their logs in float32, the kernel's bin parameters are fp64 (ties move)
        _close_tx(Tx, R, dtype if freqs.dtype == np.float64 else np.float32)
    # a real-valued function of Wx gives a real Tx (ssqueezing.py:183-188)
    Tr, _ = up.ssqueeze(We, w, ssq_freqs=f, scales=s, squeezing=lambda a: np.abs(a) ** 2, flipud=True)
    assert Tr.dtype == dtype
    _close_tx(Tr, ref.ssqueeze(We.astype(np.complex128), w.astype(np.float64), f, c, st,
                               lambda a: np.abs(a) ** 2, True), dtype)


def test_ssqueeze_stft_from_w_matches_the_restatement():
    x, _ = echirp(2048)
    win = np.hanning(256)
    _, Sx, _, Sfs, dSx = up.ssq_stft(x, win, n_fft=256, get_dWx=True)
    w = up.phase_stft(Sx, dSx, Sfs)
    sq = np.linspace(0.01, 0.5, len(Sfs))                          # a grid of the caller's (w path: any linear array)
    Tx, fo = up.ssqueeze(Sx, w, ssq_freqs=sq, transform="stft", flipud=True)
    R = ref.ssqueeze(Sx, w, sq, sq[1] - sq[0], "linear", "sum", True)
    assert np.array_equal(fo, sq[::-1])
    _close_tx(Tx, R, np.float64)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_equals_single_calls(dtype):
    B, N = 3, 512
    x, fs, s, Wx, dWx = _cwt("log-piecewise", N, dtype, batch=B)
    assert Wx.shape[0] == B
    w = up.phase_cwt(Wx, dWx, gamma=1e-3)
    for b in range(B):
        assert np.array_equal(w[b], up.phase_cwt(Wx[b], dWx[b], gamma=1e-3))
    kw = dict(scales=s, fs=fs, ssq_freqs="log-piecewise", maprange="peak", wavelet=GMW8)
    for sq in ("sum", "lebesgue", "abs"):
        Tb, _ = up.ssqueeze(Wx, w, squeezing=sq, **kw)
        for b in range(B):
            assert np.array_equal(Tb[b], up.ssqueeze(Wx[b], w[b], squeezing=sq, **kw)[0])
    Td, _ = up.ssqueeze(Wx, None, dWx=dWx, flipud=True, **kw)
    for b in range(B):
        assert np.array_equal(Td[b], up.ssqueeze(Wx[b], None, dWx=dWx[b], flipud=True, **kw)[0])
    win = np.hanning(64)
    _, Sx, _, Sfs, dSx = up.ssq_stft(x.astype(dtype), win, n_fft=64, get_dWx=True)
    Ts, _ = up.ssqueeze(Sx, None, ssq_freqs=Sfs, Sfs=Sfs, dWx=dSx, transform="stft")
    for b in range(B):
        assert np.array_equal(Ts[b], up.ssqueeze(Sx[b], None, ssq_freqs=Sfs, Sfs=Sfs, dWx=dSx[b], transform="stft")[0])
