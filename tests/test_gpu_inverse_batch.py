"""GPU tests of the batched full inverses: `upstream.istft`, `issq_stft`, `issq_cwt`, `icwt` on [B, F, N] against the
numba-free restatement oracle/upstream_oracle.py (2-D, looped over the batch) and against the 2-D calls."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import upstream_oracle as u
from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def echirp(N):                                   # reconstruction_test.py:33-35
    t = np.linspace(0, 10, N, endpoint=False)
    return np.cos(2 * np.pi * 3 * np.exp(t / 3)), t


def mad_rms(x, xrec):                            # reconstruction_test.py:26-29
    return np.mean(np.abs(x - xrec)) / np.sqrt(np.mean(x ** 2))


def _dpss(n):
    from scipy.signal.windows import dpss        # upstream's default window (_stft.py:283-285); data, not code under test
    return dpss(n, max(4, n // 8), sym=False)


def _scales(wavelet, nv=32, octaves=9):
    wc = 20 ** (1 / 3) if wavelet == "gmw" else 13.4
    j0 = int(np.ceil(np.log2(wc / np.pi) * nv))
    return 2 ** (np.arange(j0, j0 + octaves * nv) / nv)


# ------------------------------------------------------------------------- 1. upstream's thresholds on a batch ----
def test_stft_istft_batch_reconstruction_thresholds():
    """reconstruction_test.py:160-180 on B = 3 signals per call: MAE < 1e-14 per signal."""
    rng = np.random.default_rng(0)
    for N in (128, 129):
        x = rng.standard_normal((3, N))
        for n_fft in (120, 121):
            win = _dpss(n_fft)
            for hop in (1, 2, 3):
                for mod in (True, False):
                    Sx = up.stft(x, win, n_fft=n_fft, hop_len=hop, modulated=mod)
                    xr = up.istft(Sx, win, n_fft=n_fft, hop_len=hop, N=N, modulated=mod)
                    assert xr.shape == (3, N)
                    for b in range(3):
                        assert np.abs(x[b] - xr[b]).mean() < 1e-14, (N, n_fft, hop, mod, b)


def test_ssq_stft_issq_stft_batch_reconstruction_thresholds():
    """reconstruction_test.py:183-206 on B = 3 signals per call: MAE < 1e-1."""
    rng = np.random.default_rng(1)
    for N in (128, 129):
        x = rng.standard_normal((3, N))
        for n_fft in (120, 121):
            for scaling in (1.0, 0.5):
                win = _dpss(n_fft) * scaling
                Tx, *_ = up.ssq_stft(x, win, n_fft=n_fft)
                xr = up.issq_stft(Tx, win, n_fft=n_fft)
                assert xr.shape == (3, N)
                for b in range(3):
                    assert np.abs(x[b] - xr[b]).mean() < 1e-1, (N, n_fft, scaling, b)


def _cwt_batch():
    """echirp(1024), a linear chirp (2 -> 32 Hz at fs = 102.4) and two tones: the restatement alone reconstructs each to
    mad_rms .0016 - .0026 with both wavelets."""
    x, t = echirp(1024)
    return np.stack([x, np.cos(2 * np.pi * (2 + 1.5 * t) * t), np.cos(2 * np.pi * 8 * t) + np.cos(2 * np.pi * 20 * t)])


@pytest.mark.parametrize("wavelet", ["gmw", "morlet"])
def test_cwt_icwt_issq_cwt_batch_reconstruction_thresholds(wavelet):
    """reconstruction_test.py:111-123: mad_rms < .02 on echirp(1024), the batch holding it and two other signals."""
    x = _cwt_batch()
    sc = _scales(wavelet)
    Tx, Wx, *_ = up.ssq_cwt(x, wavelet, scales=sc)
    xs, xi = up.issq_cwt(Tx, wavelet), up.icwt(Wx, wavelet, scales=sc)
    assert xs.shape == xi.shape == x.shape
    for b in range(3):
        assert mad_rms(x[b], xs[b]) < .02 and mad_rms(x[b], xi[b]) < .02, b


# --------------------------------------------------------------------- 2. row sums: bitwise the 2-D call ----
def _cmap(*shape, dtype):
    rng = np.random.default_rng(sum(shape))
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)


LOG = 2.0 ** (np.arange(40) / 8 + 1)
LIN = np.linspace(2.0, 80.0, 40)
PIECE = np.concatenate([2.0 ** (np.arange(24) / 8 + 1), 2.0 ** (np.arange(16) / 4 + 4)])


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_row_sum_inverses_equal_the_2d_call_bitwise(dtype):
    B, N = 4, 777
    T = _cmap(B, 33, N, dtype=dtype)
    win = np.hanning(64) + 0.1
    calls = [(lambda A: up.issq_stft(A, win), T), (lambda A: up.issq_cwt(A, "gmw"), T),
             (lambda A: up.issq_cwt(A, "morlet"), T)]
    for f, A in calls:
        out = f(A)
        assert out.shape == (B, N) and out.dtype == A.real.dtype
        for b in range(B):
            assert np.array_equal(out[b], f(A[b]))
        assert np.array_equal(f(A[:1])[0], f(A[0]))
    W = _cmap(B, 40, N, dtype=dtype)
    xm = [0.25, -1.5, 3.0, 0.0]
    for sc in (LOG, LIN, PIECE):
        for l1 in (True, False):
            out = up.icwt(W, scales=sc, l1_norm=l1, x_mean=0.5)
            outv = up.icwt(W, scales=sc, l1_norm=l1, x_mean=np.array(xm))
            assert out.shape == outv.shape == (B, N)
            for b in range(B):
                assert np.array_equal(out[b], up.icwt(W[b], scales=sc, l1_norm=l1, x_mean=0.5))
                assert np.array_equal(outv[b], up.icwt(W[b], scales=sc, l1_norm=l1, x_mean=xm[b]))
            assert np.array_equal(up.icwt(W[:1], scales=sc, l1_norm=l1)[0], up.icwt(W[0], scales=sc, l1_norm=l1))


# ------------------------------------------------------------------------- 3. the fused istft against the oracle ----
def _nola(win, hop, win_exp):
    wn = np.zeros(len(win) + 8 * hop * (len(win) // hop + 1))
    for i in range(0, len(wn) - len(win) + 1, hop):
        wn[i:i + len(win)] += win ** (win_exp + 1)
    mid = wn[len(win):-len(win)] if len(wn) > 2 * len(win) else wn
    return mid.min() > 1e-3


def _frames(n_fft, hop, short):
    halo = (n_fft - 1) // hop
    return 7 if short else int(2.3 * max(16, 2 * halo)) + 5        # several tiles and a ragged last one | less than a tile


FUSED_CASES = [(n, h, short) for n in (16, 64, 256, 1024, 4096) for h in sorted({1, 3, n // 4, n})
               for short in (False, True) if not (short and h != 3)]
# (n_fft, hop, frames) long enough for the 256 tiles per signal from which the kernel is chosen without being forced:
# 313 tiles of 128 frames at hop 1; and 2053 tiles of 16 frames, which the plan doubles to 32
LONG_CASES = [(64, 1, 40000), (16, 16, 2 * 1024 * 16 + 77)]


def _is_fused(n_fft, hop, nfr, N):
    fused = C.c_int(-1)
    _lib.load().ssq_istft_batch_workspace_bytes(_lib.SSQ_F64, 1, nfr, n_fft, hop, N, C.byref(fused))
    return fused.value


@pytest.mark.parametrize("cdtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("n_fft,hop,short", FUSED_CASES + LONG_CASES)
def test_fused_istft_against_the_oracle(n_fft, hop, short, cdtype, monkeypatch):
    """Bound per case: e_new <= 4 e_old + 4 eps max|x|, e_old the error of the 2-D `up.istft` (the three-kernel path)
    against `u.istft` on the same spectrum; every (modulated, win_exp, B) of the case is compared.  The short cases
    would take the three-kernel path by themselves (fewer than 256 tiles): SSQ_ISTFT_FUSED=1 holds them on the kernel;
    the long ones must get there unforced."""
    rng = np.random.default_rng(n_fft * 31 + hop)
    nfr = short if short > 1 else _frames(n_fft, hop, short)
    N = hop * nfr - hop // 2
    monkeypatch.delenv("SSQ_ISTFT_FUSED", raising=False)
    if short <= 1:
        monkeypatch.setenv("SSQ_ISTFT_FUSED", "1")
    assert _is_fused(n_fft, hop, nfr, N) == 1
    win = np.hanning(n_fft) + 0.1
    x = rng.standard_normal((5, N))
    eps = np.finfo(np.float32 if cdtype == np.complex64 else np.float64).eps
    for mod in (True, False):
        S = np.stack([u.stft(x[b], win, n_fft=n_fft, hop_len=hop, modulated=mod) for b in range(5)]).astype(cdtype)
        for win_exp in (0, 1, 2):
            assert _nola(win, hop, win_exp)
            kw = dict(n_fft=n_fft, hop_len=hop, N=N, modulated=mod, win_exp=win_exp)
            ref = np.stack([u.istft(S[b], win, **kw) for b in range(5)])
            old = np.stack([up.istft(S[b], win, **kw) for b in range(5)])
            new5 = up.istft(S, win, **kw)
            new1 = up.istft(S[:1], win, **kw)
            assert new5.shape == (5, N) and new5.dtype == old.dtype
            for b in range(5):
                e_old = np.abs(old[b] - ref[b]).max()
                bound = 4 * e_old + 4 * eps * np.abs(ref[b]).max()
                e_new = np.abs(new5[b] - ref[b]).max()
                print(f"n_fft={n_fft} hop={hop} nfr={nfr} {np.dtype(cdtype).name} mod={mod} win_exp={win_exp} b={b} "
                      f"e_old={e_old:.3g} e_new={e_new:.3g} bound={bound:.3g}")
                assert e_new <= bound, (mod, win_exp, b, e_old, e_new)
            assert np.abs(new1[0] - ref[0]).max() <= 4 * np.abs(old[0] - ref[0]).max() + 4 * eps * np.abs(ref[0]).max()


# ----------------------------------------------------------------------------------------- 4. fallback lengths ----
@pytest.mark.parametrize("n_fft,hop", [(120, 1), (121, 3), (1000, 250), (1000, 7), (16, 20), (1024, 1500), (256, 64)])
def test_fallback_lengths(n_fft, hop, monkeypatch):
    """Lengths the fused kernel does not take, hops longer than the frame (gaps no frame covers stay zero), and a
    power of two with too few tiles to be worth the kernel."""
    monkeypatch.delenv("SSQ_ISTFT_FUSED", raising=False)
    rng = np.random.default_rng(n_fft + hop)
    N = 2600 if hop < n_fft else 12 * hop + 5
    x = rng.standard_normal((4, N))
    win = np.hanning(n_fft) + 0.1
    fused = C.c_int(1)
    _lib.load().ssq_istft_batch_workspace_bytes(_lib.SSQ_F64, 4, (N - 1) // hop + 1, n_fft, hop, N, C.byref(fused))
    assert fused.value == 0
    for mod in (True, False):
        S = np.stack([u.stft(x[b], win, n_fft=n_fft, hop_len=hop, modulated=mod) for b in range(4)])
        out = up.istft(S, win, n_fft=n_fft, hop_len=hop, N=N, modulated=mod)
        assert out.shape == (4, N)
        for b in range(4):
            assert np.abs(out[b] - u.istft(S[b], win, n_fft=n_fft, hop_len=hop, N=N, modulated=mod)).max() < 1e-13


# ------------------------------------------------------------- 5. determinism, batch independence, the A/B switch ----
@pytest.mark.parametrize("cdtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("n_fft,hop,frames", [(64, 1, 0), (256, 64, 0), (1024, 3, 0), (4096, 1024, 0), (16, 16, 0),
                                              (64, 1, 40000)])
def test_fused_istft_is_deterministic_and_batch_independent(n_fft, hop, frames, cdtype, monkeypatch):
    rng = np.random.default_rng(n_fft + hop)
    nfr = frames or _frames(n_fft, hop, False)
    N = hop * nfr
    monkeypatch.delenv("SSQ_ISTFT_FUSED", raising=False)
    if not frames:
        monkeypatch.setenv("SSQ_ISTFT_FUSED", "1")
    assert _is_fused(n_fft, hop, nfr, N) == 1
    win = np.hanning(n_fft) + 0.1
    S = np.stack([u.stft(rng.standard_normal(N), win, n_fft=n_fft, hop_len=hop) for _ in range(5)]).astype(cdtype)
    a = up.istft(S, win, hop_len=hop)
    assert np.array_equal(a, up.istft(S, win, hop_len=hop))
    for b in range(5):
        assert np.array_equal(a[b], up.istft(S[b:b + 1], win, hop_len=hop)[0])


_CHILD = r"""
import ctypes as C
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from oracle import upstream_oracle as u
from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
rng = np.random.default_rng(3)
for n_fft, hop, nfr in ((64, 16, 5000), (1024, 256, 4200)):
    N = hop * nfr
    fused = C.c_int(1)
    _lib.load().ssq_istft_batch_workspace_bytes(_lib.SSQ_F64, 3, nfr, n_fft, hop, N, C.byref(fused))
    assert fused.value == 0, "SSQ_ISTFT_FUSED=0 was not honoured"
    win = np.hanning(n_fft) + 0.1
    x = rng.standard_normal((3, N))
    for cdt, eps in ((np.complex128, np.finfo(np.float64).eps), (np.complex64, np.finfo(np.float32).eps)):
        S = np.stack([u.stft(x[b], win, n_fft=n_fft, hop_len=hop) for b in range(3)]).astype(cdt)
        out = up.istft(S, win, hop_len=hop)
        for b in range(3):
            ref = u.istft(S[b], win, hop_len=hop)
            e_old = np.abs(up.istft(S[b], win, hop_len=hop) - ref).max()
            assert np.abs(out[b] - ref).max() <= 4 * e_old + 4 * eps * np.abs(ref).max()
print("child ok")
"""


def test_three_kernel_path_behind_the_switch(monkeypatch):
    """SSQ_ISTFT_FUSED=0 in a fresh child process: the batched entry point on the three-kernel path (the child checks
    that it is), same bound; the same shapes take the kernel here, where the switch is unset."""
    monkeypatch.delenv("SSQ_ISTFT_FUSED", raising=False)
    for n_fft, hop, nfr in ((64, 16, 5000), (1024, 256, 4200)):
        assert _is_fused(n_fft, hop, nfr, hop * nfr) == 1
    env = dict(os.environ, SSQ_ISTFT_FUSED="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr
