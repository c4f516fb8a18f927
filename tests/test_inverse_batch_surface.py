"""CPU tests of the batched full inverses (`upstream.istft`, `issq_stft`, `issq_cwt`, `icwt` on [B, F, N]): the two
C entry points exist, every refusal comes before the GPU is asked for, well-formed batches get as far as the GPU, the
signatures are upstream's, and without a GPU the entry points fail with a message instead of crashing."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up

E = inspect.Parameter.empty
NEW = ("ssq_istft_batch_host", "ssq_issq_batch_host", "ssq_istft_batch_exec")


def _sig(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class _Reached(Exception):
    pass


@pytest.fixture
def no_gpu(monkeypatch):
    def refuse():
        raise _Reached("require_gpu")
    monkeypatch.setattr(up._lib, "require_gpu", refuse)


def _cmap(*shape, dtype=np.complex128):
    rng = np.random.default_rng(sum(shape))
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)


LOG = 2.0 ** (np.arange(12) / 4 + 1)
LIN = np.linspace(2.0, 40.0, 12)
PIECE = np.concatenate([2.0 ** (np.arange(8) / 4 + 1), 2.0 ** (np.arange(4) / 2 + 3)])


def test_new_entry_points_are_exported_and_declared():
    lib = _lib.load()
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib._SIGNATURES and name in _lib.header_symbols()
        assert re.search(r"\bint\s+%s\s*\(" % name, header)


def test_signatures_unchanged():
    assert _sig(up.istft) == [("Sx", E), ("window", None), ("n_fft", None), ("win_len", None), ("hop_len", 1),
                              ("N", None), ("modulated", True), ("win_exp", 1)]
    assert _sig(up.issq_stft) == [("Tx", E), ("window", None), ("cc", None), ("cw", None), ("n_fft", None),
                                  ("win_len", None), ("hop_len", 1), ("modulated", True)]
    assert _sig(up.issq_cwt) == [("Tx", E), ("wavelet", "gmw"), ("cc", None), ("cw", None)]
    assert _sig(up.icwt) == [("Wx", E), ("wavelet", "gmw"), ("scales", "log-piecewise"), ("nv", None),
                             ("one_int", True), ("x_len", None), ("x_mean", 0), ("padtype", "reflect"),
                             ("rpadded", False), ("l1_norm", True)]


@pytest.mark.parametrize("lead", [(), (3,)], ids=["2d", "3d"])
def test_refusals_come_before_the_gpu(no_gpu, lead):
    win = np.hanning(16) + 0.1
    bad = (TypeError, ValueError)
    # wrong ndim
    for a in (_cmap(9), _cmap(2, 3, 9, 20)):
        with pytest.raises(bad):
            up.istft(a, win, n_fft=16)
        with pytest.raises(bad):
            up.issq_stft(a, win, n_fft=16)
        with pytest.raises(bad):
            up.issq_cwt(a)
    with pytest.raises(bad):
        up.icwt(_cmap(2, 3, 12, 20), scales=LOG)
    with pytest.raises(bad):
        up.icwt(_cmap(12), scales=LOG)
    # real dtype
    with pytest.raises(bad):
        up.istft(np.zeros(lead + (9, 20)), win, n_fft=16)
    with pytest.raises(bad):
        up.issq_stft(np.zeros(lead + (9, 20)), win, n_fft=16)
    with pytest.raises(bad):
        up.issq_cwt(np.zeros(lead + (12, 20)))
    with pytest.raises(bad):
        up.icwt(np.zeros(lead + (12, 20)), scales=LOG)
    # row count against n_fft / len(scales)
    with pytest.raises(ValueError):
        up.istft(_cmap(*lead, 8, 20), win, n_fft=16)
    with pytest.raises(ValueError):
        up.icwt(_cmap(*lead, 11, 20), scales=LOG)
    with pytest.raises(AssertionError):                     # upstream's own exception type for it, kept
        up.icwt(_cmap(*lead, 11, 20), scales=LOG)
    # what upstream refuses
    with pytest.raises(ValueError):
        up.issq_stft(_cmap(*lead, 9, 20), win, n_fft=16, hop_len=2)
    with pytest.raises(ValueError):
        up.issq_stft(_cmap(*lead, 9, 20), win, n_fft=16, modulated=False)
    with pytest.raises(ValueError):
        up.icwt(_cmap(*lead, 12, 20), scales=LOG, one_int=False)
    with pytest.raises(ValueError):
        up.icwt(_cmap(*lead, 12, 20), scales="log")
    with pytest.raises(ValueError):
        up.istft(_cmap(*lead, 9, 20), win, n_fft=16, win_len=20)
    with pytest.raises(ValueError):
        up.istft(_cmap(*lead, 9, 20), "hann", n_fft=16)


def test_batch_only_refusals_come_before_the_gpu(no_gpu):
    win = np.hanning(16) + 0.1
    for xm in (np.zeros(2), np.zeros(4), np.zeros((3, 1)), np.zeros((3, 20))):
        with pytest.raises(ValueError, match="x_mean"):
            up.icwt(_cmap(3, 12, 20), scales=LOG, x_mean=xm)
        with pytest.raises(ValueError, match="x_mean"):
            up.icwt(_cmap(3, 12, 20), scales=PIECE, x_mean=xm)
    with pytest.raises(ValueError):
        up.istft(_cmap(3, 9, 20)[:0], win, n_fft=16)
    with pytest.raises(ValueError):
        up.issq_stft(_cmap(3, 9, 20)[:0], win, n_fft=16)
    with pytest.raises(ValueError):
        up.issq_cwt(_cmap(3, 12, 20)[:0])
    with pytest.raises(ValueError):
        up.icwt(_cmap(3, 12, 20)[:0], scales=LOG)


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_well_formed_batches_reach_the_gpu(no_gpu, dtype):
    win = np.hanning(16) + 0.1
    with pytest.raises(_Reached):
        up.istft(_cmap(3, 9, 20, dtype=dtype), win, n_fft=16)
    with pytest.raises(_Reached):
        up.istft(_cmap(3, 9, 20, dtype=dtype), win)              # n_fft from Sx.shape[-2]
    with pytest.raises(_Reached):
        up.istft(_cmap(3, 61, 20, dtype=dtype), np.hanning(120), hop_len=3, N=58)
    with pytest.raises(_Reached):
        up.issq_stft(_cmap(3, 9, 20, dtype=dtype), win)          # n_fft from Tx.shape[-2]
    with pytest.raises(_Reached):
        up.issq_cwt(_cmap(3, 12, 20, dtype=dtype))
    for sc in (LOG, LIN, PIECE):
        for l1 in (True, False):
            for xm in (0, 1.5, np.arange(3.0)):
                with pytest.raises(_Reached):
                    up.icwt(_cmap(3, 12, 20, dtype=dtype), scales=sc, l1_norm=l1, x_mean=xm)
    # the 2-D calls are what they were
    with pytest.raises(_Reached):
        up.istft(_cmap(9, 20, dtype=dtype), win)
    with pytest.raises(_Reached):
        up.icwt(_cmap(12, 20, dtype=dtype), scales=PIECE)


def test_entry_points_fail_loudly_without_a_gpu():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    lib = _lib.load()
    S = _cmap(2, 9, 20)
    win = np.hanning(16) + 0.1
    x = np.empty((2, 20))
    rc = lib.ssq_istft_batch_host(_lib.SSQ_F64, _vp(S), 2, 20, _vp(win), 16, 1, 20, 1, 1, _vp(x))
    assert rc != 0 and b"no HIP device visible" in lib.ssq_last_error()
    rc = lib.ssq_issq_batch_host(_lib.SSQ_F64, _vp(S), 2, 9, 20, 1.0, None, _vp(x))
    assert rc != 0 and b"no HIP device visible" in lib.ssq_last_error()
    # argument checks in the style of the single-signal entry points
    assert lib.ssq_istft_batch_host(_lib.SSQ_F64, _vp(S), 0, 20, _vp(win), 16, 1, 20, 1, 1, _vp(x)) != 0
    assert b"batch" in lib.ssq_last_error()
    assert lib.ssq_istft_batch_host(_lib.SSQ_F64, _vp(S), 2, 19, _vp(win), 16, 1, 20, 1, 1, _vp(x)) != 0
    assert b"wrong number of frames" in lib.ssq_last_error()
    assert lib.ssq_istft_batch_host(7, _vp(S), 2, 20, _vp(win), 16, 1, 20, 1, 1, _vp(x)) != 0
    assert lib.ssq_issq_batch_host(_lib.SSQ_F64, None, 2, 9, 20, 1.0, None, _vp(x)) != 0
    assert b"NULL" in lib.ssq_last_error()
    assert lib.ssq_issq_batch_host(_lib.SSQ_F64, _vp(S), 2, 0, 20, 1.0, None, _vp(x)) != 0
    rc = lib.ssq_istft_batch_exec(_lib.SSQ_F64, _vp(S), 2, 20, _vp(win), 16, 1, 20, 1, 1, -1, _vp(x), None)
    assert rc != 0 and b"no HIP device visible" in lib.ssq_last_error()
    assert lib.ssq_istft_batch_exec(_lib.SSQ_F64, _vp(S), 2, 20, _vp(win), 16, 1, 20, 1, 1, 2, _vp(x), None) != 0
    assert b"path" in lib.ssq_last_error()
    with pytest.raises(_lib.SsqHipError):
        up.istft(S, win)
    with pytest.raises(_lib.SsqHipError):
        up.issq_cwt(S)


def test_fused_istft_workspace_is_linear_in_the_signal(monkeypatch):
    """The streaming path's device workspace beside Sx is x and three tables of n_fft entries, exactly: nothing per
    tile, nothing of the expanded [n_frames][n_fft] form that the three-kernel path needs.  Computed on the host.
    A signal of fewer than 256 tiles takes the three-kernel path unless SSQ_ISTFT_FUSED=1 forces the kernel."""
    monkeypatch.delenv("SSQ_ISTFT_FUSED", raising=False)
    lib = _lib.load()
    fused = C.c_int(0)
    N = 1 << 20
    for code, rsz, csz in ((_lib.SSQ_F32, 4, 8), (_lib.SSQ_F64, 8, 16)):
        for n_fft, hop, auto in ((1024, 1, 1), (1024, 256, 1), (4096, 1, 0), (4096, 1024, 0), (16, 16, 1), (256, 3, 1)):
            for B in (1, 16):
                nfr = (N - 1) // hop + 1
                for force in (False, True):
                    if force:
                        monkeypatch.setenv("SSQ_ISTFT_FUSED", "1")
                    w = lib.ssq_istft_batch_workspace_bytes(code, B, nfr, n_fft, hop, N, C.byref(fused))
                    monkeypatch.delenv("SSQ_ISTFT_FUSED", raising=False)
                    assert fused.value == (1 if force else auto), (n_fft, hop, force)
                    if fused.value:
                        assert w == B * N * rsz + n_fft * (16 + csz)
                    else:
                        assert w >= csz * n_fft * nfr
        w = lib.ssq_istft_batch_workspace_bytes(code, 4, 1 << 12, 1000, 1, 1 << 12, C.byref(fused))
        assert fused.value == 0 and w >= csz * 1000 * (1 << 12)
        monkeypatch.setenv("SSQ_ISTFT_FUSED", "1")
        lib.ssq_istft_batch_workspace_bytes(code, 4, 100, 16, 20, 1981, C.byref(fused))       # hop_len > n_fft
        assert fused.value == 0
        monkeypatch.setenv("SSQ_ISTFT_FUSED", "0")
        lib.ssq_istft_batch_workspace_bytes(code, 1, N, 1024, 1, N, C.byref(fused))
        assert fused.value == 0
        monkeypatch.delenv("SSQ_ISTFT_FUSED")
    assert lib.ssq_istft_batch_workspace_bytes(_lib.SSQ_F32, 0, 16, 16, 1, 16, None) == -1
