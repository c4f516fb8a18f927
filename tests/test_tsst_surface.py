"""CPU tests of `upstream.tssq_stft`'s surface: the signature, every refusal before the GPU is asked for, and the C entry
points exported, declared and refusing bad arguments on the host."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up

E = inspect.Parameter.empty
NEW = ("ssq_tssq_stft_host", "ssq_tssq_stft_workspace_bytes", "ssq_tssq_stft_exec")


class _Reached(Exception):
    pass


@pytest.fixture
def no_gpu(monkeypatch):
    def refuse():
        raise _Reached("require_gpu")
    monkeypatch.setattr(up._lib, "require_gpu", refuse)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_signature():
    sig = [(p.name, p.default) for p in inspect.signature(up.tssq_stft).parameters.values()]
    assert sig == [("x", E), ("window", None), ("n_fft", None), ("win_len", None), ("hop_len", 1), ("fs", None),
                   ("t", None), ("modulated", True), ("padtype", "reflect"), ("order", 2), ("gamma", None),
                   ("get_tau", False)]


def test_docstrings_state_the_definition():
    assert "tssq_stft" in up.__doc__
    doc = up.tssq_stft.__doc__
    for word in ("group delay", "power of two", "spill", "V1 D / (V num)", "ascending source frame", "no inverse"):
        assert word in doc, word


def test_entry_points_are_exported_and_declared():
    lib = _lib.load()
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib._SIGNATURES and name in _lib.header_symbols()
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, header)


@pytest.mark.parametrize("n_fft", [8, 15, 24, 100, 1000, 8192, 0.5, True])
def test_n_fft_refusals_come_before_the_gpu(no_gpu, n_fft):
    x = np.random.default_rng(0).standard_normal(9000)
    with pytest.raises(ValueError, match="n_fft"):
        up.tssq_stft(x, np.hanning(8), n_fft=n_fft)


def test_default_n_fft_is_checked_too(no_gpu):
    with pytest.raises(ValueError, match="n_fft"):
        up.tssq_stft(np.zeros(100), np.hanning(8))               # min(N // hop_len, 512) = 100
    with pytest.raises(_Reached):
        up.tssq_stft(np.zeros(600), np.hanning(8))               # 512


@pytest.mark.parametrize("order", [0, 3, -1, 1.5, "2", None, True])
def test_order_refusals_come_before_the_gpu(no_gpu, order):
    with pytest.raises(ValueError, match="order"):
        up.tssq_stft(np.zeros(300), np.hanning(16), n_fft=16, order=order)


def test_other_refusals_come_before_the_gpu(no_gpu):
    x = np.random.default_rng(1).standard_normal(300)
    win = np.hanning(16)
    with pytest.raises(ValueError, match="gamma"):
        up.tssq_stft(x, win, n_fft=16, gamma=float("nan"))
    with pytest.raises(ValueError, match="padtype"):
        up.tssq_stft(x, win, n_fft=16, padtype="constant")
    with pytest.raises(ValueError, match="window"):
        up.tssq_stft(x, None, n_fft=16)
    with pytest.raises(ValueError, match="window"):
        up.tssq_stft(x, "hann", n_fft=16)
    with pytest.raises(ValueError, match="win_len"):
        up.tssq_stft(x, np.hanning(32), n_fft=16)
    with pytest.raises(TypeError):
        up.tssq_stft(list(x), win, n_fft=16)
    with pytest.raises(TypeError):
        up.tssq_stft(np.zeros((2, 3, 40)), win, n_fft=16)
    with pytest.raises(ValueError, match="`t`"):
        up.tssq_stft(x, win, n_fft=16, t=np.arange(10))


@pytest.mark.parametrize("kw", [dict(), dict(order=1), dict(padtype="wrap", order=1, modulated=False, get_tau=True,
                                                           hop_len=3, fs=2.0, gamma=1e-6)])
@pytest.mark.parametrize("shape,dtype", [((300,), np.float64), ((2, 300), np.float32)])
def test_well_formed_calls_reach_the_gpu(no_gpu, kw, shape, dtype):
    x = np.random.default_rng(2).standard_normal(shape).astype(dtype)
    for n_fft in (16, 64, 4096):
        with pytest.raises(_Reached):
            up.tssq_stft(x, np.hanning(16), n_fft=n_fft, **kw)


def test_c_entry_points_refuse_on_the_host():
    lib = _lib.load()
    err = lambda: lib.ssq_last_error().decode()                                      # noqa: E731
    for code in (_lib.SSQ_F32, _lib.SSQ_F64):
        # one int16 target per bin, and for float32 calls the signals widened to fp64
        assert lib.ssq_tssq_stft_workspace_bytes(code, 3, 1000, 64, 7) == 2 * 3 * 33 * 143 + (8 * 3 * 1000 if code == _lib.SSQ_F32 else 0)
        for n_fft in (8, 48, 8192):
            assert lib.ssq_tssq_stft_workspace_bytes(code, 1, 1000, n_fft, 1) == -1
            assert "n_fft" in err()
        assert lib.ssq_tssq_stft_workspace_bytes(code, 0, 1000, 64, 1) == -1 and "batch" in err()
        assert lib.ssq_tssq_stft_workspace_bytes(code, 1, 1000, 64, 0) == -1 and "hop" in err()
        assert lib.ssq_tssq_stft_workspace_bytes(code, 1, 0, 64, 1) == -1 and "n_signal" in err()
    assert lib.ssq_tssq_stft_workspace_bytes(7, 1, 1000, 64, 1) == -1 and "dtype" in err()
    x = np.zeros(100)
    win = np.ones(24)
    out = np.zeros((13, 100), dtype=np.complex128)

    def host(n_fft=16, hop=1, fs=1.0, pad=0, order=2, gamma=-1.0, x_=x):
        return lib.ssq_tssq_stft_host(_lib.SSQ_F64, None if x_ is None else _vp(x_), 1, 100, _vp(win), n_fft, hop, fs, pad,
                                      order, gamma, 3, _vp(out), _vp(out), None)

    def execute(n_fft=16, order=2, gamma=-1.0, ws=out.nbytes):
        return lib.ssq_tssq_stft_exec(_lib.SSQ_F64, _vp(x), 1, 100, _vp(win), n_fft, 1, 1.0, 0, order, gamma, 3, _vp(out),
                                      _vp(out), None, _vp(out), ws, None)
    for call in (host, execute):
        assert call(n_fft=24) != 0 and "n_fft" in err()
        for order in (0, 3):
            assert call(order=order) != 0 and "order" in err()
        assert call(gamma=float("nan")) != 0 and "gamma" in err()
    assert host(pad=9) != 0 and "padtype" in err()
    assert host(fs=0.0) != 0 and "fs" in err()
    assert host(hop=0) != 0 and "hop" in err()
    assert host(x_=None) != 0 and "NULL" in err()
    # a workspace that is too small is refused before any device work
    assert execute(ws=16) != 0 and "workspace" in err()
    if _lib.device_count() < 1:                                                      # a good call gets as far as the device check
        assert host() != 0 and "no HIP device" in err()
