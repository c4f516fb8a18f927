"""CPU tests of `upstream.reassign_stft`'s surface: the signature, every refusal before the GPU is asked for, the published
quantum, and the C entry points exported, declared and refusing bad arguments on the host."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up

E = inspect.Parameter.empty
NEW = ("ssq_reassign_stft_host", "ssq_reassign_stft_workspace_bytes", "ssq_reassign_stft_exec")


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
    sig = [(p.name, p.default) for p in inspect.signature(up.reassign_stft).parameters.values()]
    assert sig == [("x", E), ("window", None), ("n_fft", None), ("win_len", None), ("hop_len", 1), ("fs", None),
                   ("t", None), ("modulated", True), ("padtype", "reflect"), ("gamma", None), ("get_w", False),
                   ("get_tau", False)]


def test_the_quantum_is_published():
    assert isinstance(up.REASSIGN_QUANTUM_LOG2, int) and up.REASSIGN_QUANTUM_LOG2 == -38
    # a cell takes at most (2 H + 1) F < 2^24 contributions of at most 2^38 quanta each: inside 63 bits
    H, F = 2048, 2049
    assert (2 * H + 1) * F < 2 ** 24 and 24 - up.REASSIGN_QUANTUM_LOG2 < 63
    with open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "stft_reassign.hip")) as f:
        assert re.search(r"kReassignQuantumLog2\s*=\s*%d\s*;" % up.REASSIGN_QUANTUM_LOG2, f.read())


def test_docstrings_state_the_definition():
    assert "reassign_stft" in up.__doc__
    doc = up.reassign_stft.__doc__
    for word in ("group delay", "instantaneous frequency", "power of two", "spill", "Im(V1 / V)", "Re(Vt / V)", "2^-38",
                 "REASSIGN_QUANTUM_LOG2", "First order only", "conserves energy"):
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
        up.reassign_stft(x, np.hanning(8), n_fft=n_fft)


def test_default_n_fft_is_checked_too(no_gpu):
    with pytest.raises(ValueError, match="n_fft"):
        up.reassign_stft(np.zeros(100), np.hanning(8))               # min(N // hop_len, 512) = 100
    with pytest.raises(_Reached):
        up.reassign_stft(np.zeros(600), np.hanning(8))               # 512


def test_other_refusals_come_before_the_gpu(no_gpu):
    x = np.random.default_rng(1).standard_normal(300)
    win = np.hanning(16)
    with pytest.raises(ValueError, match="gamma"):
        up.reassign_stft(x, win, n_fft=16, gamma=float("nan"))
    with pytest.raises(ValueError, match="padtype"):
        up.reassign_stft(x, win, n_fft=16, padtype="constant")
    with pytest.raises(ValueError, match="window"):
        up.reassign_stft(x, None, n_fft=16)
    with pytest.raises(ValueError, match="window"):
        up.reassign_stft(x, "hann", n_fft=16)
    with pytest.raises(ValueError, match="win_len"):
        up.reassign_stft(x, np.hanning(32), n_fft=16)
    with pytest.raises(TypeError):
        up.reassign_stft(list(x), win, n_fft=16)
    with pytest.raises(TypeError):
        up.reassign_stft(np.zeros((2, 3, 40)), win, n_fft=16)
    with pytest.raises(ValueError, match="`t`"):
        up.reassign_stft(x, win, n_fft=16, t=np.arange(10))


@pytest.mark.parametrize("kw", [dict(), dict(get_w=True), dict(padtype="wrap", modulated=False, get_w=True, get_tau=True,
                                                              hop_len=3, fs=2.0, gamma=1e-6)])
@pytest.mark.parametrize("shape,dtype", [((300,), np.float64), ((2, 300), np.float32)])
def test_well_formed_calls_reach_the_gpu(no_gpu, kw, shape, dtype):
    x = np.random.default_rng(2).standard_normal(shape).astype(dtype)
    for n_fft in (16, 64, 4096):
        with pytest.raises(_Reached):
            up.reassign_stft(x, np.hanning(16), n_fft=n_fft, **kw)


def test_c_entry_points_refuse_on_the_host():
    lib = _lib.load()
    err = lambda: lib.ssq_last_error().decode()                                      # noqa: E731
    for code in (_lib.SSQ_F32, _lib.SSQ_F64):
        # one packed 4-byte target per bin, 8 bytes a signal for its maximum, and for float32 calls the signals widened
        # to fp64
        assert lib.ssq_reassign_stft_workspace_bytes(code, 3, 1000, 64, 7) == (4 * 3 * 33 * 143 + 8 * 3 +
                                                                             (8 * 3 * 1000 if code == _lib.SSQ_F32 else 0))
        for n_fft in (16, 1024, 4096):
            assert lib.ssq_reassign_stft_workspace_bytes(code, 1, 5000, n_fft, 1) > 0
        for n_fft in (8, 48, 8192):
            assert lib.ssq_reassign_stft_workspace_bytes(code, 1, 1000, n_fft, 1) == -1
            assert "n_fft" in err()
        assert lib.ssq_reassign_stft_workspace_bytes(code, 0, 1000, 64, 1) == -1 and "batch" in err()
        assert lib.ssq_reassign_stft_workspace_bytes(code, 1, 1000, 64, 0) == -1 and "hop" in err()
        assert lib.ssq_reassign_stft_workspace_bytes(code, 1, 0, 64, 1) == -1 and "n_signal" in err()
    assert lib.ssq_reassign_stft_workspace_bytes(7, 1, 1000, 64, 1) == -1 and "dtype" in err()
    x = np.zeros(100)
    win = np.ones(24)
    out = np.zeros((13, 100), dtype=np.complex128)

    def host(n_fft=16, hop=1, fs=1.0, pad=0, gamma=-1.0, x_=x):
        return lib.ssq_reassign_stft_host(_lib.SSQ_F64, None if x_ is None else _vp(x_), 1, 100, _vp(win), n_fft, hop, fs,
                                          pad, gamma, 3, _vp(out), _vp(out), None, None)

    def execute(n_fft=16, gamma=-1.0, ws=out.nbytes):
        return lib.ssq_reassign_stft_exec(_lib.SSQ_F64, _vp(x), 1, 100, _vp(win), n_fft, 1, 1.0, 0, gamma, 3, _vp(out),
                                          _vp(out), None, None, _vp(out), ws, None)
    for call in (host, execute):
        assert call(n_fft=24) != 0 and "n_fft" in err()
        assert call(gamma=float("nan")) != 0 and "gamma" in err()
    assert host(pad=9) != 0 and "padtype" in err()
    assert host(fs=0.0) != 0 and "fs" in err()
    assert host(hop=0) != 0 and "hop" in err()
    assert host(x_=None) != 0 and "NULL" in err()
    # a workspace that is too small is refused before any device work
    assert execute(ws=16) != 0 and "workspace" in err()
    if _lib.device_count() < 1:                                                      # a good call gets as far as the device check
        assert host() != 0 and "no HIP device" in err()
