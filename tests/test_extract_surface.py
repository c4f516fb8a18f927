"""CPU tests of the surface of `upstream.set_stft` and `upstream.tet_stft`: the signatures, every refusal before the GPU is
asked for, and the C entry points exported, declared with the header's arity, sizing their workspace and refusing bad
arguments on the host."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up

E = inspect.Parameter.empty
NEW = ("ssq_extract_stft_host", "ssq_extract_stft_workspace_bytes", "ssq_extract_stft_exec")
BOTH = pytest.mark.parametrize("fn", [up.set_stft, up.tet_stft], ids=["set_stft", "tet_stft"])
COMMON = [("x", E), ("window", None), ("n_fft", None), ("win_len", None), ("hop_len", 1), ("fs", None), ("t", None),
          ("modulated", True), ("padtype", "reflect"), ("order", 2), ("gamma", None), ("get_Sx", True)]


class _Reached(Exception):
    pass


@pytest.fixture
def no_gpu(monkeypatch):
    def refuse():
        raise _Reached("require_gpu")
    monkeypatch.setattr(up._lib, "require_gpu", refuse)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_signatures():
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]     # noqa: E731
    assert sig(up.set_stft) == COMMON + [("get_w", False)]
    assert sig(up.tet_stft) == COMMON + [("get_tau", False)]


def test_docstrings_state_the_definition():
    assert "`set_stft` and `tet_stft`" in up.__doc__
    for word in ("b == k", "round-half-even", "mssq_stft(order=order, n_iter=1)", "no inverse", "bin\n    centre",
                 "power of two", "spill", "+0 + 0i"):
        assert word in up.set_stft.__doc__, word
    for word in ("r == 0", "BEFORE", "clip", "no inverse", "power of two", "spill", "+0 + 0i", "g[n_fft // 2]"):
        assert word in up.tet_stft.__doc__, word


def test_entry_points_are_exported_and_declared_with_the_headers_arity():
    lib = _lib.load()
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib._SIGNATURES and name in _lib.header_symbols()
        decl = re.search(r"\b(int|int64_t)\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl, name
        restype, argtypes = _lib._SIGNATURES[name]
        assert len(argtypes) == len(decl.group(2).split(",")), name
        assert restype is (C.c_int64 if decl.group(1) == "int64_t" else C.c_int), name


@BOTH
@pytest.mark.parametrize("n_fft", [0, 8, 24, 8192])
def test_n_fft_refusals_come_before_the_gpu(no_gpu, fn, n_fft):
    x = np.random.default_rng(0).standard_normal(9000)
    if n_fft == 0:                                               # 0 asks for the default, min(N // hop_len, 512): 100 here
        x, n_fft = x[:100], None
    with pytest.raises(ValueError, match="n_fft"):
        fn(x, np.hanning(8), n_fft=n_fft)


@BOTH
@pytest.mark.parametrize("order", [0, 3, True])
def test_order_refusals_come_before_the_gpu(no_gpu, fn, order):
    with pytest.raises(ValueError, match="order"):
        fn(np.zeros(300), np.hanning(16), n_fft=16, order=order)


@BOTH
def test_other_refusals_come_before_the_gpu(no_gpu, fn):
    x = np.random.default_rng(1).standard_normal(300)
    win = np.hanning(16)
    with pytest.raises(ValueError, match="padtype"):
        fn(x, win, n_fft=16, padtype="foo")
    with pytest.raises(ValueError, match="window"):
        fn(x, None, n_fft=16)
    with pytest.raises(ValueError, match="window"):
        fn(x, "hann", n_fft=16)
    with pytest.raises(ValueError, match="gamma"):
        fn(x, win, n_fft=16, gamma=float("nan"))
    with pytest.raises(TypeError):
        fn(np.zeros((2, 3, 40)), win, n_fft=16)
    with pytest.raises(TypeError):
        fn(list(x), win, n_fft=16)


@BOTH
@pytest.mark.parametrize("kw", [dict(), dict(order=1, get_Sx=False),
                                dict(padtype="wrap", order=1, modulated=False, hop_len=3, fs=2.0, gamma=1e-6)])
@pytest.mark.parametrize("shape,dtype", [((300,), np.float64), ((2, 300), np.float32)])
def test_well_formed_calls_reach_the_gpu(no_gpu, fn, kw, shape, dtype):
    x = np.random.default_rng(2).standard_normal(shape).astype(dtype)
    for n_fft in (16, 64, 4096):
        with pytest.raises(_Reached):
            fn(x, np.hanning(16), n_fft=n_fft, **kw)


def test_workspace_bytes():
    """0 for float64, the widened signals (batch N 8 bytes, no padding) for float32, -1 on a refused shape."""
    lib = _lib.load()
    err = lambda: lib.ssq_last_error().decode()                                      # noqa: E731
    for batch, N, n_fft, hop in ((1, 40, 64, 1), (3, 1000, 64, 7), (70000, 16, 16, 1), (2, 5000, 4096, 64)):
        assert lib.ssq_extract_stft_workspace_bytes(_lib.SSQ_F64, batch, N, n_fft, hop) == 0
        assert lib.ssq_extract_stft_workspace_bytes(_lib.SSQ_F32, batch, N, n_fft, hop) == 8 * batch * N
    for code in (_lib.SSQ_F32, _lib.SSQ_F64):
        for n_fft in (0, 8, 24, 8192):
            assert lib.ssq_extract_stft_workspace_bytes(code, 1, 1000, n_fft, 1) == -1 and "n_fft" in err()
        assert lib.ssq_extract_stft_workspace_bytes(code, 0, 1000, 64, 1) == -1 and "batch" in err()
        assert lib.ssq_extract_stft_workspace_bytes(code, 1, 1000, 64, 0) == -1 and "hop" in err()
        assert lib.ssq_extract_stft_workspace_bytes(code, 1, 0, 64, 1) == -1 and "n_signal" in err()
    assert lib.ssq_extract_stft_workspace_bytes(7, 1, 1000, 64, 1) == -1 and "dtype" in err()


def test_c_entry_points_refuse_on_the_host():
    lib = _lib.load()
    err = lambda: lib.ssq_last_error().decode()                                      # noqa: E731
    x = np.zeros(100)
    x32 = np.zeros(100, dtype=np.float32)
    win = np.ones(24)
    out = np.zeros((13, 100), dtype=np.complex128)

    def host(n_fft=16, hop=1, fs=1.0, pad=0, axis=0, order=2, gamma=-1.0, x_=x, Te=out):
        return lib.ssq_extract_stft_host(_lib.SSQ_F64, None if x_ is None else _vp(x_), 1, 100, _vp(win), n_fft, hop, fs,
                                         pad, axis, order, gamma, 3, None if Te is None else _vp(Te), None, None)

    def execute(n_fft=16, axis=0, order=2, gamma=-1.0, code=_lib.SSQ_F64, ws=0, work=None):
        xin = x if code == _lib.SSQ_F64 else x32
        return lib.ssq_extract_stft_exec(code, _vp(xin), 1, 100, _vp(win), n_fft, 1, 1.0, 0, axis, order, gamma, 3,
                                         _vp(out), None, None, work, ws, None)
    for call in (host, execute):
        assert call(n_fft=24) != 0 and "n_fft" in err()
        for order in (0, 3):
            assert call(order=order) != 0 and "order" in err()
        for axis in (-1, 2):
            assert call(axis=axis) != 0 and "axis" in err()
        assert call(gamma=float("nan")) != 0 and "gamma" in err()
    assert host(pad=9) != 0 and "padtype" in err()
    assert host(fs=0.0) != 0 and "fs" in err()
    assert host(hop=0) != 0 and "hop" in err()
    assert host(x_=None) != 0 and "NULL" in err()
    assert host(Te=None) != 0 and "NULL" in err()
    # a float32 call's workspace one byte short, and a missing one, are refused before any device work
    assert execute(code=_lib.SSQ_F32, ws=8 * 100 - 1, work=_vp(out)) != 0 and "workspace" in err()
    assert execute(code=_lib.SSQ_F32, ws=8 * 100, work=None) != 0 and "NULL" in err()
    if _lib.device_count() < 1:
        # a good call gets as far as the device check -- a float64 one with a NULL workspace of 0 bytes included
        assert host() != 0 and "no HIP device" in err()
        assert execute() != 0 and "no HIP device" in err()
