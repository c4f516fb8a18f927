"""CPU tests of `upstream.ssq_stft2`'s surface: the signature, every refusal before the GPU is asked for, and the C entry
points exported, declared and refusing bad shapes on the host; the window tables the library builds."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up

E = inspect.Parameter.empty
NEW = ("ssq_ssq_stft2_host", "ssq_ssq_stft2_workspace_bytes", "ssq_ssq_stft2_exec", "ssq_ssq_stft2_window_tables")


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
    sig = [(p.name, p.default) for p in inspect.signature(up.ssq_stft2).parameters.values()]
    assert sig == [("x", E), ("window", None), ("n_fft", None), ("win_len", None), ("hop_len", 1), ("fs", None),
                   ("t", None), ("modulated", True), ("padtype", "reflect"), ("squeezing", "sum"), ("gamma", None),
                   ("flipud", False), ("get_w", False)]


def test_docstrings_name_the_feature():
    assert "ssq_stft2" in up.__doc__
    assert "power of two" in up.ssq_stft2.__doc__ and "spill" in up.ssq_stft2.__doc__


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
        up.ssq_stft2(x, np.hanning(8), n_fft=n_fft)


def test_default_n_fft_is_checked_too(no_gpu):
    with pytest.raises(ValueError, match="n_fft"):
        up.ssq_stft2(np.zeros(100), np.hanning(8))               # min(N // hop_len, 512) = 100
    with pytest.raises(_Reached):
        up.ssq_stft2(np.zeros(600), np.hanning(8))               # 512


def test_other_refusals_come_before_the_gpu(no_gpu):
    x = np.random.default_rng(1).standard_normal(300)
    win = np.hanning(16)
    with pytest.raises(ValueError, match="squeezing"):
        up.ssq_stft2(x, win, n_fft=16, squeezing="abs")
    with pytest.raises(ValueError, match="padtype"):
        up.ssq_stft2(x, win, n_fft=16, padtype="constant")
    with pytest.raises(ValueError, match="window"):
        up.ssq_stft2(x, None, n_fft=16)
    with pytest.raises(ValueError, match="window"):
        up.ssq_stft2(x, "hann", n_fft=16)
    with pytest.raises(ValueError, match="win_len"):
        up.ssq_stft2(x, np.hanning(32), n_fft=16)
    with pytest.raises(TypeError):
        up.ssq_stft2(list(x), win, n_fft=16)
    with pytest.raises(TypeError):
        up.ssq_stft2(np.zeros((2, 3, 40)), win, n_fft=16)
    with pytest.raises(ValueError, match="`t`"):
        up.ssq_stft2(x, win, n_fft=16, t=np.arange(10))


@pytest.mark.parametrize("kw", [dict(), dict(padtype="wrap", squeezing="lebesgue", flipud=True, modulated=False,
                                             get_w=True, hop_len=3, fs=2.0, gamma=1e-6)])
@pytest.mark.parametrize("shape,dtype", [((300,), np.float64), ((2, 300), np.float32)])
def test_well_formed_calls_reach_the_gpu(no_gpu, kw, shape, dtype):
    x = np.random.default_rng(2).standard_normal(shape).astype(dtype)
    for n_fft in (16, 64, 4096):
        with pytest.raises(_Reached):
            up.ssq_stft2(x, np.hanning(16), n_fft=n_fft, **kw)


def test_c_entry_points_refuse_on_the_host():
    lib = _lib.load()
    for code in (_lib.SSQ_F32, _lib.SSQ_F64):
        esz = 8 if code == _lib.SSQ_F32 else 16
        # the map, and for float32 calls the signals widened to fp64
        assert lib.ssq_ssq_stft2_workspace_bytes(code, 3, 1000, 64, 7) == esz * 3 * 33 * 143 + (8 * 3 * 1000 if esz == 8 else 0)
        for n_fft in (8, 48, 8192):
            assert lib.ssq_ssq_stft2_workspace_bytes(code, 1, 1000, n_fft, 1) == -1
            assert "n_fft" in lib.ssq_last_error().decode()
        assert lib.ssq_ssq_stft2_workspace_bytes(code, 0, 1000, 64, 1) == -1
        assert lib.ssq_ssq_stft2_workspace_bytes(code, 1, 1000, 64, 0) == -1
    assert lib.ssq_ssq_stft2_workspace_bytes(7, 1, 1000, 64, 1) == -1
    x = np.zeros(100)
    win = np.ones(24)
    out = np.zeros((13, 100), dtype=np.complex128)
    f = np.zeros(13)
    args = (_vp(x), 1, 100, _vp(win), 24, 1, 1.0, 0, 0, -1.0, 3, _vp(out), _vp(f), _vp(out), None)
    assert lib.ssq_ssq_stft2_host(_lib.SSQ_F64, *args) != 0                          # n_fft = 24, refused on the host
    assert "n_fft" in lib.ssq_last_error().decode()
    ok = (_vp(x), 1, 100, _vp(win), 16, 1, 1.0)
    assert lib.ssq_ssq_stft2_host(_lib.SSQ_F64, *ok, 9, 0, -1.0, 3, _vp(out), _vp(f), _vp(out), None) != 0
    assert "padtype" in lib.ssq_last_error().decode()
    assert lib.ssq_ssq_stft2_host(_lib.SSQ_F64, *ok, 0, 2, -1.0, 3, _vp(out), _vp(f), _vp(out), None) != 0
    assert "squeezing" in lib.ssq_last_error().decode()
    assert lib.ssq_ssq_stft2_host(_lib.SSQ_F64, None, 1, 100, _vp(win), 16, 1, 1.0, 0, 0, -1.0, 3, _vp(out), _vp(f),
                                  _vp(out), None) != 0
    assert lib.ssq_ssq_stft2_exec(_lib.SSQ_F64, _vp(x), 1, 100, _vp(win), 24, 1, 1.0, 0, 0, -1.0, 3, _vp(out), _vp(out),
                                  None, _vp(out), out.nbytes, None) != 0
    assert "n_fft" in lib.ssq_last_error().decode()
    # a workspace that is too small is refused before any device work
    assert lib.ssq_ssq_stft2_exec(_lib.SSQ_F64, _vp(x), 1, 100, _vp(win), 16, 1, 1.0, 0, 0, -1.0, 3, _vp(out), _vp(out),
                                  None, _vp(out), 16, None) != 0
    assert "workspace" in lib.ssq_last_error().decode()


@pytest.mark.parametrize("n", [16, 256, 1024, 4096])
def test_window_tables_are_the_definitions(n):
    """The library's fp64 tables against the numpy model's.  tg and tg1 are exact products.  g1 and g2 are spectral
    derivatives by FFT: rounding noise of 1e-16 of the spectrum's peak sits on every bin and is multiplied by xi (g1)
    or xi^2 (g2) up to the highest bin, pi, while the window's own band lies at xi ~ 1 / sigma = 10 / n, so two FFTs
    agree to about 1e-16 (pi n / 10) and 1e-16 (pi n / 10)^2 of the table's size; the bounds leave a factor 30."""
    from tests.helpers import sst2_ref as m
    lib = _lib.load()
    g = m.gauss_window(n, n / 10.0)
    t = [np.empty(n) for _ in range(4)]
    assert lib.ssq_ssq_stft2_window_tables(_vp(g), n, *[_vp(a) for a in t]) == 0
    g1, g2, tg, tg1 = t
    _, r1, r2, rt, _ = m.window_tables(g, n)
    u = np.arange(n) - n // 2
    assert np.array_equal(tg, rt) and np.array_equal(tg1, u * g1)
    amp = np.pi * n / 10
    e1, e2 = np.abs(g1 - r1).max() / np.abs(r1).max(), np.abs(g2 - r2).max() / np.abs(r2).max()
    print("g1 %.3g (bound %.3g)  g2 %.3g (bound %.3g)" % (e1, 30 * 1.1e-16 * amp, e2, 30 * 1.1e-16 * amp ** 2))
    assert e1 <= 30 * 1.1e-16 * amp and e2 <= 30 * 1.1e-16 * amp ** 2
    assert lib.ssq_ssq_stft2_window_tables(_vp(g), 24, *[_vp(a) for a in t]) != 0
    assert lib.ssq_ssq_stft2_window_tables(None, 16, *[_vp(a) for a in t]) != 0
