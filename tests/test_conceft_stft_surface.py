"""CPU tests of the surface of `upstream.conceft_stft` and `upstream.hermite_windows`: the signatures, every refusal by
its message before the GPU is asked for, and the C entry points exported, declared, bound and refusing bad arguments on the
host."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up

E = inspect.Parameter.empty
NEW = ("ssq_conceft_stft_host", "ssq_conceft_stft_workspace_bytes", "ssq_conceft_stft_exec")
X = np.random.default_rng(0).standard_normal(300)


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
    sig = [(p.name, p.default) for p in inspect.signature(up.conceft_stft).parameters.values()]
    assert sig == [("x", E), ("tapers", None), ("n_fft", None), ("win_len", None), ("hop_len", 1), ("fs", None), ("t", None),
                   ("modulated", True), ("padtype", "reflect"), ("n_tapers", 3), ("n_draws", 20), ("seed", 0),
                   ("vectors", None), ("gamma", None), ("flipud", False), ("get_planes", False), ("get_w", False)]
    sig = [(p.name, p.default) for p in inspect.signature(up.hermite_windows).parameters.values()]
    assert sig == [("n_fft", E), ("n_tapers", E), ("sigma", None)]


def test_docstrings_name_the_feature():
    assert "conceft_stft" in up.__doc__ and "hermite_windows" in up.__doc__
    doc = up.conceft_stft.__doc__
    for word in ("power of two", "gauge", "issq_stft", "atomics", "tapers[0]", "get_planes", "+inf"):
        assert word in doc, word
    assert "NOT orthogonal" in up.hermite_windows.__doc__


def test_entry_points_are_exported_declared_and_bound():
    lib = _lib.load()
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib._SIGNATURES and name in _lib.header_symbols()
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, header)
        assert getattr(lib, name).argtypes == _lib._SIGNATURES[name][1]
    # the declared parameter counts are those of the bound argtypes
    for name in NEW:
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(decl.split(",")) == len(_lib._SIGNATURES[name][1]), name


def test_hermite_windows_refusals():
    for bad in (0, 9, -1, 2.0, True, "3", None):
        with pytest.raises(ValueError, match="n_tapers"):
            up.hermite_windows(64, bad)
    for bad in (0, -4, 64.0, True, None):
        with pytest.raises(ValueError, match="n_fft"):
            up.hermite_windows(bad, 3)
    for bad in (0, -1.0, float("inf"), float("nan"), "4", True):
        with pytest.raises(ValueError, match="sigma"):
            up.hermite_windows(64, 3, bad)
    assert up.hermite_windows(64, 1).shape == (1, 64) and up.hermite_windows(16, 8, sigma=np.float32(2)).shape == (8, 16)
    assert np.array_equal(up.hermite_windows(64, 3), up.hermite_windows(64, 3, 4.0))        # the default: n_fft / 16


@pytest.mark.parametrize("n_fft", [8, 15, 24, 100, 1000, 8192, 0.5, True])
def test_n_fft_refusals_come_before_the_gpu(no_gpu, n_fft):
    x = np.random.default_rng(0).standard_normal(9000)
    with pytest.raises(ValueError, match="n_fft .*conceft_stft takes a power of two from 16 to 4096"):
        up.conceft_stft(x, n_fft=n_fft)
    with pytest.raises(ValueError, match="n_fft"):
        up.conceft_stft(np.zeros(100))                                 # the default, min(N // hop_len, 512) = 100


def test_taper_refusals_come_before_the_gpu(no_gpu):
    h = up.hermite_windows(64, 3)
    for bad in (list(h), h[0], h[None], np.zeros((0, 64)), np.zeros((9, 64)), np.zeros((2, 0)), h.astype(complex), "hermite"):
        with pytest.raises(ValueError, match="`tapers` must be a real ndarray"):
            up.conceft_stft(X, bad, n_fft=64)
    nan = h.copy()
    nan[1, 3] = np.nan
    with pytest.raises(ValueError, match="`tapers` must be finite"):
        up.conceft_stft(X, nan, n_fft=64)
    with pytest.raises(ValueError, match="win_len > n_fft"):
        up.conceft_stft(X, up.hermite_windows(128, 2), n_fft=64)
    zero = h.copy()
    zero[0, 32] = 0.0
    with pytest.raises(ValueError, match="tapers\\[0\\] at the window's centre .* must be finite and non-zero"):
        up.conceft_stft(X, zero, n_fft=64)
    for bad in (0, 9, -1, 2.0, True, "3", None):
        with pytest.raises(ValueError, match="n_tapers"):
            up.conceft_stft(X, n_fft=64, n_tapers=bad)


def test_draw_refusals_come_before_the_gpu(no_gpu):
    h = up.hermite_windows(64, 3)
    for bad in (0, 257, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="n_draws"):
            up.conceft_stft(X, h, n_fft=64, n_draws=bad)
    for bad in (np.ones(3), np.ones((2, 4)), np.ones((2, 3, 1)), np.array([["a", "b", "c"]])):
        with pytest.raises(ValueError, match="`vectors` must be a numeric array \\[n_draws, 3\\]"):
            up.conceft_stft(X, h, n_fft=64, vectors=bad)
    with pytest.raises(ValueError, match="1 .. 256 draws are built"):
        up.conceft_stft(X, h, n_fft=64, vectors=np.ones((257, 3)))
    with pytest.raises(ValueError, match="`vectors` must be finite"):
        up.conceft_stft(X, h, n_fft=64, vectors=np.array([[1.0, np.inf, 0.0]]))
    with pytest.raises(ValueError, match="zero vector"):
        up.conceft_stft(X, h, n_fft=64, vectors=np.zeros((2, 3)))
    # h_1 is odd: it vanishes at the centre, so the draw e_1 has no admittance (the gauge's 1e-6 refusal)
    with pytest.raises(ValueError, match="draw 1 is degenerate"):
        up.conceft_stft(X, h, n_fft=64, vectors=np.array([[1.0, 0, 0], [0, 1.0, 0]]))


def test_other_refusals_come_before_the_gpu(no_gpu):
    h = up.hermite_windows(16, 2)
    with pytest.raises(ValueError, match="padtype"):
        up.conceft_stft(X, h, n_fft=16, padtype="constant")
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="hop_len"):
            up.conceft_stft(X, h, n_fft=16, hop_len=bad)
    with pytest.raises(ValueError, match="gamma is NaN"):
        up.conceft_stft(X, h, n_fft=16, gamma=float("nan"))
    with pytest.raises(TypeError):
        up.conceft_stft(list(X), h, n_fft=16)
    with pytest.raises(ValueError, match="fs must be positive"):
        up.conceft_stft(X, h, n_fft=16, fs=-2.0)


@pytest.mark.parametrize("kw", [dict(), dict(padtype="wrap", flipud=True, modulated=False, get_w=True, get_planes=True,
                                             hop_len=3, fs=2.0, gamma=1e-6, n_draws=256, seed=5),
                                dict(vectors=np.array([[1, 0], [1j, 1]]))])
@pytest.mark.parametrize("shape,dtype", [((300,), np.float64), ((2, 300), np.float32)])
def test_well_formed_calls_reach_the_gpu(no_gpu, kw, shape, dtype):
    x = np.random.default_rng(2).standard_normal(shape).astype(dtype)
    for n_fft in (16, 64, 4096):
        with pytest.raises(_Reached):
            up.conceft_stft(x, up.hermite_windows(16, 2), n_fft=n_fft, **kw)
    with pytest.raises(_Reached):
        up.conceft_stft(x, n_fft=64, n_tapers=8)


def test_c_entry_points_refuse_on_the_host():
    lib = _lib.load()
    mn = C.c_int64(0)
    for code, csz, wid in ((_lib.SSQ_F32, 8, 8 * 1000), (_lib.SSQ_F64, 16, 0)):
        # 1000 samples at hop 7: 143 frames of 33 bins; a store tile of n_fft = 64 is 64 frames
        assert lib.ssq_conceft_stft_workspace_bytes(code, 3, 1000, 64, 7, 3, C.byref(mn)) == 3 * (wid + 6 * 33 * 143 * csz)
        assert mn.value == wid + 6 * 33 * 64 * csz
        assert lib.ssq_conceft_stft_workspace_bytes(code, 3, 1000, 64, 7, 3, None) > 0
        # a signal larger than the preferred 1 GiB: runs of whole store tiles of one signal
        pref = lib.ssq_conceft_stft_workspace_bytes(code, 2, 1 << 22, 1024, 1, 8, C.byref(mn))
        tile = 16 * 513 * 4 * csz
        wide = 8 * (1 << 22) if code == _lib.SSQ_F32 else 0
        assert mn.value == wide + tile and (pref - wide) % tile == 0 and (1 << 30) - tile < pref <= 1 << 30
        for n_fft in (8, 48, 8192):
            assert lib.ssq_conceft_stft_workspace_bytes(code, 1, 1000, n_fft, 1, 3, None) == -1
            assert "conceft_stft: n_fft" in lib.ssq_last_error().decode()
        for args, word in (((0, 1000, 64, 1, 3), "batch"), ((1, 0, 64, 1, 3), "n_signal"), ((1, 1000, 64, 0, 3), "hop"),
                           ((1, 1000, 64, 1, 0), "n_tapers"), ((1, 1000, 64, 1, 9), "n_tapers")):
            assert lib.ssq_conceft_stft_workspace_bytes(code, *args, None) == -1, args
            assert word in lib.ssq_last_error().decode(), args
    assert lib.ssq_conceft_stft_workspace_bytes(7, 1, 1000, 64, 1, 3, None) == -1
    assert "dtype" in lib.ssq_last_error().decode()

    x = np.zeros(100)
    h = np.ascontiguousarray(up.hermite_windows(16, 2))
    r = np.array([[1.0 + 0j, 0.0]])
    out = np.zeros((2, 9, 100), dtype=np.complex128)
    f = np.zeros(9)

    def host(n_fft=16, J=2, hop=1, fs=1.0, pad=0, M=1, scale=1.0, gamma=-1.0, limit=0, xp=_vp(x), hp=_vp(h), rp=_vp(r)):
        return lib.ssq_conceft_stft_host(_lib.SSQ_F64, xp, 1, 100, hp, J, n_fft, hop, fs, pad, rp, M, scale, gamma, 3, limit,
                                         _vp(out), _vp(f), None, None, None)

    nan_h = h.copy()
    nan_h[1, 2] = np.nan
    inf_r = np.array([[1.0 + 0j, np.inf]])
    for kw, word in ((dict(n_fft=24), "n_fft"), (dict(pad=9), "padtype"), (dict(J=0), "n_tapers"), (dict(J=9), "n_tapers"),
                     (dict(hop=0), "hop"), (dict(fs=0.0), "fs"), (dict(M=0), "n_draws"), (dict(M=257), "n_draws"),
                     (dict(scale=0.0), "scale"), (dict(scale=float("nan")), "scale"), (dict(gamma=float("nan")), "gamma"),
                     (dict(xp=None), "NULL"), (dict(hp=None), "NULL"), (dict(rp=None), "NULL"),
                     (dict(hp=_vp(nan_h)), "tapers must be finite"), (dict(rp=_vp(inf_r)), "vectors must be finite"),
                     (dict(limit=-1), "work_limit_bytes"), (dict(limit=100), "work_limit_bytes")):
        assert host(**kw) != 0, kw
        assert word in lib.ssq_last_error().decode(), kw

    def execute(n_fft=16, J=2, M=1, ws=1 << 20, xp=_vp(x), wp=_vp(out)):
        return lib.ssq_conceft_stft_exec(_lib.SSQ_F64, xp, 1, 100, _vp(h), J, n_fft, 1, 1.0, 0, _vp(r), M, 1.0, -1.0, 3, _vp(out),
                                         None, None, None, wp, ws, None, None)

    # (a workspace that is too small is refused before any device work)
    for kw, word in ((dict(n_fft=24), "n_fft"), (dict(J=9), "n_tapers"), (dict(M=0), "n_draws"), (dict(ws=16), "workspace too small"),
                     (dict(xp=None), "NULL"), (dict(wp=None), "NULL")):
        assert execute(**kw) != 0, kw
        assert word in lib.ssq_last_error().decode(), kw
