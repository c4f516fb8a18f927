"""CPU tests of the surface of `upstream.mssq_stft` and `upstream.msst_walk`: the signatures, every refusal before the GPU
is asked for, and the C entry points exported, declared, bound and refusing bad arguments on the host."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up

E = inspect.Parameter.empty
NEW = ("ssq_mssq_stft_host", "ssq_mssq_stft_workspace_bytes", "ssq_mssq_stft_exec", "ssq_msst_walk_host",
       "ssq_msst_tile_cols")


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
    sig = [(p.name, p.default) for p in inspect.signature(up.mssq_stft).parameters.values()]
    assert sig == [("x", E), ("window", None), ("n_fft", None), ("win_len", None), ("hop_len", 1), ("fs", None),
                   ("t", None), ("modulated", True), ("padtype", "reflect"), ("squeezing", "sum"), ("gamma", None),
                   ("flipud", False), ("order", 2), ("n_iter", 4), ("get_w", False), ("get_bins", False)]
    assert [(p.name, p.default) for p in inspect.signature(up.msst_walk).parameters.values()] == [("bins", E), ("n_iter", E)]


def test_docstrings_name_the_feature():
    assert "mssq_stft" in up.__doc__ and "msst_walk" in up.__doc__
    doc = up.mssq_stft.__doc__
    for word in ("power of two", "spill", "n_iter", "fixed point", "rows ascending", "flipud"):
        assert word in doc, word


def test_entry_points_are_exported_declared_and_bound():
    lib = _lib.load()
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib._SIGNATURES and name in _lib.header_symbols()
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, header)
        assert getattr(lib, name).argtypes == _lib._SIGNATURES[name][1]


@pytest.mark.parametrize("n_fft", [8, 15, 24, 100, 1000, 8192, 0.5, True])
def test_n_fft_refusals_come_before_the_gpu(no_gpu, n_fft):
    x = np.random.default_rng(0).standard_normal(9000)
    with pytest.raises(ValueError, match="n_fft"):
        up.mssq_stft(x, np.hanning(8), n_fft=n_fft)


@pytest.mark.parametrize("order", [0, 3, -1, 1.5, True, "2", None])
def test_order_refusals_come_before_the_gpu(no_gpu, order):
    with pytest.raises(ValueError, match="order"):
        up.mssq_stft(np.zeros(300), np.hanning(16), n_fft=16, order=order)


@pytest.mark.parametrize("n_iter", [0, -1, 65, 1000, 2.0, 2.5, True, False, "4", None])
def test_n_iter_refusals_come_before_the_gpu(no_gpu, n_iter):
    with pytest.raises(ValueError, match="n_iter"):
        up.mssq_stft(np.zeros(300), np.hanning(16), n_fft=16, n_iter=n_iter)
    with pytest.raises(ValueError, match="n_iter"):
        up.msst_walk(np.zeros((9, 4), dtype=np.int32), n_iter)


def test_other_refusals_come_before_the_gpu(no_gpu):
    x = np.random.default_rng(1).standard_normal(300)
    win = np.hanning(16)
    with pytest.raises(ValueError, match="squeezing"):
        up.mssq_stft(x, win, n_fft=16, squeezing="abs")
    with pytest.raises(ValueError, match="padtype"):
        up.mssq_stft(x, win, n_fft=16, padtype="constant")
    with pytest.raises(ValueError, match="window"):
        up.mssq_stft(x, None, n_fft=16)
    with pytest.raises(ValueError, match="win_len"):
        up.mssq_stft(x, np.hanning(32), n_fft=16)
    with pytest.raises(TypeError):
        up.mssq_stft(list(x), win, n_fft=16)
    with pytest.raises(ValueError, match="n_fft"):
        up.mssq_stft(np.zeros(100), np.hanning(8))               # the default, min(N // hop_len, 512) = 100


def test_walk_refusals_come_before_the_gpu(no_gpu):
    good = np.zeros((9, 4), dtype=np.int32)
    for bad in (good.astype(np.int64), good.astype(np.float32), good.astype(np.int16), list(good), good[0],
                np.zeros((2, 2, 9, 4), dtype=np.int32), np.zeros((2050, 2), dtype=np.int32),
                np.zeros((9, 0), dtype=np.int32)):
        with pytest.raises(ValueError, match="bins"):
            up.msst_walk(bad, 2)
    for v in (-2, 9, 2 ** 20):
        bad = good.copy()
        bad[3, 1] = v
        with pytest.raises(ValueError, match="targets"):
            up.msst_walk(bad, 2)
    edge = good.copy()
    edge[0, 0], edge[1, 1] = -1, 8
    for m in (edge, np.stack([edge, edge]), np.asfortranarray(edge)):
        with pytest.raises(_Reached):
            up.msst_walk(m, 64)


@pytest.mark.parametrize("kw", [dict(), dict(padtype="wrap", squeezing="lebesgue", flipud=True, modulated=False, get_w=True,
                                             get_bins=True, hop_len=3, fs=2.0, gamma=1e-6, order=1, n_iter=64),
                                dict(order=2, n_iter=1, get_bins=True)])
@pytest.mark.parametrize("shape,dtype", [((300,), np.float64), ((2, 300), np.float32)])
def test_well_formed_calls_reach_the_gpu(no_gpu, kw, shape, dtype):
    x = np.random.default_rng(2).standard_normal(shape).astype(dtype)
    for n_fft in (16, 64, 4096):
        with pytest.raises(_Reached):
            up.mssq_stft(x, np.hanning(16), n_fft=n_fft, **kw)


def test_tile_widths():
    """The tile table of DESIGN 4.17: 2^15 / (n_fft / 2) columns, 16 .. 256, and the tile stays inside 66048 bytes."""
    lib = _lib.load()
    table = {9: 256, 33: 256, 129: 256, 257: 128, 513: 64, 1025: 32, 2049: 16}
    for F, cols in table.items():
        assert up.msst_tile_cols(F) == cols and 2 * F * cols <= 66048
    assert up.msst_tile_cols(1) == 256 and up.msst_tile_cols(130) == 128 and up.msst_tile_cols(2000) == 16
    for F in (0, -3, 2050):
        assert lib.ssq_msst_tile_cols(F) == -1
        with pytest.raises(ValueError):
            up.msst_tile_cols(F)


def test_c_entry_points_refuse_on_the_host():
    lib = _lib.load()
    for code in (_lib.SSQ_F32, _lib.SSQ_F64):
        want = lib.ssq_ssq_stft2_workspace_bytes(code, 3, 1000, 64, 7)
        assert want > 0 and lib.ssq_mssq_stft_workspace_bytes(code, 3, 1000, 64, 7) == want
        for n_fft in (8, 48, 8192):
            assert lib.ssq_mssq_stft_workspace_bytes(code, 1, 1000, n_fft, 1) == -1
            assert "n_fft" in lib.ssq_last_error().decode()
        assert lib.ssq_mssq_stft_workspace_bytes(code, 0, 1000, 64, 1) == -1
        assert lib.ssq_mssq_stft_workspace_bytes(code, 1, 1000, 64, 0) == -1
    assert lib.ssq_mssq_stft_workspace_bytes(7, 1, 1000, 64, 1) == -1
    x = np.zeros(100)
    win = np.ones(24)
    out = np.zeros((13, 100), dtype=np.complex128)
    f = np.zeros(13)
    tail = (_vp(out), _vp(f), _vp(out), None, None)

    def host(n_fft=16, pad=0, sq=0, order=2, n_iter=4, xp=_vp(x)):
        return lib.ssq_mssq_stft_host(_lib.SSQ_F64, xp, 1, 100, _vp(win), n_fft, 1, 1.0, pad, sq, -1.0, 3, order, n_iter, *tail)

    for kw, word in ((dict(n_fft=24), "n_fft"), (dict(pad=9), "padtype"), (dict(sq=2), "squeezing"), (dict(order=0), "order"),
                     (dict(order=3), "order"), (dict(n_iter=0), "n_iter"), (dict(n_iter=65), "n_iter"),
                     (dict(xp=None), "NULL")):
        assert host(**kw) != 0, kw
        assert word in lib.ssq_last_error().decode(), kw

    def execute(n_fft=16, order=2, n_iter=4, ws=out.nbytes):
        return lib.ssq_mssq_stft_exec(_lib.SSQ_F64, _vp(x), 1, 100, _vp(win), n_fft, 1, 1.0, 0, 0, -1.0, 3, order, n_iter,
                                      _vp(out), _vp(out), None, None, _vp(out), ws, None)

    # (a workspace that is too small is refused before any device work)
    for kw, word in ((dict(n_fft=24), "n_fft"), (dict(order=5), "order"), (dict(n_iter=-1), "n_iter"), (dict(ws=16), "workspace")):
        assert execute(**kw) != 0, kw
        assert word in lib.ssq_last_error().decode(), kw

    m = np.zeros((2, 9, 5), dtype=np.int32)
    o = np.empty_like(m)
    for args, word in (((None, 2, 9, 5, 2, _vp(o)), "NULL"), ((_vp(m), 2, 9, 5, 2, None), "NULL"),
                       ((_vp(m), 0, 9, 5, 2, _vp(o)), "batch"), ((_vp(m), 2, 0, 5, 2, _vp(o)), "n_rows"),
                       ((_vp(m), 2, 2050, 5, 2, _vp(o)), "n_rows"), ((_vp(m), 2, 9, 0, 2, _vp(o)), "n_cols"),
                       ((_vp(m), 2, 9, 5, 0, _vp(o)), "n_iter"), ((_vp(m), 2, 9, 5, 65, _vp(o)), "n_iter")):
        assert lib.ssq_msst_walk_host(*args) != 0, word
        assert word in lib.ssq_last_error().decode(), word
    for v in (-2, 9):
        m[1, 8, 4] = v
        assert lib.ssq_msst_walk_host(_vp(m), 2, 9, 5, 2, _vp(o)) != 0
        assert "target" in lib.ssq_last_error().decode()
