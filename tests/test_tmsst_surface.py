"""CPU tests of the surface of `upstream.tmssq_stft`, `upstream.tmsst_walk` and `upstream.tmsst_tile_frames`: the
signatures, every refusal before the GPU is asked for, and the C entry points exported, declared, bound and refusing bad
arguments on the host."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up

E = inspect.Parameter.empty
i64, vp = C.c_int64, C.c_void_p
NEW = {
    "ssq_tmssq_stft_host": (C.c_int, [C.c_int, vp, i64, i64, vp, i64, i64, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int,
                                      C.c_int, vp, vp, vp, vp]),
    "ssq_tmssq_stft_workspace_bytes": (i64, [C.c_int, i64, i64, i64, i64, C.c_int]),
    "ssq_tmssq_stft_exec": (C.c_int, [C.c_int, vp, i64, i64, vp, i64, i64, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int,
                                      C.c_int, vp, vp, vp, vp, vp, i64, C.POINTER(C.c_float)]),
    "ssq_tmsst_walk_host": (C.c_int, [vp, i64, i64, i64, C.c_int, i64, vp]),
    "ssq_tmsst_tile_frames": (C.c_int, [i64, C.c_int]),
}


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
    sig = [(p.name, p.default) for p in inspect.signature(up.tmssq_stft).parameters.values()]
    assert sig == [("x", E), ("window", None), ("n_fft", None), ("win_len", None), ("hop_len", 1), ("fs", None),
                   ("t", None), ("modulated", True), ("padtype", "reflect"), ("order", 2), ("gamma", None), ("n_iter", 4),
                   ("get_tau", False), ("get_targets", False)]
    assert [(p.name, p.default) for p in inspect.signature(up.tmsst_walk).parameters.values()] == \
        [("targets", E), ("n_iter", E), ("reach", E)]
    assert [(p.name, p.default) for p in inspect.signature(up.tmsst_tile_frames).parameters.values()] == \
        [("reach", E), ("n_iter", E)]


def test_docstrings_name_the_feature():
    assert "tmssq_stft" in up.__doc__ and "tmsst_walk" in up.__doc__
    doc = up.tmssq_stft.__doc__
    for word in ("power of two", "spill", "n_iter", "fixed point", "ascending source frame", "16384", "There is no"):
        assert word in doc, word


def test_entry_points_are_exported_declared_and_bound():
    lib = _lib.load()
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for name, (res, args) in NEW.items():
        assert hasattr(lib, name), name
        assert name in _lib.header_symbols()
        assert _lib._SIGNATURES[name] == (res, args), name
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, header)
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    # the header's argument lists, by name and in order
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)

    def names(fn):
        params = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % fn, src).group(1).split(",")
        return [re.split(r"[\s*]+", p.strip())[-1] for p in params]

    front = ["dtype", "x", "batch", "n_signal", "window", "n_fft", "hop", "fs", "padtype", "order", "gamma", "variant", "n_iter"]
    assert names("ssq_tmssq_stft_host") == front + ["Tx", "Sx", "tau", "targets"]
    assert names("ssq_tmssq_stft_exec") == ["dtype", "d_x"] + front[2:] + ["d_Tx", "d_Sx", "d_tau", "d_targets", "d_workspace",
                                                                           "workspace_bytes", "kernel_ms"]
    assert names("ssq_tmssq_stft_workspace_bytes") == ["dtype", "batch", "n_signal", "n_fft", "hop", "n_iter"]
    assert names("ssq_tmsst_walk_host") == ["targets_in", "batch", "n_rows", "n_frames", "n_iter", "reach", "targets_out"]
    assert names("ssq_tmsst_tile_frames") == ["reach", "n_iter"]
    assert names("ssq_tmssq_stft_host")[:12] == names("ssq_tssq_stft_host")[:12]


@pytest.mark.parametrize("n_fft", [8, 15, 24, 100, 1000, 8192, 0.5, True])
def test_n_fft_refusals_come_before_the_gpu(no_gpu, n_fft):
    x = np.random.default_rng(0).standard_normal(9000)
    with pytest.raises(ValueError, match="n_fft"):
        up.tmssq_stft(x, np.hanning(8), n_fft=n_fft)


@pytest.mark.parametrize("order", [0, 3, -1, 1.5, True, "2", None])
def test_order_refusals_come_before_the_gpu(no_gpu, order):
    with pytest.raises(ValueError, match="order"):
        up.tmssq_stft(np.zeros(300), np.hanning(16), n_fft=16, order=order)


@pytest.mark.parametrize("n_iter", [0, -1, 65, 1000, 2.0, 2.5, True, False, "4", None])
def test_n_iter_refusals_come_before_the_gpu(no_gpu, n_iter):
    with pytest.raises(ValueError, match="n_iter"):
        up.tmssq_stft(np.zeros(300), np.hanning(16), n_fft=16, n_iter=n_iter)
    with pytest.raises(ValueError, match="n_iter"):
        up.tmsst_walk(np.zeros((9, 4), dtype=np.int32), n_iter, 1)


@pytest.mark.parametrize("n_fft,hop,n_iter", [(4096, 1, 9), (4096, 1, 64), (4096, 2, 17), (1024, 1, 33), (2048, 1, 17)])
def test_reach_refusals_come_before_the_gpu(no_gpu, n_fft, hop, n_iter):
    """n_iter ceil(n_fft / (2 hop)) > 16384"""
    x = np.zeros(5000)
    with pytest.raises(ValueError, match="16384"):
        up.tmssq_stft(x, np.hanning(16), n_fft=n_fft, hop_len=hop, n_iter=n_iter)
    assert _lib.load().ssq_tmssq_stft_workspace_bytes(_lib.SSQ_F64, 1, 5000, n_fft, hop, n_iter) == -1
    assert "16384" in _lib.load().ssq_last_error().decode()


@pytest.mark.parametrize("n_fft,hop,n_iter", [(4096, 1, 8), (4096, 2, 16), (1024, 1, 32), (512, 1, 64), (256, 1, 64)])
def test_the_largest_reaches_are_accepted(no_gpu, n_fft, hop, n_iter):
    with pytest.raises(_Reached):
        up.tmssq_stft(np.zeros(5000), np.hanning(16), n_fft=n_fft, hop_len=hop, n_iter=n_iter)
    assert _lib.load().ssq_tmssq_stft_workspace_bytes(_lib.SSQ_F64, 1, 5000, n_fft, hop, n_iter) > 0


def test_other_refusals_come_before_the_gpu(no_gpu):
    x = np.random.default_rng(1).standard_normal(300)
    win = np.hanning(16)
    with pytest.raises(ValueError, match="padtype"):
        up.tmssq_stft(x, win, n_fft=16, padtype="constant")
    with pytest.raises(ValueError, match="window"):
        up.tmssq_stft(x, None, n_fft=16)
    with pytest.raises(ValueError, match="win_len"):
        up.tmssq_stft(x, np.hanning(32), n_fft=16)
    with pytest.raises(ValueError, match="gamma"):
        up.tmssq_stft(x, win, n_fft=16, gamma=float("nan"))
    with pytest.raises(TypeError):
        up.tmssq_stft(list(x), win, n_fft=16)
    with pytest.raises(ValueError, match="n_fft"):
        up.tmssq_stft(np.zeros(100), np.hanning(8))               # the default, min(N // hop_len, 512) = 100


def test_walk_refusals_come_before_the_gpu(no_gpu):
    good = np.tile(np.arange(4, dtype=np.int32), (9, 1))
    for bad in (good.astype(np.int64), good.astype(np.float32), good.astype(np.int16), good.tolist(), good[0],
                np.zeros((2, 2, 9, 4), dtype=np.int32), np.zeros((9, 0), dtype=np.int32), np.zeros((0, 9, 4), dtype=np.int32)):
        with pytest.raises(ValueError, match="targets"):
            up.tmsst_walk(bad, 2, 1)
    for v in (-2, 4, 2 ** 20):
        bad = good.copy()
        bad[3, 1] = v
        with pytest.raises(ValueError, match="outside"):
            up.tmsst_walk(bad, 2, 4)
    far = good.copy()
    far[3, 0] = 3                                             # three frames from its own
    with pytest.raises(ValueError, match="farther"):
        up.tmsst_walk(far, 2, 2)
    for reach in (0, -1, 1.5, True, None, "1"):
        with pytest.raises(ValueError, match="reach"):
            up.tmsst_walk(good, 2, reach)
    for n_iter, reach in ((2, 8193), (64, 257), (1, 16385), (9, 2048)):
        with pytest.raises(ValueError, match="16384"):
            up.tmsst_walk(good, n_iter, reach)
    edge = good.copy()
    edge[0, 0], edge[1, 1], edge[3, 0] = -1, 3, 3
    for m, n_iter, reach in ((edge, 64, 3), (np.stack([edge, edge]), 8, 2048), (np.asfortranarray(edge), 1, 16384),
                             (edge, np.int64(2), np.int32(3))):
        with pytest.raises(_Reached):
            up.tmsst_walk(m, n_iter, reach)


@pytest.mark.parametrize("kw", [dict(), dict(padtype="wrap", modulated=False, get_tau=True, get_targets=True, hop_len=3, fs=2.0,
                                             gamma=1e-6, order=1, n_iter=5),
                                dict(order=2, n_iter=1, get_targets=True)])
@pytest.mark.parametrize("shape,dtype", [((300,), np.float64), ((2, 300), np.float32)])
def test_well_formed_calls_reach_the_gpu(no_gpu, kw, shape, dtype):
    x = np.random.default_rng(2).standard_normal(shape).astype(dtype)
    for n_fft in (16, 64, 4096):
        with pytest.raises(_Reached):
            up.tmssq_stft(x, np.hanning(16), n_fft=n_fft, **kw)


def test_tile_frames():
    """The tile table of DESIGN 4.21: 1024 frames up to a reach n_iter H of 511, then twice the reach rounded up to 256, 4096
    from a reach of 2048 on; the stage of tile + 2 reach targets stays inside 36864."""
    lib = _lib.load()
    table = {(1, 1): 1024, (128, 1): 1024, (128, 3): 1024, (128, 4): 1024, (128, 5): 1280, (8, 64): 1024, (2048, 1): 4096,
             (2048, 8): 4096, (1000, 2): 4096, (300, 3): 2048, (16384, 1): 4096, (256, 64): 4096}
    for (reach, n_iter), tile in table.items():
        assert up.tmsst_tile_frames(reach, n_iter) == tile, (reach, n_iter)
        assert tile % 256 == 0 and tile + 2 * reach * n_iter <= 36864
    for reach, n_iter in ((0, 1), (-3, 1), (1, 0), (1, 65), (2048, 9), (16385, 1)):
        assert lib.ssq_tmsst_tile_frames(reach, n_iter) == -1
        with pytest.raises(ValueError):
            up.tmsst_tile_frames(reach, n_iter)


def test_c_entry_points_refuse_on_the_host():
    lib = _lib.load()
    for code in (_lib.SSQ_F32, _lib.SSQ_F64):
        base = lib.ssq_tssq_stft_workspace_bytes(code, 3, 1000, 64, 7)
        n_bins = 3 * 33 * ((1000 - 1) // 7 + 1)
        assert base > 0 and lib.ssq_tmssq_stft_workspace_bytes(code, 3, 1000, 64, 7, 4) == base + 2 * n_bins
        for n_fft in (8, 48, 8192):
            assert lib.ssq_tmssq_stft_workspace_bytes(code, 1, 1000, n_fft, 1, 4) == -1
            assert "n_fft" in lib.ssq_last_error().decode()
        assert lib.ssq_tmssq_stft_workspace_bytes(code, 0, 1000, 64, 1, 4) == -1
        assert lib.ssq_tmssq_stft_workspace_bytes(code, 1, 1000, 64, 0, 4) == -1
        for n_iter in (0, 65):
            assert lib.ssq_tmssq_stft_workspace_bytes(code, 1, 1000, 64, 1, n_iter) == -1
            assert "n_iter" in lib.ssq_last_error().decode()
        assert lib.ssq_tmssq_stft_workspace_bytes(code, 1, 1000, 4096, 1, 9) == -1
        assert "16384" in lib.ssq_last_error().decode()
    assert lib.ssq_tmssq_stft_workspace_bytes(7, 1, 1000, 64, 1, 4) == -1
    x = np.zeros(100)
    win = np.ones(4096)
    out = np.zeros((2049, 100), dtype=np.complex128)
    tail = (_vp(out), _vp(out), None, None)

    def host(n_fft=16, pad=0, order=2, n_iter=4, gamma=-1.0, xp=_vp(x)):
        return lib.ssq_tmssq_stft_host(_lib.SSQ_F64, xp, 1, 100, _vp(win), n_fft, 1, 1.0, pad, order, gamma, 3, n_iter, *tail)

    for kw, word in ((dict(n_fft=24), "n_fft"), (dict(pad=9), "padtype"), (dict(order=0), "order"), (dict(order=3), "order"),
                     (dict(n_iter=0), "n_iter"), (dict(n_iter=65), "n_iter"), (dict(n_fft=4096, n_iter=9), "16384"),
                     (dict(gamma=float("nan")), "gamma"), (dict(xp=None), "NULL")):
        assert host(**kw) != 0, kw
        assert word in lib.ssq_last_error().decode(), kw
        assert "tmssq_stft" in lib.ssq_last_error().decode() or word == "NULL"

    def execute(n_fft=16, order=2, n_iter=4, ws=out.nbytes):
        return lib.ssq_tmssq_stft_exec(_lib.SSQ_F64, _vp(x), 1, 100, _vp(win), n_fft, 1, 1.0, 0, order, -1.0, 3, n_iter,
                                       _vp(out), _vp(out), None, None, _vp(out), ws, None)

    # (a workspace that is too small is refused before any device work)
    for kw, word in ((dict(n_fft=24), "n_fft"), (dict(order=5), "order"), (dict(n_iter=-1), "n_iter"),
                     (dict(n_fft=4096, n_iter=9), "16384"), (dict(ws=16), "workspace")):
        assert execute(**kw) != 0, kw
        assert word in lib.ssq_last_error().decode(), kw

    m = np.tile(np.arange(5, dtype=np.int32), (2, 9, 1))
    o = np.empty_like(m)
    for args, word in (((None, 2, 9, 5, 2, 1, _vp(o)), "NULL"), ((_vp(m), 2, 9, 5, 2, 1, None), "NULL"),
                       ((_vp(m), 0, 9, 5, 2, 1, _vp(o)), "batch"), ((_vp(m), 2, 0, 5, 2, 1, _vp(o)), "n_rows"),
                       ((_vp(m), 2, 9, 0, 2, 1, _vp(o)), "n_frames"), ((_vp(m), 2, 9, 5, 0, 1, _vp(o)), "n_iter"),
                       ((_vp(m), 2, 9, 5, 65, 1, _vp(o)), "n_iter"), ((_vp(m), 2, 9, 5, 2, 0, _vp(o)), "reach"),
                       ((_vp(m), 2, 9, 5, 9, 2048, _vp(o)), "16384")):
        assert lib.ssq_tmsst_walk_host(*args) != 0, word
        assert word in lib.ssq_last_error().decode(), word
    for v, word in ((-2, "outside"), (5, "outside"), (0, "farther")):
        m[1, 8, 4] = v
        assert lib.ssq_tmsst_walk_host(_vp(m), 2, 9, 5, 2, 3, _vp(o)) != 0
        assert word in lib.ssq_last_error().decode()


def test_host_slice_cap_is_exported_bound_and_refuses_a_negative_cap():
    """`ssq_host_slice_cap` (include/ssq_hip.h: an aid for testing the host slices; tests/test_gpu_host_slices.py uses it)."""
    lib = _lib.load()
    assert "ssq_host_slice_cap" in _lib.header_symbols()
    assert _lib._SIGNATURES["ssq_host_slice_cap"] == (C.c_int, [i64])
    try:
        assert lib.ssq_host_slice_cap(-1) != 0
        assert lib.ssq_last_error().decode() == "ssq_host_slice_cap: signals must be >= 0 (0: no cap)"
        assert lib.ssq_host_slice_cap(3) == 0
    finally:
        assert lib.ssq_host_slice_cap(0) == 0
