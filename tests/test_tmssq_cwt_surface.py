"""CPU tests of the surface of `upstream.tmssq_cwt`, `upstream.tmssq_cwt_walk` and `upstream.tmssq_cwt_tile_cols` (DESIGN
4.22): the signatures, every refusal before the GPU is asked for, the workspace, and the C entry points exported,
declared, bound and refusing bad arguments on the host."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up

E = inspect.Parameter.empty
i64, vp, dbl = C.c_int64, C.c_void_p, C.c_double
NEW = {
    "ssq_tmssq_cwt_host": (C.c_int, [C.c_int, vp, i64, i64, C.c_int, dbl, dbl, vp, vp, i64, dbl, C.c_int, C.c_int, dbl,
                                     C.c_int, i64, vp, vp, vp, vp]),
    "ssq_tmssq_cwt_workspace_bytes": (i64, [C.c_int, i64, i64, i64, C.c_int, C.POINTER(i64)]),
    "ssq_tmssq_cwt_exec": (C.c_int, [C.c_int, vp, i64, i64, C.c_int, dbl, dbl, vp, vp, i64, dbl, C.c_int, C.c_int, dbl,
                                     C.c_int, vp, vp, vp, vp, vp, i64, vp, C.POINTER(C.c_float)]),
    "ssq_tmssq_cwt_walk_host": (C.c_int, [vp, i64, i64, i64, C.c_int, vp]),
    "ssq_tmssq_cwt_tile_cols": (C.c_int, [C.POINTER(C.c_int)]),
}
SC = 2.0 * 2.0 ** (np.arange(20) / 4)


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
    sig = [(p.name, p.default) for p in inspect.signature(up.tmssq_cwt).parameters.values()]
    assert sig == [("x", E), ("wavelet", "gmw"), ("scales", "log-piecewise"), ("nv", None), ("fs", None), ("t", None),
                   ("padtype", "reflect"), ("order", 2), ("n_iter", 4), ("gamma", None), ("get_tau", False),
                   ("get_targets", False), ("work_limit_bytes", None)]
    assert [(p.name, p.default) for p in inspect.signature(up.tmssq_cwt_walk).parameters.values()] == \
        [("targets", E), ("n_iter", E)]
    assert not inspect.signature(up.tmssq_cwt_tile_cols).parameters


def test_docstrings_name_the_feature():
    assert "tmssq_cwt" in up.__doc__ and "tmssq_cwt_walk" in up.__doc__ and "4.22" in up.__doc__
    doc = up.tmssq_cwt.__doc__
    for word in ("n_iter", "fixed point", "spill", "There is no inverse", "bit for bit", "LDS"):
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
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)

    def names(fn):
        params = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % fn, src).group(1).split(",")
        return [re.split(r"[\s*]+", p.strip())[-1] for p in params]

    one = names("ssq_tssq_cwt_host")
    assert names("ssq_tmssq_cwt_host") == one[:14] + ["n_iter"] + one[14:]          # ssq_tssq_cwt_host's plus n_iter
    one = names("ssq_tssq_cwt_exec")
    assert names("ssq_tmssq_cwt_exec") == one[:14] + ["n_iter"] + one[14:]
    assert names("ssq_tmssq_cwt_workspace_bytes") == names("ssq_tssq_cwt_workspace_bytes")
    assert names("ssq_tmssq_cwt_walk_host") == ["targets_in", "batch", "n_rows", "n_cols", "n_iter", "targets_out"]
    assert names("ssq_tmssq_cwt_tile_cols") == ["halo"]


@pytest.mark.parametrize("n_iter", [0, -1, 65, 1000, 2.0, 2.5, True, False, "4", None])
def test_n_iter_refusals_come_before_the_gpu(no_gpu, n_iter):
    with pytest.raises(ValueError, match="n_iter"):
        up.tmssq_cwt(np.zeros(300), scales=SC, n_iter=n_iter)
    with pytest.raises(ValueError, match="n_iter"):
        up.tmssq_cwt_walk(np.zeros((9, 4), dtype=np.int32), n_iter)


def test_other_refusals_come_before_the_gpu(no_gpu):
    x = np.random.default_rng(1).standard_normal(300)
    for order in (0, 3, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="order"):
            up.tmssq_cwt(x, scales=SC, order=order)
    with pytest.raises(ValueError, match="wavelet"):
        up.tmssq_cwt(x, "bump", scales=SC)
    with pytest.raises(ValueError, match="wavelet"):
        up.tmssq_cwt(x, ("gmw", {"beta": -1.0}), scales=SC)
    with pytest.raises(ValueError, match="order"):
        up.tmssq_cwt(x, ("gmw", {"order": 1}), scales=SC)
    with pytest.raises(ValueError, match="scales"):
        up.tmssq_cwt(x)
    with pytest.raises(ValueError, match="scales"):
        up.tmssq_cwt(x, scales=-SC)
    with pytest.raises(ValueError, match="padtype"):
        up.tmssq_cwt(x, scales=SC, padtype="constant")
    with pytest.raises(ValueError, match="gamma"):
        up.tmssq_cwt(x, scales=SC, gamma=float("nan"))
    with pytest.raises(ValueError, match="nv"):
        up.tmssq_cwt(x, scales=SC, nv=8)
    mn = C.c_int64(0)
    assert _lib.load().ssq_tmssq_cwt_workspace_bytes(_lib.SSQ_F64, 1, 300, len(SC), 2, C.byref(mn)) > 0
    for limit in (1024, mn.value - 1):
        with pytest.raises(ValueError, match="work_limit_bytes"):
            up.tmssq_cwt(x, scales=SC, work_limit_bytes=limit)
    with pytest.raises(_Reached):
        up.tmssq_cwt(x, scales=SC, work_limit_bytes=mn.value)
    with pytest.raises(TypeError):
        up.tmssq_cwt(list(x), scales=SC)
    for gone in ("ssq_freqs", "maprange", "squeezing", "flipud"):
        with pytest.raises(TypeError):
            up.tmssq_cwt(x, scales=SC, **{gone: None})


def test_walk_refusals_come_before_the_gpu(no_gpu):
    good = np.tile(np.arange(4, dtype=np.int32), (9, 1))
    for bad in (good.astype(np.int64), good.astype(np.float32), good.astype(np.float64), good.astype(np.int16), good.tolist(),
                good[0], np.zeros((2, 2, 9, 4), dtype=np.int32), np.zeros((9, 0), dtype=np.int32),
                np.zeros((0, 4), dtype=np.int32), np.zeros((0, 9, 4), dtype=np.int32)):
        with pytest.raises(ValueError, match="targets"):
            up.tmssq_cwt_walk(bad, 2)
    for v in (-2, 4, 2 ** 20):                                  # a target of n, of -2, far outside
        bad = good.copy()
        bad[3, 1] = v
        with pytest.raises(ValueError, match="outside"):
            up.tmssq_cwt_walk(bad, 2)
    far = good.copy()
    far[0, 0], far[1, 1], far[3, 0] = -1, 3, 3                 # any column of the row is a target
    for m, n_iter in ((far, 64), (np.stack([far, far]), 8), (np.asfortranarray(far), 1), (far, np.int64(2))):
        with pytest.raises(_Reached):
            up.tmssq_cwt_walk(m, n_iter)


@pytest.mark.parametrize("kw", [dict(), dict(wavelet=("morlet", {"mu": 6.0}), padtype="wrap", order=1, get_tau=True,
                                             get_targets=True, fs=2.0, gamma=1e-6, n_iter=64),
                                dict(n_iter=1, get_targets=True)])
@pytest.mark.parametrize("shape,dtype", [((300,), np.float64), ((2, 300), np.float32)])
def test_well_formed_calls_reach_the_gpu(no_gpu, kw, shape, dtype):
    x = np.random.default_rng(2).standard_normal(shape).astype(dtype)
    for sc in (SC, np.linspace(2, 60, 50)):
        with pytest.raises(_Reached):
            up.tmssq_cwt(x, scales=sc, **kw)


def test_tile_cols():
    T, halo = up.tmssq_cwt_tile_cols()
    assert isinstance(T, int) and isinstance(halo, int) and T > 0 and halo >= 0
    assert T % 256 == 0                                         # whole passes of the workgroup
    assert 4 * (T + 2 * halo) <= 160 * 1024 // 2                # the int32 stage leaves two workgroups a CU at the least
    assert _lib.load().ssq_tmssq_cwt_tile_cols(None) == T


def test_workspace_is_tssq_cwts_plus_one_plane():
    """`tssq_cwt`'s head has 20 bytes a cell, this one 24 (the walked int32 plane), each rounded up to 16 bytes after the
    maxima; the chunk area is the same."""
    lib = _lib.load()
    mn, mn1 = C.c_int64(0), C.c_int64(0)
    for code in (_lib.SSQ_F32, _lib.SSQ_F64):
        for order in (1, 2):
            for B, N, na in ((3, 300, 37), (1, 301, 37), (2, 1000, 50), (4, 1 << 16, 128)):
                cells = B * na * N
                one = lib.ssq_tssq_cwt_workspace_bytes(code, B, N, na, order, C.byref(mn1))
                got = lib.ssq_tmssq_cwt_workspace_bytes(code, B, N, na, order, C.byref(mn))
                grow = (24 * cells + 15) // 16 * 16 - (20 * cells + 15) // 16 * 16
                assert one > 0 and got == one + grow and mn.value == mn1.value + grow
                assert abs(grow - 4 * cells) < 16 and (grow == 4 * cells or cells % 4)
            for bad in ((0, 300, 37), (1, 1, 37), (1, 300, 1), (1, 300, 40000), (1, (1 << 26) + 1, 4)):
                assert lib.ssq_tmssq_cwt_workspace_bytes(code, *bad, order, None) == -1
                assert "tmssq_cwt" in lib.ssq_last_error().decode() or bad[0] == 0
        for order in (0, 3, -1):
            assert lib.ssq_tmssq_cwt_workspace_bytes(code, 1, 300, 37, order, None) == -1
            assert "order" in lib.ssq_last_error().decode()
    assert lib.ssq_tmssq_cwt_workspace_bytes(7, 1, 300, 37, 2, None) == -1
    assert lib.ssq_tmssq_cwt_workspace_bytes(_lib.SSQ_F32, 1, 1 << 26, 32767, 2, None) == -1
    assert "2^40" in lib.ssq_last_error().decode()


def test_c_entry_points_refuse_on_the_host():
    lib = _lib.load()
    N, na = 100, 20
    x = np.zeros(N)
    nu = up.tssq_cwt_row_freqs("gmw", SC)
    out = np.zeros((na, N), dtype=np.complex128)
    mn = C.c_int64(0)
    assert lib.ssq_tmssq_cwt_workspace_bytes(_lib.SSQ_F64, 1, N, na, 2, C.byref(mn)) > 0

    def host(**kw):
        a = dict(dtype=_lib.SSQ_F64, x=_vp(x), batch=1, N=N, wavelet=0, p0=3.0, p1=60.0, scales=_vp(SC), nu=_vp(nu), na=na,
                 dt=1.0, pad=0, order=2, gamma=-1.0, n_iter=4, limit=0, Tx=_vp(out), Wx=_vp(out), tau=None, mm=None)
        a.update(kw)
        return lib.ssq_tmssq_cwt_host(*a.values())

    def exec_(**kw):
        a = dict(dtype=_lib.SSQ_F64, x=_vp(x), batch=1, N=N, wavelet=0, p0=3.0, p1=60.0, scales=_vp(SC), nu=_vp(nu), na=na,
                 dt=1.0, pad=0, order=2, gamma=-1.0, n_iter=4, Tx=_vp(out), Wx=_vp(out), tau=None, mm=None, work=_vp(out),
                 work_bytes=1 << 30, stream=None, ms=None)
        a.update(kw)
        return lib.ssq_tmssq_cwt_exec(*a.values())

    for call in (host, exec_):
        for kw, word in ((dict(wavelet=2), "wavelet"), (dict(p0=0.0), "p0"), (dict(na=1), "na"), (dict(batch=0), "batch"),
                         (dict(N=1), "n_signal"), (dict(dtype=5), "dtype"), (dict(x=None), "NULL"), (dict(scales=None), "NULL"),
                         (dict(nu=None), "NULL"), (dict(Tx=None), "NULL"), (dict(dt=0.0), "dt"), (dict(order=0), "order"),
                         (dict(order=3), "order"), (dict(n_iter=0), "n_iter"), (dict(n_iter=65), "n_iter"),
                         (dict(n_iter=-4), "n_iter"), (dict(pad=5), "padtype"), (dict(gamma=float("nan")), "gamma"),
                         (dict(scales=_vp(-SC)), "scales"), (dict(nu=_vp(-nu)), "row_freqs"),
                         (dict(N=1 << 26, na=32767), "2^40")):
            assert call(**kw) != 0, kw
            msg = lib.ssq_last_error().decode()
            assert word in msg, (kw, msg)
            assert "tmssq_cwt" in msg or word in ("NULL", "dtype", "batch"), msg
    assert host(limit=16) != 0 and "work_limit_bytes" in lib.ssq_last_error().decode()
    assert host(limit=mn.value - 1) != 0 and "ssq_tmssq_cwt_workspace_bytes" in lib.ssq_last_error().decode()
    assert exec_(work_bytes=mn.value - 1) != 0 and "workspace" in lib.ssq_last_error().decode()
    assert exec_(work=None) != 0 and "NULL" in lib.ssq_last_error().decode()

    m = np.tile(np.arange(5, dtype=np.int32), (2, 9, 1))
    o = np.empty_like(m)
    for args, word in (((None, 2, 9, 5, 2, _vp(o)), "NULL"), ((_vp(m), 2, 9, 5, 2, None), "NULL"),
                       ((_vp(m), 0, 9, 5, 2, _vp(o)), "batch"), ((_vp(m), 2, 0, 5, 2, _vp(o)), "n_rows"),
                       ((_vp(m), 2, 9, 0, 2, _vp(o)), "n_cols"), ((_vp(m), 2, 9, (1 << 30) + 1, 2, _vp(o)), "n_cols"),
                       ((_vp(m), 2, 9, 5, 0, _vp(o)), "n_iter"), ((_vp(m), 2, 9, 5, 65, _vp(o)), "n_iter")):
        assert lib.ssq_tmssq_cwt_walk_host(*args) != 0, word
        assert word in lib.ssq_last_error().decode(), word
    for v in (-2, 5, 2 ** 30):
        m[1, 8, 4] = v
        assert lib.ssq_tmssq_cwt_walk_host(_vp(m), 2, 9, 5, 2, _vp(o)) != 0
        assert "outside" in lib.ssq_last_error().decode()
