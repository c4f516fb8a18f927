"""CPU tests of `upstream.tssq_cwt`'s surface: the signature, every refusal before the GPU is asked for, the
fixed-point quantum, the rows' frequencies, and the C entry points exported, declared, bound and refusing bad arguments
on the host."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up

E = inspect.Parameter.empty
NEW = ("ssq_tssq_cwt_host", "ssq_tssq_cwt_workspace_bytes", "ssq_tssq_cwt_exec")
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


def test_signature():
    sig = [(p.name, p.default) for p in inspect.signature(up.tssq_cwt).parameters.values()]
    assert sig == [("x", E), ("wavelet", "gmw"), ("scales", "log-piecewise"), ("nv", None), ("fs", None), ("t", None),
                   ("padtype", "reflect"), ("order", 2), ("gamma", None), ("get_tau", False), ("get_targets", False),
                   ("work_limit_bytes", None)]


def test_docstrings_name_the_feature():
    assert "tssq_cwt" in up.__doc__ and "4.16" in up.__doc__
    doc = up.tssq_cwt.__doc__
    assert "Re(Wt / W)" in doc and "no inverse" in doc and "marginal identity" in doc


def test_quantum_log2():
    assert up.TSSQ_CWT_QUANTUM_LOG2_MAX == 38 and up.TSSQ_CWT_MAX_CELLS == 1 << 40 and up.TSSQ_CWT_MAX_N == 1 << 26
    assert up.tssq_cwt_quantum_log2(2) == -38                            # L = 1
    assert up.tssq_cwt_quantum_log2(1 << 23) == -38                      # L = 23, the last length with the full 38 bits
    assert up.tssq_cwt_quantum_log2((1 << 23) + 1) == -37
    assert up.tssq_cwt_quantum_log2(1 << 24) == -37                      # L = 24: 61 - 24
    assert up.tssq_cwt_quantum_log2(1 << 30) == -31                      # L = 30: 61 - 30
    with pytest.raises(ValueError):
        up.tssq_cwt_quantum_log2(0)


def test_row_freqs_are_the_closed_forms():
    nu = up.tssq_cwt_row_freqs(("gmw", {"gamma": 3.0, "beta": 60.0}), SC)
    assert nu.dtype == np.float64 and nu.shape == SC.shape
    assert np.allclose(nu, 20.0 ** (1 / 3) / (2 * np.pi * SC), rtol=4e-16, atol=0)
    assert np.allclose(up.tssq_cwt_row_freqs("gmw", SC), nu, rtol=0, atol=0)
    nu = up.tssq_cwt_row_freqs(("gmw", {"gamma": 2.0, "beta": 8.0}), SC.astype(np.float32))
    assert nu.dtype == np.float64 and np.allclose(nu, 2.0 / (2 * np.pi * SC.astype(np.float32).astype(np.float64)), rtol=4e-16, atol=0)
    nu = up.tssq_cwt_row_freqs(("morlet", {"mu": 13.4}), SC)
    assert np.allclose(nu, 13.4 / (2 * np.pi * SC), rtol=4e-16, atol=0)
    assert np.allclose(up.tssq_cwt_row_freqs("morlet", SC), nu, rtol=0, atol=0)
    from tests.helpers import tssq_cwt_ref as m
    assert np.array_equal(m.row_freqs(("gmw", 3.0, 60.0), SC), up.tssq_cwt_row_freqs("gmw", SC))
    assert np.array_equal(m.row_freqs(("morlet", 13.4), SC), up.tssq_cwt_row_freqs("morlet", SC))
    with pytest.raises(ValueError, match="scales"):
        up.tssq_cwt_row_freqs("gmw", -SC)
    with pytest.raises(ValueError, match="wavelet"):
        up.tssq_cwt_row_freqs("bump", SC)


def test_entry_points_are_exported_declared_and_bound():
    lib = _lib.load()
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib._SIGNATURES and name in _lib.header_symbols()
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, header)
    assert set(_lib._SIGNATURES) <= set(_lib.header_symbols())            # the header declares what `_lib` binds


def test_refusals_come_before_the_gpu(no_gpu):
    x = np.random.default_rng(1).standard_normal(300)
    with pytest.raises(ValueError, match="scales"):
        up.tssq_cwt(x)                                           # the string default, as ssq_cwt2
    with pytest.raises(ValueError, match="scales"):
        up.tssq_cwt(x, scales="log")
    with pytest.raises(ValueError, match="scales"):
        up.tssq_cwt(x, scales=np.array([4.0]))
    with pytest.raises(ValueError, match="scales"):
        up.tssq_cwt(x, scales=-SC)
    with pytest.raises(ValueError, match="scales"):
        up.tssq_cwt(x, scales=np.concatenate([[0.0], SC]))
    with pytest.raises(ValueError, match="scales"):
        up.tssq_cwt(x, scales=np.concatenate([SC, [np.inf]]))
    with pytest.raises(ValueError, match="padtype"):
        up.tssq_cwt(x, scales=SC, padtype="constant")
    for order in (0, 3, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="order"):
            up.tssq_cwt(x, scales=SC, order=order)
    with pytest.raises(ValueError, match="order"):
        up.tssq_cwt(x, ("gmw", {"order": 1}), scales=SC)
    with pytest.raises(ValueError, match="wavelet"):
        up.tssq_cwt(x, "bump", scales=SC)
    with pytest.raises(ValueError, match="wavelet"):
        up.tssq_cwt(x, ("gmw", {"beta": -1.0}), scales=SC)
    with pytest.raises(ValueError, match="wavelet"):
        up.tssq_cwt(x, ("gmw", {"gamma": float("inf")}), scales=SC)
    with pytest.raises(ValueError, match="wavelet"):
        up.tssq_cwt(x, ("morlet", {"mu": 0.0}), scales=SC)
    with pytest.raises(ValueError, match="gamma"):
        up.tssq_cwt(x, scales=SC, gamma=float("nan"))
    with pytest.raises(ValueError, match="sampling period"):
        up.tssq_cwt(x, scales=SC, fs=-1.0)
    with pytest.raises(ValueError, match="sampling period"):
        up.tssq_cwt(x, scales=SC, fs=float("nan"))
    with pytest.raises(ValueError, match="`t`"):
        up.tssq_cwt(x, scales=SC, t=np.arange(10))
    with pytest.raises(ValueError, match="nv"):
        up.tssq_cwt(x, scales=SC, nv=8)
    with pytest.raises(ValueError, match="work_limit_bytes"):
        up.tssq_cwt(x, scales=SC, work_limit_bytes=1024)
    with pytest.raises(TypeError):
        up.tssq_cwt(list(x), scales=SC)
    with pytest.raises(ValueError, match="samples"):
        up.tssq_cwt(np.zeros(1), scales=SC)
    for gone in ("ssq_freqs", "maprange", "squeezing", "flipud"):
        with pytest.raises(TypeError):
            up.tssq_cwt(x, scales=SC, **{gone: None})


def test_too_many_cells_is_refused_by_the_c_checks(no_gpu):
    """na N > 2^40: 32767 scales on 2^26 samples (a calloc'ed signal: no page of it is touched before the refusal)."""
    x = np.zeros(1 << 26, dtype=np.float32)
    sc = 2.0 * 2.0 ** (np.arange(32767) / 4096)
    with pytest.raises(ValueError, match="2\\^40"):
        up.tssq_cwt(x, scales=sc)
    lib = _lib.load()
    for order in (1, 2):
        assert lib.ssq_tssq_cwt_workspace_bytes(_lib.SSQ_F32, 1, 1 << 26, 32767, order, None) == -1
        assert "2^40" in lib.ssq_last_error().decode()
        assert lib.ssq_tssq_cwt_workspace_bytes(_lib.SSQ_F32, 1, 1 << 26, 16384, order, None) > 0     # exactly 2^40


@pytest.mark.parametrize("kw", [dict(), dict(wavelet=("morlet", {"mu": 6.0}), padtype="wrap", order=1, get_tau=True,
                                             get_targets=True, fs=2.0, gamma=1e-6),
                                dict(wavelet=("gmw", {"gamma": 3, "beta": 20}), nv=4, padtype="symmetric")])
@pytest.mark.parametrize("shape,dtype", [((300,), np.float64), ((2, 300), np.float32)])
def test_well_formed_calls_reach_the_gpu(no_gpu, kw, shape, dtype):
    x = np.random.default_rng(2).standard_normal(shape).astype(dtype)
    for sc in (SC, np.linspace(2, 60, 50)):
        if kw.get("nv") and len(sc) != 20:
            continue
        with pytest.raises(_Reached):
            up.tssq_cwt(x, scales=sc, **kw)


def test_log_piecewise_scales_and_a_work_limit_reach_the_gpu(no_gpu):
    morlet = ("morlet", {"mu": 13.4})
    sc = np.ascontiguousarray(up.process_scales("log-piecewise", 777, morlet, nv=8), dtype=np.float64).reshape(-1)
    mn = C.c_int64(0)
    assert _lib.load().ssq_tssq_cwt_workspace_bytes(_lib.SSQ_F64, 1, 777, len(sc), 2, C.byref(mn)) > 0
    with pytest.raises(_Reached):
        up.tssq_cwt(np.zeros(777), morlet, scales=sc, padtype="replicate", get_targets=True, work_limit_bytes=mn.value)


def test_workspace_bytes():
    lib = _lib.load()
    mn = C.c_int64(0)
    for code in (_lib.SSQ_F32, _lib.SSQ_F64):
        for order, M in ((1, 2), (2, 5)):
            # N = 300 -> P = 512; the maxima (to 16 bytes), 20 bytes a cell (to 16 bytes), then 16 P (batch + 2 M R)
            fixed = 32 + 20 * 3 * 37 * 300
            assert fixed % 16 == 0
            assert lib.ssq_tssq_cwt_workspace_bytes(code, 3, 300, 37, order, C.byref(mn)) == fixed + 16 * 512 * (3 + 2 * M * 3 * 37)
            assert mn.value == fixed + 16 * 512 * (3 + 2 * M)
            # 37 x 301 cells: the int32 map is rounded up to 16 bytes
            assert lib.ssq_tssq_cwt_workspace_bytes(code, 1, 301, 37, order, C.byref(mn)) > 0
            assert mn.value == 16 + 16 * 37 * 301 + (4 * 37 * 301 + 15) // 16 * 16 + 16 * 512 * (1 + 2 * M)
            # the chunk area capped at 2 GiB: batch 4 x 2^16 samples (P = 2^17) x 128 scales
            big = lib.ssq_tssq_cwt_workspace_bytes(code, 4, 1 << 16, 128, order, C.byref(mn))
            fixed = 32 + 20 * 4 * 128 * (1 << 16)
            assert mn.value < big <= fixed + (2 << 30) and (big - fixed - 16 * (1 << 17) * 4) % ((32 * M) << 17) == 0
            for bad in ((0, 300, 37), (1, 1, 37), (1, 300, 1), (1, 300, 40000), (1, (1 << 26) + 1, 4)):
                assert lib.ssq_tssq_cwt_workspace_bytes(code, *bad, order, None) == -1
                assert lib.ssq_last_error()
        for order in (0, 3, -1):
            assert lib.ssq_tssq_cwt_workspace_bytes(code, 1, 300, 37, order, None) == -1
            assert "order" in lib.ssq_last_error().decode()
    assert lib.ssq_tssq_cwt_workspace_bytes(7, 1, 300, 37, 2, None) == -1


def test_c_entry_points_refuse_on_the_host():
    lib = _lib.load()
    N, na = 100, 20
    x = np.zeros(N)
    nu = up.tssq_cwt_row_freqs("gmw", SC)
    bad_nu = nu.copy()
    bad_nu[3] = float("nan")
    out = np.zeros((na, N), dtype=np.complex128)
    mn = C.c_int64(0)
    assert lib.ssq_tssq_cwt_workspace_bytes(_lib.SSQ_F64, 1, N, na, 2, C.byref(mn)) > 0

    def host(**kw):
        a = dict(dtype=_lib.SSQ_F64, x=_vp(x), batch=1, N=N, wavelet=0, p0=3.0, p1=60.0, scales=_vp(SC), nu=_vp(nu), na=na,
                 dt=1.0, pad=0, order=2, gamma=-1.0, limit=0, Tx=_vp(out), Wx=_vp(out), tau=None, mm=None)
        a.update(kw)
        return lib.ssq_tssq_cwt_host(*a.values())

    def exec_(**kw):
        a = dict(dtype=_lib.SSQ_F64, x=_vp(x), batch=1, N=N, wavelet=0, p0=3.0, p1=60.0, scales=_vp(SC), nu=_vp(nu), na=na,
                 dt=1.0, pad=0, order=2, gamma=-1.0, Tx=_vp(out), Wx=_vp(out), tau=None, mm=None, work=_vp(out),
                 work_bytes=1 << 30, stream=None, ms=None)
        a.update(kw)
        return lib.ssq_tssq_cwt_exec(*a.values())

    for call in (host, exec_):
        for kw, word in ((dict(wavelet=2), "wavelet"), (dict(wavelet=-1), "wavelet"), (dict(p0=0.0), "p0"),
                         (dict(p0=-3.0), "p0"), (dict(p0=float("inf")), "p0"), (dict(p1=0.0), "p1"),
                         (dict(p1=float("nan")), "p1"), (dict(wavelet=1, p0=0.0), "p0"), (dict(na=1), "na"),
                         (dict(batch=0), "batch"), (dict(N=1), "n_signal"), (dict(dtype=5), "dtype"),
                         (dict(x=None), "NULL"), (dict(scales=None), "NULL"), (dict(nu=None), "NULL"),
                         (dict(Tx=None), "NULL"), (dict(Wx=None), "NULL"), (dict(dt=0.0), "dt"),
                         (dict(dt=float("inf")), "dt"), (dict(dt=float("nan")), "dt"), (dict(order=0), "order"),
                         (dict(order=3), "order"), (dict(pad=5), "padtype"), (dict(pad=-1), "padtype"),
                         (dict(gamma=float("nan")), "gamma"), (dict(scales=_vp(-SC)), "scales"),
                         (dict(nu=_vp(-nu)), "row_freqs"), (dict(nu=_vp(bad_nu)), "row_freqs"),
                         (dict(N=1 << 26, na=32767), "2^40")):
            assert call(**kw) != 0, kw
            assert word in lib.ssq_last_error().decode(), (kw, lib.ssq_last_error())
    assert host(limit=16) != 0 and "work_limit_bytes" in lib.ssq_last_error().decode()
    assert host(limit=mn.value - 1) != 0 and "work_limit_bytes" in lib.ssq_last_error().decode()
    assert host(limit=-1) != 0
    assert exec_(work_bytes=mn.value - 1) != 0 and "workspace" in lib.ssq_last_error().decode()
    assert exec_(work=None) != 0 and "NULL" in lib.ssq_last_error().decode()
