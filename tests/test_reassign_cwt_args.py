"""CPU tests of `upstream.reassign_cwt`'s surface: the signature, every refusal before the GPU is asked for, the
fixed-point quantum, and the C entry points exported, declared, bound and refusing bad arguments on the host."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.helpers import cwt_sst2_ref as m

E = inspect.Parameter.empty
NEW = ("ssq_reassign_cwt_host", "ssq_reassign_cwt_workspace_bytes", "ssq_reassign_cwt_exec")
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
    sig = [(p.name, p.default) for p in inspect.signature(up.reassign_cwt).parameters.values()]
    assert sig == [("x", E), ("wavelet", "gmw"), ("scales", "log-piecewise"), ("nv", None), ("fs", None), ("t", None),
                   ("ssq_freqs", None), ("padtype", "reflect"), ("maprange", "peak"), ("gamma", None), ("flipud", True),
                   ("get_w", False), ("get_tau", False), ("get_targets", False)]


def test_docstrings_name_the_feature():
    assert "reassign_cwt" in up.__doc__ and "4.15" in up.__doc__
    doc = up.reassign_cwt.__doc__
    assert "First order only" in doc and "Re(Wt / W)" in doc and "no inverse" in doc


def test_quantum_log2():
    assert up.REASSIGN_CWT_QUANTUM_LOG2_MAX == 38
    assert up.reassign_cwt_quantum_log2(2, 2) == -38                     # L = 2
    assert up.reassign_cwt_quantum_log2(180, 512) == -38                 # L = 17
    assert up.reassign_cwt_quantum_log2(256, 1 << 20) == -34             # L = 28: 62 - 28
    assert up.reassign_cwt_quantum_log2(32767, 1 << 25) == -22           # L = 40: 62 - 40
    assert up.reassign_cwt_quantum_log2(1 << 12, 1 << 12) == -38         # L = 24, the last shape with the full 38 bits
    assert up.reassign_cwt_quantum_log2((1 << 12) + 1, 1 << 12) == -37
    with pytest.raises(ValueError):
        up.reassign_cwt_quantum_log2(0, 5)


def test_entry_points_are_exported_declared_and_bound():
    lib = _lib.load()
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib._SIGNATURES and name in _lib.header_symbols()
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, header)


def test_refusals_come_before_the_gpu(no_gpu):
    x = np.random.default_rng(1).standard_normal(300)
    with pytest.raises(ValueError, match="scales"):
        up.reassign_cwt(x)                                       # the string default, as ssq_cwt2
    with pytest.raises(ValueError, match="scales"):
        up.reassign_cwt(x, scales="log")
    with pytest.raises(ValueError, match="scales"):
        up.reassign_cwt(x, scales=np.array([4.0]))
    with pytest.raises(ValueError, match="scales"):
        up.reassign_cwt(x, scales=-SC)
    with pytest.raises(ValueError, match="scales"):
        up.reassign_cwt(x, scales=np.concatenate([[0.0], SC]))
    with pytest.raises(ValueError, match="padtype"):
        up.reassign_cwt(x, scales=SC, padtype="constant")
    with pytest.raises(ValueError, match="maprange"):
        up.reassign_cwt(x, scales=SC, maprange="energy")
    with pytest.raises(ValueError, match="maprange"):
        up.reassign_cwt(x, scales=SC, ssq_freqs="log-piecewise", maprange="maximal")
    with pytest.raises(ValueError, match="ssq_freqs"):
        up.reassign_cwt(x, scales=SC, ssq_freqs=np.linspace(0.01, 0.5, 7))
    with pytest.raises(ValueError, match="order"):
        up.reassign_cwt(x, ("gmw", {"order": 1}), scales=SC)
    with pytest.raises(ValueError, match="wavelet"):
        up.reassign_cwt(x, "bump", scales=SC)
    with pytest.raises(ValueError, match="wavelet"):
        up.reassign_cwt(x, ("gmw", {"beta": -1.0}), scales=SC)
    with pytest.raises(ValueError, match="gamma"):
        up.reassign_cwt(x, scales=SC, gamma=float("nan"))
    with pytest.raises(ValueError, match="`t`"):
        up.reassign_cwt(x, scales=SC, t=np.arange(10))
    with pytest.raises(TypeError):
        up.reassign_cwt(list(x), scales=SC)
    with pytest.raises(ValueError, match="samples"):
        up.reassign_cwt(np.zeros(1), scales=SC)
    with pytest.raises(TypeError):
        up.reassign_cwt(x, scales=SC, squeezing="sum")           # no row weights, no squeezing


def test_too_many_cells_is_refused_by_the_c_checks(no_gpu):
    """na N > 2^40: 32767 scales on 2^26 samples (a calloc'ed signal: no page of it is touched before the refusal)."""
    x = np.zeros(1 << 26, dtype=np.float32)
    sc = 2.0 * 2.0 ** (np.arange(32767) / 4096)
    with pytest.raises(ValueError, match="2\\^40"):
        up.reassign_cwt(x, scales=sc, maprange="maximal")
    lib = _lib.load()
    assert lib.ssq_reassign_cwt_workspace_bytes(_lib.SSQ_F32, 1, 1 << 26, 32767, None) == -1
    assert "2^40" in lib.ssq_last_error().decode()
    assert lib.ssq_reassign_cwt_workspace_bytes(_lib.SSQ_F32, 1, 1 << 26, 16384, None) > 0      # exactly 2^40


@pytest.mark.parametrize("kw", [dict(), dict(wavelet=("morlet", {"mu": 6.0}), padtype="wrap", flipud=False, get_w=True,
                                             get_tau=True, get_targets=True, fs=2.0, gamma=1e-6, maprange="maximal",
                                             ssq_freqs="linear"),
                                dict(wavelet=("gmw", {"gamma": 3, "beta": 20}), nv=4, padtype="symmetric",
                                     ssq_freqs=np.linspace(0.01, 0.5, 20))])
@pytest.mark.parametrize("shape,dtype", [((300,), np.float64), ((2, 300), np.float32)])
def test_well_formed_calls_reach_the_gpu(no_gpu, kw, shape, dtype):
    x = np.random.default_rng(2).standard_normal(shape).astype(dtype)
    for sc in (SC, np.linspace(2, 60, 50)):
        if (kw.get("nv") or isinstance(kw.get("ssq_freqs"), np.ndarray)) and len(sc) != 20:
            continue
        with pytest.raises(_Reached):
            up.reassign_cwt(x, scales=sc, **kw)


def test_log_piecewise_scales_reach_the_gpu(no_gpu):
    morlet = ("morlet", {"mu": 13.4})
    sc = np.ascontiguousarray(up.process_scales("log-piecewise", 777, morlet, nv=8), dtype=np.float64).reshape(-1)
    with pytest.raises(_Reached):
        up.reassign_cwt(np.zeros(777), morlet, scales=sc, padtype="replicate", get_targets=True)


def test_workspace_bytes():
    lib = _lib.load()
    mn = C.c_int64(0)
    for code in (_lib.SSQ_F32, _lib.SSQ_F64):
        # N = 300 -> P = 512; the maxima (to 16 bytes), 16 bytes a cell, then 16 P (batch + 6 R)
        fixed = 32 + 16 * 3 * 37 * 300
        assert lib.ssq_reassign_cwt_workspace_bytes(code, 3, 300, 37, C.byref(mn)) == fixed + 16 * 512 * (3 + 6 * 3 * 37)
        assert mn.value == fixed + 16 * 512 * (3 + 6)
        assert lib.ssq_reassign_cwt_workspace_bytes(code, 1, 300, 37, None) == 16 + 16 * 37 * 300 + 16 * 512 * (1 + 6 * 37)
        # the chunk area capped at 2 GiB: batch 4 x 2^16 samples (P = 2^17) x 128 scales
        big = lib.ssq_reassign_cwt_workspace_bytes(code, 4, 1 << 16, 128, C.byref(mn))
        fixed = 32 + 16 * 4 * 128 * (1 << 16)
        assert mn.value < big <= fixed + (2 << 30) and (big - fixed - 16 * (1 << 17) * 4) % (96 << 17) == 0
        for bad in ((0, 300, 37), (1, 1, 37), (1, 300, 1), (1, 300, 40000), (1, (1 << 26) + 1, 4)):
            assert lib.ssq_reassign_cwt_workspace_bytes(code, *bad, None) == -1
            assert lib.ssq_last_error()
    assert lib.ssq_reassign_cwt_workspace_bytes(7, 1, 300, 37, None) == -1


def test_c_entry_points_refuse_on_the_host():
    lib = _lib.load()
    N, na = 100, 20
    x = np.zeros(N)
    f = m.log_freqs(N, na)
    out = np.zeros((na, N), dtype=np.complex128)
    r = np.zeros((na, N))
    mn = C.c_int64(0)
    assert lib.ssq_reassign_cwt_workspace_bytes(_lib.SSQ_F64, 1, N, na, C.byref(mn)) > 0

    def host(**kw):
        a = dict(dtype=_lib.SSQ_F64, x=_vp(x), batch=1, N=N, wavelet=0, p0=3.0, p1=60.0, scales=_vp(SC), na=na, dt=1.0,
                 f=_vp(f), kind=0, trans=0, pad=0, gamma=-1.0, variant=4, limit=0, Rx=_vp(r), Wx=_vp(out), w=None,
                 tau=None, kk=None, mm=None)
        a.update(kw)
        return lib.ssq_reassign_cwt_host(*a.values())

    def exec_(**kw):
        a = dict(dtype=_lib.SSQ_F64, x=_vp(x), batch=1, N=N, wavelet=0, p0=3.0, p1=60.0, scales=_vp(SC), na=na, dt=1.0,
                 f=_vp(f), kind=0, trans=0, pad=0, gamma=-1.0, variant=4, Rx=_vp(r), Wx=_vp(out), w=None, tau=None,
                 kk=None, mm=None, work=_vp(out), work_bytes=1 << 30, stream=None, ms=None)
        a.update(kw)
        return lib.ssq_reassign_cwt_exec(*a.values())

    for call in (host, exec_):
        for kw, word in ((dict(wavelet=2), "wavelet"), (dict(wavelet=-1), "wavelet"), (dict(p0=0.0), "p0"),
                         (dict(p0=-3.0), "p0"), (dict(p1=0.0), "p1"), (dict(wavelet=1, p0=0.0), "p0"),
                         (dict(na=1), "na"), (dict(batch=0), "batch"), (dict(N=1), "n_signal"), (dict(dtype=5), "dtype"),
                         (dict(x=None), "NULL"), (dict(scales=None), "NULL"), (dict(f=None), "NULL"),
                         (dict(Rx=None), "NULL"), (dict(Wx=None), "NULL"), (dict(dt=0.0), "dt"),
                         (dict(dt=float("inf")), "dt"), (dict(kind=3), "freq_kind"),
                         (dict(kind=2, trans=1), "freq_transition"), (dict(kind=2, trans=na), "freq_transition"),
                         (dict(pad=5), "padtype"), (dict(pad=-1), "padtype"), (dict(gamma=float("nan")), "gamma"),
                         (dict(scales=_vp(-SC)), "scales"), (dict(N=1 << 26, na=32767), "2^40")):
            assert call(**kw) != 0, kw
            assert word in lib.ssq_last_error().decode(), (kw, lib.ssq_last_error())
    assert host(limit=16) != 0 and "work_limit_bytes" in lib.ssq_last_error().decode()
    assert host(limit=mn.value - 1) != 0 and "work_limit_bytes" in lib.ssq_last_error().decode()
    assert host(limit=-1) != 0
    assert exec_(work_bytes=mn.value - 1) != 0 and "workspace" in lib.ssq_last_error().decode()
    assert exec_(work=None) != 0 and "NULL" in lib.ssq_last_error().decode()
