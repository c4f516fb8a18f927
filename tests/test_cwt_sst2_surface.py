"""CPU tests of `upstream.ssq_cwt2`'s surface: the signature, every refusal before the GPU is asked for, the C entry
points exported, declared, bound and refusing bad arguments on the host, and the wavelet tables the library builds."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.helpers import cwt_sst2_ref as m

E = inspect.Parameter.empty
NEW = ("ssq_ssq_cwt2_host", "ssq_ssq_cwt2_workspace_bytes", "ssq_ssq_cwt2_exec", "ssq_ssq_cwt2_tables")
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
    sig = [(p.name, p.default) for p in inspect.signature(up.ssq_cwt2).parameters.values()]
    assert sig == [("x", E), ("wavelet", "gmw"), ("scales", "log-piecewise"), ("nv", None), ("fs", None), ("t", None),
                   ("ssq_freqs", None), ("padtype", "reflect"), ("squeezing", "sum"), ("maprange", "peak"),
                   ("gamma", None), ("flipud", True), ("get_w", False)]


def test_docstrings_name_the_feature():
    assert "ssq_cwt2" in up.__doc__ and "4.12" in up.__doc__
    assert "Im om2" in up.ssq_cwt2.__doc__ and "fp64" in up.ssq_cwt2.__doc__


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
        up.ssq_cwt2(x)                                           # the string default, as ssq_cwt
    with pytest.raises(ValueError, match="scales"):
        up.ssq_cwt2(x, scales="log")
    with pytest.raises(ValueError, match="scales"):
        up.ssq_cwt2(x, scales=np.array([4.0]))
    with pytest.raises(ValueError, match="scales"):
        up.ssq_cwt2(x, scales=-SC)
    with pytest.raises(ValueError, match="squeezing"):
        up.ssq_cwt2(x, scales=SC, squeezing="abs")
    with pytest.raises(ValueError, match="padtype"):
        up.ssq_cwt2(x, scales=SC, padtype="constant")
    with pytest.raises(ValueError, match="maprange"):
        up.ssq_cwt2(x, scales=SC, maprange="energy")
    with pytest.raises(ValueError, match="maprange"):
        up.ssq_cwt2(x, scales=SC, ssq_freqs="log-piecewise", maprange="maximal")
    with pytest.raises(ValueError, match="ssq_freqs"):
        up.ssq_cwt2(x, scales=SC, ssq_freqs=np.linspace(0.01, 0.5, 7))
    with pytest.raises(ValueError, match="ssq_freqs"):
        up.ssq_cwt2(x, scales=SC, ssq_freqs=3)
    with pytest.raises(ValueError, match="order"):
        up.ssq_cwt2(x, ("gmw", {"order": 1}), scales=SC)
    with pytest.raises(ValueError, match="norm"):
        up.ssq_cwt2(x, ("gmw", {"norm": "energy"}), scales=SC)
    with pytest.raises(ValueError, match="wavelet"):
        up.ssq_cwt2(x, "bump", scales=SC)
    with pytest.raises(ValueError, match="wavelet"):
        up.ssq_cwt2(x, ("gmw", {"beta": -1.0}), scales=SC)
    with pytest.raises(ValueError, match="gamma"):
        up.ssq_cwt2(x, scales=SC, gamma=float("nan"))
    with pytest.raises(ValueError, match="`t`"):
        up.ssq_cwt2(x, scales=SC, t=np.arange(10))
    with pytest.raises(Exception, match="nv"):
        up.ssq_cwt2(x, scales=SC, nv=8)
    with pytest.raises(TypeError):
        up.ssq_cwt2(list(x), scales=SC)
    with pytest.raises(TypeError):
        up.ssq_cwt2(np.zeros((2, 3, 40)), scales=SC)
    with pytest.raises(ValueError, match="samples"):
        up.ssq_cwt2(np.zeros(1), scales=SC)


@pytest.mark.parametrize("kw", [dict(), dict(wavelet=("morlet", {"mu": 6.0}), padtype="wrap", squeezing="lebesgue",
                                             flipud=False, get_w=True, fs=2.0, gamma=1e-6, maprange="maximal",
                                             ssq_freqs="linear"),
                                dict(wavelet=("gmw", {"gamma": 3, "beta": 20}), nv=4, padtype="symmetric",
                                     ssq_freqs=np.linspace(0.01, 0.5, 20))])
@pytest.mark.parametrize("shape,dtype", [((300,), np.float64), ((2, 300), np.float32)])
def test_well_formed_calls_reach_the_gpu(no_gpu, kw, shape, dtype):
    x = np.random.default_rng(2).standard_normal(shape).astype(dtype)
    for sc in (SC, np.linspace(2, 60, 50)):
        if kw.get("nv") and len(sc) == 50:
            continue
        if isinstance(kw.get("ssq_freqs"), np.ndarray) and len(sc) == 50:
            continue
        with pytest.raises(_Reached):
            up.ssq_cwt2(x, scales=sc, **kw)


def test_ssq_cwt_still_takes_its_grids_from_the_shared_helper(no_gpu):
    x = np.zeros(300)
    with pytest.raises(ValueError, match="scales"):
        up.ssq_cwt(x)
    with pytest.raises(ValueError, match="maprange"):
        up.ssq_cwt(x, scales=SC, ssq_freqs="log-piecewise", maprange="maximal")
    with pytest.raises(_Reached):
        up.ssq_cwt(x, scales=SC)
    s, rc, f, kind, idx = up._cwt_freq_grid(SC, None, None, "maximal", 300, 0, 3.0, 60.0, 0.5)
    assert kind == "log" and idx is None and np.array_equal(s, SC) and np.allclose(rc, np.log(2) / 4)
    assert np.allclose(f, m.log_freqs(300, 20, 0.5), rtol=1e-15)


def test_workspace_bytes():
    lib = _lib.load()
    mn = C.c_int64(0)
    for code in (_lib.SSQ_F32, _lib.SSQ_F64):
        # N = 300 -> P = 512; 16 P (batch + 10 R) bytes: every row in one chunk, one row at the least
        assert lib.ssq_ssq_cwt2_workspace_bytes(code, 3, 300, 37, C.byref(mn)) == 16 * 512 * (3 + 10 * 3 * 37)
        assert mn.value == 16 * 512 * (3 + 10)
        assert lib.ssq_ssq_cwt2_workspace_bytes(code, 1, 300, 37, None) == 16 * 512 * (1 + 10 * 37)
        # capped at 2 GiB: batch 4 x 2^16 samples (P = 2^17) x 128 scales
        big = lib.ssq_ssq_cwt2_workspace_bytes(code, 4, 1 << 16, 128, C.byref(mn))
        assert mn.value < big <= 2 << 30 and (big - 16 * (1 << 17) * 4) % (160 << 17) == 0
        for bad in ((0, 300, 37), (1, 1, 37), (1, 300, 1), (1, 300, 40000), (1, (1 << 26) + 1, 4)):
            assert lib.ssq_ssq_cwt2_workspace_bytes(code, *bad, None) == -1
            assert lib.ssq_last_error()
    assert lib.ssq_ssq_cwt2_workspace_bytes(7, 1, 300, 37, None) == -1


def test_c_entry_points_refuse_on_the_host():
    lib = _lib.load()
    N, na = 100, 20
    x = np.zeros(N)
    rc = np.full(na, 0.1)
    f = m.log_freqs(N, na)
    out = np.zeros((na, N), dtype=np.complex128)
    w = np.zeros((na, N))

    def host(**kw):
        a = dict(dtype=_lib.SSQ_F64, x=_vp(x), batch=1, N=N, wavelet=0, p0=3.0, p1=60.0, scales=_vp(SC), na=na, dt=1.0,
                 row_const=_vp(rc), f=_vp(f), kind=0, trans=0, pad=0, sq=0, gamma=-1.0, variant=4, limit=0, Tx=_vp(out),
                 Wx=_vp(out), w2=_vp(w))
        a.update(kw)
        return lib.ssq_ssq_cwt2_host(*a.values())

    def exec_(**kw):
        a = dict(dtype=_lib.SSQ_F64, x=_vp(x), batch=1, N=N, wavelet=0, p0=3.0, p1=60.0, scales=_vp(SC), na=na, dt=1.0,
                 row_const=_vp(rc), f=_vp(f), kind=0, trans=0, pad=0, sq=0, gamma=-1.0, variant=4, Tx=_vp(out),
                 Wx=_vp(out), w2=_vp(w), work=_vp(out), work_bytes=1 << 30, stream=None, ms=None)
        a.update(kw)
        return lib.ssq_ssq_cwt2_exec(*a.values())

    for call in (host, exec_):
        for kw, word in ((dict(wavelet=2), "wavelet"), (dict(wavelet=-1), "wavelet"), (dict(p0=0.0), "p0"),
                         (dict(p0=-3.0), "p0"), (dict(p1=0.0), "p1"), (dict(wavelet=1, p0=0.0), "p0"),
                         (dict(na=1), "na"), (dict(batch=0), "batch"), (dict(N=1), "n_signal"), (dict(dtype=5), "dtype"),
                         (dict(x=None), "NULL"), (dict(scales=None), "NULL"), (dict(row_const=None), "NULL"),
                         (dict(f=None), "NULL"), (dict(Tx=None), "NULL"), (dict(Wx=None), "NULL"), (dict(dt=0.0), "dt"),
                         (dict(kind=3), "freq_kind"), (dict(kind=2, trans=1), "freq_transition"),
                         (dict(kind=2, trans=na), "freq_transition"), (dict(pad=5), "padtype"), (dict(sq=2), "squeezing"),
                         (dict(gamma=float("nan")), "gamma"), (dict(scales=_vp(-SC)), "scales")):
            assert call(**kw) != 0, kw
            assert word in lib.ssq_last_error().decode(), (kw, lib.ssq_last_error())
    assert host(limit=16) != 0 and "work_limit_bytes" in lib.ssq_last_error().decode()
    assert host(limit=-1) != 0
    assert exec_(work_bytes=16 * 256 * 11 - 1) != 0 and "workspace" in lib.ssq_last_error().decode()
    assert exec_(work=None) != 0 and exec_(w2=None) != 0


@pytest.mark.parametrize("P", [64, 512])
@pytest.mark.parametrize("wavelet", [("gmw", 3.0, 60.0), ("gmw", 2.0, 7.5), ("morlet", 13.4), ("morlet", 5.0)],
                         ids=lambda w: "-".join(str(v) for v in w))
def test_tables_are_the_definitions(wavelet, P):
    """`ssq_ssq_cwt2_tables` (the functions the kernel evaluates, about the wavelet's peak: csrc/cwt_sst2_wavelets.h)
    against the model's tables by the textbook expressions, to 1e-13 of each table's maximum, over scales from the
    smallest (peak at Nyquist) to one with the peak near bin 6 (a grid that still resolves the wavelet: where the bins
    either side of the peak are far down the tails, the table's maximum is itself rounding noise of psih' at the peak,
    in either way of evaluating it)."""
    lib = _lib.load()
    code = 0 if wavelet[0] == "gmw" else 1
    p0, p1 = wavelet[1], (wavelet[2] if code == 0 else 0.0)
    wc = m.gmw_wc(p0, p1) if code == 0 else p0
    scales = wc / np.pi * np.array([1.0, 1.7, 4.0, 1.3 * P / 16.0])
    R0, R1 = m.tables(wavelet, scales, P)
    for i, a in enumerate(scales):
        T0, T1 = np.empty(P), np.empty(P)
        assert lib.ssq_ssq_cwt2_tables(code, p0, p1, float(a), P, _vp(T0), _vp(T1)) == 0
        assert not T0[P // 2 + 1:].any() and not T1[P // 2 + 1:].any()
        e0, e1 = np.abs(T0 - R0[i]).max() / np.abs(R0[i]).max(), np.abs(T1 - R1[i]).max() / np.abs(R1[i]).max()
        print("scale %.4g: T0 %.3g  T1 %.3g" % (a, e0, e1))
        assert e0 <= 1e-13 and e1 <= 1e-13
    T0, T1 = np.empty(P), np.empty(P)
    assert lib.ssq_ssq_cwt2_tables(2, p0, p1, 4.0, P, _vp(T0), _vp(T1)) != 0
    assert lib.ssq_ssq_cwt2_tables(code, -1.0, p1, 4.0, P, _vp(T0), _vp(T1)) != 0
    assert lib.ssq_ssq_cwt2_tables(code, p0, p1, 0.0, P, _vp(T0), _vp(T1)) != 0
    assert lib.ssq_ssq_cwt2_tables(code, p0, p1, 4.0, 48, _vp(T0), _vp(T1)) != 0
    assert lib.ssq_ssq_cwt2_tables(code, p0, p1, 4.0, P, None, _vp(T1)) != 0
