"""CPU tests of the surface of `upstream.set_cwt` and `upstream.tet_cwt`: the signatures, every refusal
before the GPU is asked for, the rows' edges on the three scale grids, and the C entry points exported, declared with the
header's arity, sizing their workspace (no head) and refusing bad arguments on the host."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.helpers import extract_cwt_ref as m

E = inspect.Parameter.empty
NEW = ("ssq_extract_cwt_host", "ssq_extract_cwt_workspace_bytes", "ssq_extract_cwt_exec")
BOTH = pytest.mark.parametrize("fn", [up.set_cwt, up.tet_cwt], ids=["set_cwt", "tet_cwt"])
COMMON = [("x", E), ("wavelet", "gmw"), ("scales", "log-piecewise"), ("nv", None), ("fs", None), ("t", None),
          ("padtype", "reflect"), ("order", 2), ("gamma", None), ("get_Wx", True)]
SC = 2.0 * 2.0 ** (np.arange(20) / 4)
GMW = ("gmw", {"gamma": 3.0, "beta": 60.0})
MORLET = ("morlet", {"mu": 13.4})


class _Reached(Exception):
    pass


@pytest.fixture
def no_gpu(monkeypatch):
    def refuse():
        raise _Reached("require_gpu")
    monkeypatch.setattr(up._lib, "require_gpu", refuse)


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_signatures():
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]     # noqa: E731
    assert sig(up.set_cwt) == COMMON + [("get_w", False), ("work_limit_bytes", None)]
    assert sig(up.tet_cwt) == COMMON + [("get_tau", False), ("work_limit_bytes", None)]
    assert [p.name for p in inspect.signature(up.set_cwt_row_edges).parameters.values()] == ["wavelet", "scales", "fs"]


def test_docstrings_state_the_definition():
    assert "`set_cwt` and `tet_cwt`" in up.__doc__ and "4.24" in up.__doc__
    for word in ("e[i+1] <= w < e[i]", "set_cwt_row_edges", "higher-frequency", "no inverse", "+0 + 0i", "|W| < gamma",
                 "spill"):
        assert word in up.set_cwt.__doc__, word
    for word in ("r == 0", "BEFORE", "clip", "no inverse", "+0 + 0i", "|W| < gamma", "spill"):
        assert word in up.tet_cwt.__doc__, word


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
    with open(_lib.HEADER_PATH.replace("include/ssq_hip.h", "INTEGRATION.md")) as f:
        assert "ssq_extract_cwt_exec" in f.read()


# ------------------------------------------------------------------------------------------------- the rows' edges ----
@pytest.mark.parametrize("wavelet,scales,fs", [
    (GMW, SC, None),
    (GMW, np.linspace(2, 60, 50), 250.0),
    (MORLET, None, 2.0),                                       # upstream's log-piecewise grid of 777 samples
], ids=["log", "linear", "log-piecewise"])
def test_row_edges_on_the_three_scale_grids(wavelet, scales, fs):
    if scales is None:
        scales = np.ascontiguousarray(up.process_scales("log-piecewise", 777, wavelet, nv=8), dtype=np.float64).reshape(-1)
        assert up._scales(scales)[1] == "log-piecewise"
    na, dt = len(scales), 1.0 if fs is None else 1.0 / fs
    e = up.set_cwt_row_edges(wavelet, scales, fs=fs)
    nu = up.tssq_cwt_row_freqs(wavelet, scales)
    assert e.dtype == np.float64 and e.shape == (na + 1,)
    assert e[0] == np.inf and e[na] == 0.0
    assert np.array_equal(e[1:na], np.sqrt(nu[:-1] * nu[1:]) / dt)
    assert (np.diff(e) < 0).all()
    assert ((e[1:na] < nu[:-1] / dt) & (e[1:na] > nu[1:] / dt)).all()     # every row's own frequency lies in its band
    assert np.allclose(np.log(e[1:na]), 0.5 * (np.log(nu[:-1] / dt) + np.log(nu[1:] / dt)), rtol=1e-14, atol=1e-14)
    mw = (wavelet[0], *up._wavelet(wavelet)[1:]) if wavelet[0] == "gmw" else (wavelet[0], up._wavelet(wavelet)[1])
    assert np.array_equal(e, m.row_edges(mw, scales, dt))      # the model's edges are these


def test_row_edges_refusals():
    with pytest.raises(ValueError, match="decreasing"):
        up.set_cwt_row_edges("gmw", SC[::-1].copy())
    with pytest.raises(ValueError, match="decreasing"):
        up.set_cwt_row_edges("gmw", np.array([4.0, 4.0, 5.0]))
    with pytest.raises(ValueError, match="decreasing"):
        up.set_cwt_row_edges("gmw", np.array([4.0]))
    with pytest.raises(ValueError, match="scales"):
        up.set_cwt_row_edges("gmw", -SC)
    with pytest.raises(ValueError, match="wavelet"):
        up.set_cwt_row_edges("bump", SC)
    for fs in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sampling period"):
            up.set_cwt_row_edges("gmw", SC, fs=fs)


# ----------------------------------------------------------------------------------------------------- the refusals ----
@BOTH
def test_refusals_come_before_the_gpu(no_gpu, fn):
    x = np.random.default_rng(1).standard_normal(300)
    with pytest.raises(ValueError, match="scales"):
        fn(x)                                                    # the string default, as tssq_cwt
    with pytest.raises(ValueError, match="scales"):
        fn(x, scales="log")
    with pytest.raises(ValueError, match="scales"):
        fn(x, scales=np.array([4.0]))
    with pytest.raises(ValueError, match="scales"):
        fn(x, scales=-SC)
    with pytest.raises(ValueError, match="scales"):
        fn(x, scales=np.concatenate([[0.0], SC]))
    with pytest.raises(ValueError, match="scales"):
        fn(x, scales=np.concatenate([SC, [np.inf]]))
    with pytest.raises(ValueError, match="padtype"):
        fn(x, scales=SC, padtype="constant")
    for order in (0, 3, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="order"):
            fn(x, scales=SC, order=order)
    with pytest.raises(ValueError, match="order"):
        fn(x, ("gmw", {"order": 1}), scales=SC)
    with pytest.raises(ValueError, match="wavelet"):
        fn(x, "bump", scales=SC)
    with pytest.raises(ValueError, match="wavelet"):
        fn(x, ("gmw", {"beta": -1.0}), scales=SC)
    with pytest.raises(ValueError, match="wavelet"):
        fn(x, ("gmw", {"gamma": float("inf")}), scales=SC)
    with pytest.raises(ValueError, match="wavelet"):
        fn(x, ("morlet", {"mu": 0.0}), scales=SC)
    with pytest.raises(ValueError, match="gamma"):
        fn(x, scales=SC, gamma=float("nan"))
    with pytest.raises(ValueError, match="sampling period"):
        fn(x, scales=SC, fs=-1.0)
    with pytest.raises(ValueError, match="sampling period"):
        fn(x, scales=SC, fs=float("nan"))
    with pytest.raises(ValueError, match="`t`"):
        fn(x, scales=SC, t=np.arange(10))
    with pytest.raises(ValueError, match="nv"):
        fn(x, scales=SC, nv=8)
    with pytest.raises(ValueError, match="work_limit_bytes"):
        fn(x, scales=SC, work_limit_bytes=1024)
    with pytest.raises(TypeError):
        fn(list(x), scales=SC)
    with pytest.raises(ValueError, match="samples"):
        fn(np.zeros(1), scales=SC)
    for gone in ("ssq_freqs", "maprange", "squeezing", "flipud", "n_iter", "get_targets"):
        with pytest.raises(TypeError):
            fn(x, scales=SC, **{gone: None})


def test_set_cwt_refuses_rows_that_do_not_strictly_decrease(no_gpu):
    """Decreasing scales are rows of increasing frequency: `set_cwt` has no edges for them; `tet_cwt` has no use for edges."""
    x = np.zeros(300)
    with pytest.raises(ValueError, match="decreasing"):
        up.set_cwt(x, scales=SC[::-1].copy())
    with pytest.raises(_Reached):
        up.tet_cwt(x, scales=SC[::-1].copy())


@BOTH
@pytest.mark.parametrize("kw", [dict(), dict(wavelet=MORLET, padtype="wrap", order=1, get_Wx=False, fs=2.0, gamma=1e-6),
                                dict(wavelet=("gmw", {"gamma": 3, "beta": 20}), nv=4, padtype="symmetric")])
@pytest.mark.parametrize("shape,dtype", [((300,), np.float64), ((2, 300), np.float32)])
def test_well_formed_calls_reach_the_gpu(no_gpu, fn, kw, shape, dtype):
    x = np.random.default_rng(2).standard_normal(shape).astype(dtype)
    for sc in (SC, np.linspace(2, 60, 50)):
        if kw.get("nv") and len(sc) != 20:
            continue
        with pytest.raises(_Reached):
            fn(x, scales=sc, **kw)
    with pytest.raises(_Reached):
        fn(x, scales=SC, **{"get_w" if fn is up.set_cwt else "get_tau": True})


@BOTH
def test_log_piecewise_scales_and_a_work_limit_reach_the_gpu(no_gpu, fn):
    sc = np.ascontiguousarray(up.process_scales("log-piecewise", 777, MORLET, nv=8), dtype=np.float64).reshape(-1)
    mn = C.c_int64(0)
    assert _lib.load().ssq_extract_cwt_workspace_bytes(_lib.SSQ_F64, 1, 777, len(sc), 2, C.byref(mn)) > 0
    with pytest.raises(_Reached):
        fn(np.zeros(777), MORLET, scales=sc, padtype="replicate", work_limit_bytes=mn.value)
    with pytest.raises(ValueError, match="work_limit_bytes"):
        fn(np.zeros(777), MORLET, scales=sc, work_limit_bytes=mn.value - 1)


def test_more_cells_than_tssq_cwt_takes_are_sized():
    """na N > 2^40 is `tssq_cwt`'s limit, for its accumulators; there are none here."""
    lib = _lib.load()
    for order in (1, 2):
        assert lib.ssq_tssq_cwt_workspace_bytes(_lib.SSQ_F32, 1, 1 << 26, 32767, order, None) == -1
        assert lib.ssq_extract_cwt_workspace_bytes(_lib.SSQ_F32, 1, 1 << 26, 32767, order, None) > 0


# ----------------------------------------------------------------------------------------------- the C entry points ----
def test_workspace_bytes():
    """16 P (batch + 2 M R) and nothing else: no head term, min <= pref, the limits of ssq_cwt2."""
    lib = _lib.load()
    mn, mn2 = C.c_int64(0), C.c_int64(0)
    for code in (_lib.SSQ_F32, _lib.SSQ_F64):
        for order, M in ((1, 2), (2, 5)):
            # N = 300 -> P = 512
            assert lib.ssq_extract_cwt_workspace_bytes(code, 3, 300, 37, order, C.byref(mn)) == 16 * 512 * (3 + 2 * M * 3 * 37)
            assert mn.value == 16 * 512 * (3 + 2 * M)
            assert lib.ssq_extract_cwt_workspace_bytes(code, 1, 301, 37, order, C.byref(mn)) == 16 * 512 * (1 + 2 * M * 37)
            assert mn.value == 16 * 512 * (1 + 2 * M)
            # the chunk area capped at 2 GiB: batch 4 x 2^16 samples (P = 2^17) x 128 scales
            big = lib.ssq_extract_cwt_workspace_bytes(code, 4, 1 << 16, 128, order, C.byref(mn))
            assert mn.value < big <= (2 << 30) and (big - 16 * (1 << 17) * 4) % ((32 * M) << 17) == 0
            assert mn.value == 16 * (1 << 17) * (4 + 2 * M)
            for bad in ((0, 300, 37), (1, 1, 37), (1, 300, 1), (1, 300, 40000), (1, (1 << 26) + 1, 4)):
                assert lib.ssq_extract_cwt_workspace_bytes(code, *bad, order, None) == -1
                assert lib.ssq_last_error()
        # order 2 is ssq_cwt2's workspace exactly; tssq_cwt's is this plus its head
        pref = lib.ssq_extract_cwt_workspace_bytes(code, 3, 300, 37, 2, C.byref(mn))
        assert pref == lib.ssq_ssq_cwt2_workspace_bytes(code, 3, 300, 37, C.byref(mn2)) and mn.value == mn2.value
        assert lib.ssq_tssq_cwt_workspace_bytes(code, 3, 300, 37, 2, C.byref(mn2)) == pref + 32 + 20 * 3 * 37 * 300
        for order in (0, 3, -1):
            assert lib.ssq_extract_cwt_workspace_bytes(code, 1, 300, 37, order, None) == -1
            assert "order" in lib.ssq_last_error().decode()
    assert lib.ssq_extract_cwt_workspace_bytes(7, 1, 300, 37, 2, None) == -1 and "dtype" in lib.ssq_last_error().decode()


def test_c_entry_points_refuse_on_the_host():
    lib = _lib.load()
    err = lambda: lib.ssq_last_error().decode()                                      # noqa: E731
    N, na = 100, 20
    x = np.zeros(N)
    nu = up.tssq_cwt_row_freqs("gmw", SC)
    edges = up.set_cwt_row_edges("gmw", SC)
    bad_nu = nu.copy()
    bad_nu[3] = float("nan")

    def changed(i, v):
        e = edges.copy()
        e[i] = v
        return e
    out = np.zeros((na, N), dtype=np.complex128)
    mn = C.c_int64(0)
    assert lib.ssq_extract_cwt_workspace_bytes(_lib.SSQ_F64, 1, N, na, 2, C.byref(mn)) > 0

    def host(**kw):
        a = dict(dtype=_lib.SSQ_F64, x=_vp(x), batch=1, N=N, wavelet=0, p0=3.0, p1=60.0, scales=_vp(SC), nu=_vp(nu),
                 edges=_vp(edges), na=na, dt=1.0, pad=0, axis=0, order=2, gamma=-1.0, limit=0, Te=_vp(out), Wx=None, mp=None)
        a.update(kw)
        return lib.ssq_extract_cwt_host(*a.values())

    def exec_(**kw):
        a = dict(dtype=_lib.SSQ_F64, x=_vp(x), batch=1, N=N, wavelet=0, p0=3.0, p1=60.0, scales=_vp(SC), nu=_vp(nu),
                 edges=_vp(edges), na=na, dt=1.0, pad=0, axis=0, order=2, gamma=-1.0, Te=_vp(out), Wx=None, mp=None,
                 work=_vp(out), work_bytes=1 << 30, stream=None, ms=None)
        a.update(kw)
        return lib.ssq_extract_cwt_exec(*a.values())

    keep = []                                                    # (the arrays the pointers below point into)

    def ptr(a):
        keep.append(np.ascontiguousarray(a))
        return _vp(keep[-1])
    for call in (host, exec_):
        for kw, word in ((dict(wavelet=2), "wavelet"), (dict(wavelet=-1), "wavelet"), (dict(p0=0.0), "p0"),
                         (dict(p0=-3.0), "p0"), (dict(p0=float("inf")), "p0"), (dict(p1=0.0), "p1"),
                         (dict(p1=float("nan")), "p1"), (dict(wavelet=1, p0=0.0), "p0"), (dict(na=1), "na"),
                         (dict(batch=0), "batch"), (dict(N=1), "n_signal"), (dict(dtype=5), "dtype"),
                         (dict(x=None), "NULL"), (dict(scales=None), "NULL"), (dict(Te=None), "NULL"),
                         (dict(dt=0.0), "dt"), (dict(dt=float("inf")), "dt"), (dict(dt=float("nan")), "dt"),
                         (dict(order=0), "order"), (dict(order=3), "order"), (dict(axis=-1), "axis"),
                         (dict(axis=2), "axis"), (dict(pad=5), "padtype"), (dict(pad=-1), "padtype"),
                         (dict(gamma=float("nan")), "gamma"), (dict(scales=ptr(-SC)), "scales"),
                         # the table the axis uses is required; one that is given is checked on either axis
                         (dict(axis=0, edges=None), "NULL"), (dict(axis=1, nu=None), "NULL"),
                         (dict(axis=1, nu=ptr(-nu)), "row_freqs"), (dict(axis=1, nu=ptr(bad_nu)), "row_freqs"),
                         (dict(axis=0, nu=ptr(bad_nu)), "row_freqs"),
                         (dict(edges=ptr(changed(5, float("nan")))), "row_edges"),
                         (dict(edges=ptr(changed(0, float("nan")))), "row_edges"),
                         (dict(edges=ptr(changed(0, 1e300))), "row_edges"),
                         (dict(edges=ptr(changed(na, 1e-300))), "row_edges"),
                         (dict(edges=ptr(changed(na, -0.5))), "row_edges"),
                         (dict(edges=ptr(changed(7, edges[6] * 1.01))), "row_edges"),
                         (dict(axis=1, edges=ptr(changed(7, edges[6] * 1.01))), "row_edges")):
            assert call(**kw) != 0, kw
            assert word in err(), (kw, err())
    assert "NaN" in (host(edges=ptr(changed(5, float("nan")))), err())[1]
    assert "+inf to 0" in (host(edges=ptr(changed(0, 1e300))), err())[1]
    assert "increase" in (host(edges=ptr(changed(7, edges[6] * 1.01))), err())[1]
    assert host(limit=16) != 0 and "work_limit_bytes" in err()
    assert host(limit=mn.value - 1) != 0 and "work_limit_bytes" in err()
    assert host(limit=-1) != 0
    assert exec_(work_bytes=mn.value - 1) != 0 and "workspace" in err() and "ssq_extract_cwt_workspace_bytes" in err()
    assert exec_(work=None) != 0 and "NULL" in err()
    if _lib.device_count() < 1:
        # a good call gets as far as the device check: with the other axis's table left out, with equal edges (a step that
        # does not increase), and unlike tssq_cwt with 2^26 samples x 32767 scales (sized by the checks alone)
        for call in (host, exec_):
            for kw in (dict(), dict(axis=0, nu=None), dict(axis=1, edges=None), dict(axis=1, order=1),
                       dict(edges=ptr(changed(7, edges[6]))), dict(limit=mn.value) if call is host else dict(work_bytes=mn.value)):
                assert call(**kw) != 0 and "no HIP device" in err(), kw
