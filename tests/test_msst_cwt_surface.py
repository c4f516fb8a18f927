"""CPU tests of the surface of `upstream.mssq_cwt`, `mssq_cwt_walk`, `mssq_cwt_row_of_bin` and `mssq_cwt_tile_cols`: the
signatures, every refusal before the GPU is asked for, and the C entry points exported, declared, bound and refusing bad
arguments on the host, message by message."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up

E = inspect.Parameter.empty
NEW = ("ssq_mssq_cwt_host", "ssq_mssq_cwt_workspace_bytes", "ssq_mssq_cwt_exec", "ssq_mssq_cwt_walk_host",
       "ssq_mssq_cwt_tile_cols")
GMW = ("gmw", {"gamma": 3.0, "beta": 60.0})
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
    sig = [(p.name, p.default) for p in inspect.signature(up.mssq_cwt).parameters.values()]
    assert sig == [("x", E), ("wavelet", "gmw"), ("scales", "log-piecewise"), ("nv", None), ("fs", None), ("t", None),
                   ("ssq_freqs", None), ("padtype", "reflect"), ("squeezing", "sum"), ("maprange", "peak"), ("gamma", None),
                   ("flipud", True), ("order", 2), ("n_iter", 4), ("get_w", False), ("get_rows", False), ("get_bins", False)]
    names = [p.name for p in inspect.signature(up.ssq_cwt2).parameters.values()]
    assert [n for n, _ in sig[:12]] == names[:12]                          # the front of `ssq_cwt2`'s signature
    assert [(p.name, p.default) for p in inspect.signature(up.mssq_cwt_walk).parameters.values()] == [
        ("w", E), ("ssq_freqs_asc", E), ("row_of_bin", E), ("n_iter", E)]
    assert [(p.name, p.default) for p in inspect.signature(up.mssq_cwt_row_of_bin).parameters.values()] == [
        ("wavelet", E), ("scales", E), ("ssq_freqs_asc", E), ("fs", None)]
    assert [p.name for p in inspect.signature(up.mssq_cwt_tile_cols).parameters.values()] == ["na"]


def test_docstrings_name_the_feature():
    assert "mssq_cwt" in up.__doc__ and "mssq_cwt_walk" in up.__doc__ and "mssq_cwt_row_of_bin" in up.__doc__
    doc = up.mssq_cwt.__doc__
    for word in ("rho", "n_iter", "fixed point", "rows ascending", "flipud", "row weight", "2049", "spill", "bit for bit"):
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


@pytest.mark.parametrize("order", [0, 3, -1, 1.5, True, "2", None])
def test_order_refusals_come_before_the_gpu(no_gpu, order):
    with pytest.raises(ValueError, match="order"):
        up.mssq_cwt(np.zeros(300), GMW, scales=SC, order=order)


@pytest.mark.parametrize("n_iter", [0, -1, 65, 1000, 2.0, 2.5, True, False, "4", None])
def test_n_iter_refusals_come_before_the_gpu(no_gpu, n_iter):
    with pytest.raises(ValueError, match="n_iter"):
        up.mssq_cwt(np.zeros(300), GMW, scales=SC, n_iter=n_iter)
    f = np.linspace(1.0, 2.0, 9)
    with pytest.raises(ValueError, match="n_iter"):
        up.mssq_cwt_walk(np.ones((9, 4)), f, np.arange(9), n_iter)


def test_other_refusals_come_before_the_gpu(no_gpu):
    x = np.random.default_rng(1).standard_normal(300)
    with pytest.raises(ValueError, match="squeezing"):
        up.mssq_cwt(x, GMW, scales=SC, squeezing="abs")
    with pytest.raises(ValueError, match="padtype"):
        up.mssq_cwt(x, GMW, scales=SC, padtype="constant")
    with pytest.raises(ValueError, match="scales"):
        up.mssq_cwt(x, GMW)                                               # the string forms of `scales`
    with pytest.raises(ValueError, match="scales"):
        up.mssq_cwt(x, GMW, scales=-SC)
    with pytest.raises(ValueError, match="maprange"):
        up.mssq_cwt(x, GMW, scales=SC, maprange="energy")
    with pytest.raises(ValueError, match="ssq_freqs"):
        up.mssq_cwt(x, GMW, scales=SC, ssq_freqs=np.linspace(0.1, 0.5, 7))
    with pytest.raises(ValueError, match="gamma"):
        up.mssq_cwt(x, GMW, scales=SC, gamma=float("nan"))
    with pytest.raises(ValueError, match="wavelet"):
        up.mssq_cwt(x, ("gmw", {"gamma": -3.0, "beta": 60.0}), scales=SC)
    with pytest.raises(ValueError, match="2 samples"):
        up.mssq_cwt(np.zeros(1), GMW, scales=SC)
    with pytest.raises(TypeError):
        up.mssq_cwt(list(x), GMW, scales=SC)
    with pytest.raises(ValueError, match="2049"):
        up.mssq_cwt(x, GMW, scales=2.0 * 2.0 ** (np.arange(2050) / 256))
    with pytest.raises(_Reached):
        up.mssq_cwt(x, GMW, scales=2.0 * 2.0 ** (np.arange(2049) / 256))


def test_walk_refusals_come_before_the_gpu(no_gpu):
    good = np.ones((9, 4))
    f = 0.01 * 2.0 ** (np.arange(9) / 2)
    rho = np.arange(9)[::-1]
    for bad in (good.astype(np.int32), good.astype(np.float16), list(good), good[0], np.ones((2, 2, 9, 4)),
                np.ones((2050, 2)), np.ones((1, 4)), np.ones((9, 0))):
        with pytest.raises(ValueError, match="`w`"):
            up.mssq_cwt_walk(bad, f, rho, 2)
    for bad_f in (f[:8], list(f), f[::-1], np.where(np.arange(9) == 3, np.nan, f), np.arange(9)):
        with pytest.raises(ValueError, match="ssq_freqs_asc"):
            up.mssq_cwt_walk(good, bad_f, rho, 2)
    for bad_rho in (rho[:8], rho.astype(np.float64), np.where(np.arange(9) == 3, 9, rho), np.where(np.arange(9) == 3, -1, rho)):
        with pytest.raises(ValueError, match="row_of_bin"):
            up.mssq_cwt_walk(good, f, bad_rho, 2)
    inf = good.copy()
    inf[3, 1] = np.inf
    for wv, ff in ((inf, f), (np.stack([inf, inf]).astype(np.float32), f), (np.asfortranarray(inf), np.linspace(0.0, 1.0, 9)),
                   (good[:2], f[:2])):
        with pytest.raises(_Reached):
            up.mssq_cwt_walk(wv, ff, list(rho[:len(ff)] - rho[:len(ff)].min()), 64)


@pytest.mark.parametrize("kw", [dict(), dict(padtype="wrap", squeezing="lebesgue", flipud=False, get_w=True, get_rows=True,
                                             get_bins=True, fs=2.0, gamma=1e-6, order=1, n_iter=64, maprange="maximal"),
                                dict(order=2, n_iter=1, get_rows=True, ssq_freqs="linear")])
@pytest.mark.parametrize("shape,dtype", [((300,), np.float64), ((2, 300), np.float32)])
def test_well_formed_calls_reach_the_gpu(no_gpu, kw, shape, dtype):
    x = np.random.default_rng(2).standard_normal(shape).astype(dtype)
    for wavelet, sc in ((GMW, SC), (("morlet", {"mu": 13.4}), np.linspace(2, 60, 50))):
        with pytest.raises(_Reached):
            up.mssq_cwt(x, wavelet, scales=sc, **kw)


def test_tile_widths():
    """The tile table of DESIGN 4.20: the widest of 16 .. 256 columns with na C <= 33024 16-bit words (66048 bytes)."""
    lib = _lib.load()
    table = {2: 256, 9: 256, 128: 256, 129: 256, 130: 128, 257: 128, 258: 128, 259: 64, 516: 64, 517: 32, 1032: 32, 1033: 16,
             2049: 16}
    for na, cols in table.items():
        assert up.mssq_cwt_tile_cols(na) == cols and 2 * na * cols <= 66048, na
        assert cols == 256 or 2 * na * 2 * cols > 66048, na                # (the widest that fits)
    for na in (1, 0, -3, 2050):
        assert lib.ssq_mssq_cwt_tile_cols(na) == -1
        assert "na" in lib.ssq_last_error().decode()
        with pytest.raises(ValueError):
            up.mssq_cwt_tile_cols(na)


def test_c_entry_points_refuse_on_the_host():
    lib = _lib.load()
    mn, mn2 = C.c_int64(0), C.c_int64(0)
    for code, esz in ((_lib.SSQ_F32, 4), (_lib.SSQ_F64, 8)):
        want = lib.ssq_ssq_cwt2_workspace_bytes(code, 3, 1000, 20, C.byref(mn2))
        head = (esz * 3 * 20 * 1000 + 15) // 16 * 16
        assert want > 0 and lib.ssq_mssq_cwt_workspace_bytes(code, 3, 1000, 20, C.byref(mn)) == want + head
        assert mn.value == mn2.value + head
        for na, word in ((1, "na"), (2050, "na")):
            assert lib.ssq_mssq_cwt_workspace_bytes(code, 1, 1000, na, None) == -1
            assert word in lib.ssq_last_error().decode()
        assert lib.ssq_mssq_cwt_workspace_bytes(code, 0, 1000, 20, None) == -1
        assert lib.ssq_mssq_cwt_workspace_bytes(code, 1, 1, 20, None) == -1
    assert lib.ssq_mssq_cwt_workspace_bytes(7, 1, 1000, 20, None) == -1

    N, na = 100, 20
    x = np.zeros(N)
    sc, rc = SC.copy(), np.full(na, 0.1)
    f = 0.01 * 2.0 ** (np.arange(na) / 4)
    rho = np.arange(na, dtype=np.int32)[::-1].copy()
    out = np.zeros((na, N), dtype=np.complex128)

    def host(dtype=_lib.SSQ_F64, xp=_vp(x), wavelet=0, scales=sc, na_=na, dt=1.0, rcp=_vp(rc), fp=_vp(f), kind=0, tr=0, pad=0,
             sq=0, gamma=-1.0, limit=0, order=2, n_iter=4, rho_=rho, Tx=_vp(out)):
        return lib.ssq_mssq_cwt_host(dtype, xp, 1, N, wavelet, 3.0, 60.0, _vp(scales), na_, dt, rcp, fp, kind, tr, pad, sq, gamma,
                                     4, limit, order, n_iter, None if rho_ is None else _vp(rho_), Tx, _vp(out), None, None, None)

    bad_rho_hi, bad_rho_lo = rho.copy(), rho.copy()
    bad_rho_hi[7], bad_rho_lo[0] = na, -1
    bad_sc, bad_f = sc.copy(), f.copy()
    bad_sc[3], bad_f[5] = -1.0, np.inf
    cases = ((dict(dtype=5), "dtype"), (dict(xp=None), "NULL"), (dict(Tx=None), "NULL"), (dict(order=0), "order"),
             (dict(order=3), "order"), (dict(n_iter=0), "n_iter"), (dict(n_iter=65), "n_iter"), (dict(na_=2050), "na must be"),
             (dict(na_=1), "na must be"), (dict(wavelet=9), "wavelet"), (dict(scales=bad_sc), "scales"),
             (dict(rcp=None), "NULL"), (dict(fp=_vp(bad_f)), "ssq_freqs_asc"), (dict(dt=0.0), "dt"), (dict(kind=3), "freq_kind"),
             (dict(kind=2, tr=1), "freq_transition"), (dict(pad=9), "padtype"), (dict(sq=2), "squeezing"),
             (dict(gamma=float("nan")), "gamma"), (dict(rho_=None), "NULL"), (dict(rho_=bad_rho_hi), "row_of_bin"),
             (dict(rho_=bad_rho_lo), "row_of_bin"), (dict(limit=16), "work_limit_bytes"))
    for kw, word in cases:
        assert host(**kw) != 0, kw
        msg = lib.ssq_last_error().decode()
        assert word in msg, (kw, msg)
        assert "mssq_cwt" in msg or word in ("NULL", "dtype"), (kw, msg)

    ws = lib.ssq_mssq_cwt_workspace_bytes(_lib.SSQ_F64, 1, N, na, C.byref(mn))

    def execute(order=2, n_iter=4, rho_=rho, wsb=ws, w=_vp(out), work=_vp(out)):
        return lib.ssq_mssq_cwt_exec(_lib.SSQ_F64, _vp(x), 1, N, 0, 3.0, 60.0, _vp(sc), na, 1.0, _vp(rc), _vp(f), 0, 0, 0, 0, -1.0,
                                     4, order, n_iter, _vp(rho_), _vp(out), _vp(out), w, None, None, work, wsb, None, None)

    # (a workspace that is too small is refused before any device work)
    for kw, word in ((dict(order=5), "order"), (dict(n_iter=-1), "n_iter"), (dict(rho_=bad_rho_hi), "row_of_bin"),
                     (dict(wsb=mn.value - 1), "workspace"), (dict(wsb=16), "workspace"), (dict(w=None), "NULL"),
                     (dict(work=None), "NULL")):
        assert execute(**kw) != 0, kw
        assert word in lib.ssq_last_error().decode(), kw

    w = np.ones((2, 9, 5))
    f9 = np.ascontiguousarray(f[:9])
    r9 = np.arange(9, dtype=np.int32)
    o_r, o_b, o_w = np.empty(w.shape, np.int32), np.empty(w.shape, np.int32), np.empty_like(w)

    def walk(dtype=_lib.SSQ_F64, wp=_vp(w), B=2, na_=9, n=5, fp=_vp(f9), kind=0, tr=0, rp=_vp(r9), n_iter=2, rows=_vp(o_r),
             bins=_vp(o_b), wn=_vp(o_w)):
        return lib.ssq_mssq_cwt_walk_host(dtype, wp, B, na_, n, fp, kind, tr, rp, n_iter, rows, bins, wn)

    bad_f9, bad_r9 = f9.copy(), r9.copy()
    bad_f9[2], bad_r9[8] = np.nan, 9
    for kw, word in ((dict(wp=None), "NULL"), (dict(fp=None), "NULL"), (dict(rp=None), "NULL"), (dict(rows=None), "NULL"),
                     (dict(bins=None), "NULL"), (dict(wn=None), "NULL"), (dict(dtype=3), "dtype"), (dict(B=0), "batch"),
                     (dict(na_=1), "na must be"), (dict(na_=2050), "na must be"), (dict(n=0), "n_cols"), (dict(n_iter=0), "n_iter"),
                     (dict(n_iter=65), "n_iter"), (dict(kind=7), "freq_kind"), (dict(kind=2, tr=9), "freq_transition"),
                     (dict(fp=_vp(bad_f9)), "ssq_freqs_asc"), (dict(rp=_vp(bad_r9)), "row_of_bin")):
        assert walk(**kw) != 0, kw
        assert word in lib.ssq_last_error().decode(), kw
