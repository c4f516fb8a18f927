"""CPU tests of the surface of `upstream.conceft_cwt`: every refusal is a ValueError raised before any GPU work, and the
C entry points validate their arguments on the host (no GPU call is reached)."""
import ctypes as C

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up

GMW = ("gmw", {"gamma": 3.0, "beta": 60.0})
X = np.cos(0.3 * np.arange(128))
SC = 4.0 * 2.0 ** (np.arange(16) / 4)


def _refused(match=None, **kw):
    args = dict(wavelet=GMW, scales=SC)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        up.conceft_cwt(X, **args)


def test_wavelet_refusals():
    _refused("GMW", wavelet="morlet")
    _refused("GMW", wavelet=("morlet", {"mu": 6.0}))
    _refused("bandpass", wavelet=("gmw", {"norm": "energy"}))
    _refused("bandpass", wavelet=("gmw", {"order": 1}))
    _refused("positive", wavelet=("gmw", {"gamma": -1.0}))


def test_orders_refusals():
    _refused("distinct", orders=(0, 1, 1))
    _refused("within", orders=(0, 17))
    _refused("within", orders=(-1, 0))
    _refused("orders", orders=9)
    _refused("orders", orders=0)
    _refused("orders", orders=tuple(range(9)))
    _refused("orders", orders=())
    _refused("ints", orders=(0, 1.5))
    _refused("orders", orders=True)
    _refused("orders", orders="3")


def test_draws_refusals():
    _refused("n_draws", n_draws=0)
    _refused("n_draws", n_draws=257)
    _refused("n_draws", n_draws=2.5)
    _refused("draws", vectors=np.ones((257, 3)))
    _refused("vectors", vectors=np.ones((4, 2)))                       # three orders by default
    _refused("vectors", vectors=np.ones(3))
    _refused("vectors", vectors=np.ones((0, 3)))
    _refused("zero vector", vectors=np.array([[1.0, 0, 0], [0, 0, 0]]))
    _refused("finite", vectors=np.array([[1.0, np.nan, 0]]))
    with pytest.raises(ValueError, match="draw 1 is the zero vector"):
        up.conceft_cwt(X, GMW, scales=SC, vectors=np.array([[1.0, 0, 0], [0, 0, 0]]))


def test_degenerate_draw_is_refused_by_name():
    adm = [up.gmw_adm_ssq(3.0, 60.0, k) for k in range(2)]
    good = [1.0, 0.0]
    bad = [adm[1], -adm[0]]                                              # c = C_1 C_0 - C_0 C_1 = 0
    with pytest.raises(ValueError, match="draw 2 is degenerate"):
        up.conceft_cwt(X, GMW, scales=SC, orders=2, vectors=np.array([good, good, bad]))
    with pytest.raises(ValueError, match="draw 0 is degenerate"):
        up._conceft_gauge(np.array([bad]), adm)
    # just above the floor of 1e-6 sum |r_j||C_kj| it is taken
    r, c = up._conceft_gauge(np.array([[adm[1], -adm[0] * (1 - 1e-4)]]), adm)
    assert c[0] > 0 and abs(np.linalg.norm(r[0]) - 1) < 1e-15


def test_other_refusals():
    _refused("sum", squeezing="lebesgue")
    _refused("sum", squeezing="abs")
    _refused("scales", scales="log")
    _refused("scales", scales="log-piecewise")
    _refused("scales", scales=np.array([4.0]))
    _refused("positive", scales=np.array([4.0, -8.0, 16.0]))
    _refused("padtype", padtype="mirror")
    _refused("maprange", maprange="energy")
    _refused("gamma", gamma=float("nan"))
    _refused("ssq_freqs", ssq_freqs=np.linspace(0.01, 0.5, 7))
    with pytest.raises(ValueError, match="samples"):
        up.conceft_cwt(np.ones(1), GMW, scales=SC)
    with pytest.raises(ValueError, match="32767"):
        up.conceft_cwt(np.cos(0.3 * np.arange(4096)), GMW, scales=4.0 * 2.0 ** (np.arange(4100) / 1000), orders=8)
    with pytest.raises(TypeError):
        up.conceft_cwt(list(X), GMW, scales=SC)


def test_admittance_arguments():
    for bad in ((0.0, 60.0, 0), (3.0, -1.0, 0), (3.0, 60.0, -1), (3.0, 60.0, 17), (float("inf"), 60.0, 0)):
        with pytest.raises(ValueError):
            up.gmw_adm_ssq(*bad)
    with pytest.raises(ValueError):
        up.conceft_vectors(0, 3, 0, [1.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        up.conceft_vectors(4, 9, 0, [1.0] * 9)
    with pytest.raises(ValueError):
        up.conceft_vectors(4, 3, 0, [1.0, 1.0])


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_workspace_bytes_on_the_host():
    lib = _lib.load()
    mn = C.c_int64(0)
    pref = lib.ssq_conceft_cwt_workspace_bytes(_lib.SSQ_F32, 5, 1000, 40, 3, C.byref(mn))
    assert mn.value == 2 * 3 * 40 * 1000 * 8 and pref == 5 * mn.value
    pref = lib.ssq_conceft_cwt_workspace_bytes(_lib.SSQ_F64, 100, 1 << 16, 128, 3, C.byref(mn))
    assert mn.value == 2 * 3 * 128 * (1 << 16) * 16 and pref == mn.value           # one signal is above 1 GiB / 2
    for bad in ((7, 1, 100, 10, 3), (_lib.SSQ_F32, 0, 100, 10, 3), (_lib.SSQ_F32, 1, 0, 10, 3), (_lib.SSQ_F32, 1, 100, 1, 3),
                (_lib.SSQ_F32, 1, 100, 10, 0), (_lib.SSQ_F32, 1, 100, 10, 9), (_lib.SSQ_F32, 1, 100, 5000, 8)):
        assert lib.ssq_conceft_cwt_workspace_bytes(*bad, None) == -1
        assert b"conceft_cwt" in lib.ssq_last_error()


def test_c_entry_points_validate_on_the_host():
    """Bad arguments return the library's error code with a message, before the device is looked for."""
    lib = _lib.load()
    N, na, J, M = 64, 8, 2, 3
    x = np.zeros(N)
    polys = np.ascontiguousarray(up.gmw_order_coefficients(3.0, 60.0, range(J), average=False))
    vec = np.ascontiguousarray(up.conceft_vectors(M, J, 0, [up.gmw_adm_ssq(3.0, 60.0, k) for k in range(J)]))
    s = 4.0 * 2.0 ** (np.arange(na) / 2)
    rc = np.full(na, np.log(2) / 2)
    f = np.geomspace(0.01, 0.5, na)
    Tx = np.zeros((na, N), dtype=np.complex128)

    def call(**kw):
        a = dict(dtype=_lib.SSQ_F64, x=_vp(x), batch=1, N=N, gg=3.0, gb=60.0, polys=_vp(polys), nc=polys.shape[1], J=J,
                 vec=_vp(vec), M=M, scale=1.0, s=_vp(s), na=na, dt=1.0, rc=_vp(rc), f=_vp(f), kind=0, idx=0, pad=0, gamma=-1.0,
                 variant=0, limit=0, Tx=_vp(Tx))
        a.update(kw)
        return lib.ssq_conceft_cwt_host(a["dtype"], a["x"], a["batch"], a["N"], a["gg"], a["gb"], a["polys"], a["nc"], a["J"],
                                        a["vec"], a["M"], a["scale"], a["s"], a["na"], a["dt"], a["rc"], a["f"], a["kind"],
                                        a["idx"], a["pad"], a["gamma"], a["variant"], a["limit"], a["Tx"], None, None)

    for kw, msg in ((dict(x=None), b"NULL"), (dict(Tx=None), b"NULL"), (dict(vec=None), b"NULL"), (dict(dtype=5), b"dtype"),
                    (dict(batch=0), b"batch"), (dict(J=9), b"n_orders"), (dict(M=0), b"n_draws"), (dict(M=257), b"n_draws"),
                    (dict(nc=18), b"n_coeffs"), (dict(gg=0.0), b"GMW"), (dict(dt=0.0), b"dt"), (dict(pad=5), b"padtype"),
                    (dict(gamma=float("nan")), b"gamma"), (dict(scale=0.0), b"scale"), (dict(kind=3), b"freq_kind"),
                    (dict(kind=2, idx=1), b"freq_transition"), (dict(limit=16), b"work_limit_bytes")):
        assert call(**kw) != 0, kw
        assert msg in lib.ssq_last_error(), (kw, lib.ssq_last_error())
    bad_s = s.copy()
    bad_s[3] = -1.0
    assert call(s=_vp(bad_s)) != 0 and b"scales" in lib.ssq_last_error()
    bad_v = vec.copy()
    bad_v[1, 0] = np.nan
    assert call(vec=_vp(bad_v)) != 0 and b"vectors" in lib.ssq_last_error()
