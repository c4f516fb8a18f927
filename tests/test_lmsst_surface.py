"""CPU tests of the surface of `upstream.lmssq_stft`, `upstream.lmssq_cwt` and `upstream.lmsst_rows`: the signatures, every
refusal before the GPU is asked for, and the C entry points exported, declared with the header's arity, sizing their
workspace and refusing bad arguments on the host."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up

E = inspect.Parameter.empty
NEW = ("ssq_lmssq_stft_host", "ssq_lmssq_stft_workspace_bytes", "ssq_lmssq_stft_exec", "ssq_lmssq_cwt_host",
       "ssq_lmssq_cwt_workspace_bytes", "ssq_lmssq_cwt_exec", "ssq_lmsst_rows_host")
SCALES = 4.0 * 2 ** (np.arange(24) / 8.0)


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
    sig = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]     # noqa: E731
    assert sig(up.lmssq_stft) == [("x", E), ("window", None), ("n_fft", None), ("win_len", None), ("hop_len", 1),
                                  ("fs", None), ("t", None), ("modulated", True), ("padtype", "reflect"),
                                  ("squeezing", "sum"), ("gamma", None), ("flipud", False), ("delta", None),
                                  ("get_bins", False)]
    assert sig(up.lmssq_cwt) == [("x", E), ("wavelet", "gmw"), ("scales", "log-piecewise"), ("nv", None), ("fs", None),
                                 ("t", None), ("ssq_freqs", None), ("padtype", "reflect"), ("squeezing", "sum"),
                                 ("maprange", "peak"), ("gamma", None), ("flipud", True), ("delta", None),
                                 ("get_w", False), ("get_rows", False)]
    assert sig(up.lmsst_rows) == [("A", E), ("delta", E)]
    assert sig(up.lmsst_default_delta) == [("window", E), ("n_fft", E)]
    assert sig(up.lmssq_cwt_default_delta) == [("wavelet", E), ("scales", E)]


def test_docstrings_state_the_definition():
    assert "`lmssq_stft`" in up.__doc__ and "`lmssq_cwt`" in up.__doc__ and "`lmsst_rows`" in up.__doc__
    for word in ("re^2 + im^2", "strictly greater", "lowest row wins a tie", "rows that are not kept take part",
                 "|V| > gamma", "F - 1 - b", "lmsst_default_delta", "bound on work", "not a measurement", "issq_stft",
                 "SPECTROGRAM's ridge", "power of two", "spill", "ONE transform"):
        assert word in up.lmssq_stft.__doc__, word
    for word in ("re^2 + im^2", "strictly greater", "lowest row wins a tie", "|W| < gamma", "nu_hz[m[i]]", "+inf",
                 "ssqueeze(Wx, w", "na - 1 - m[i]", "lmssq_cwt_default_delta", "bound on work", "not a measurement",
                 "bit for bit", "2 .. 2049", "spill", "ONE\n    inverse transform"):
        assert word in up.lmssq_cwt.__doc__, word
    for word in ("strictly greater", "no keep rule", "widened", "ValueError"):
        assert word in up.lmsst_rows.__doc__, word
    for fn in (up.lmsst_default_delta, up.lmssq_cwt_default_delta):
        assert "1e-3" in fn.__doc__ and "part of the definition, not a measurement" in fn.__doc__.replace("\n    ", " ")


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


# ------------------------------------------------------------------------------------------------------- lmssq_stft
@pytest.mark.parametrize("n_fft", [0, 8, 24, 8192])
def test_n_fft_refusals_come_before_the_gpu(no_gpu, n_fft):
    x = np.random.default_rng(0).standard_normal(9000)
    if n_fft == 0:                                               # 0 asks for the default, min(N // hop_len, 512): 100 here
        x, n_fft = x[:100], None
    with pytest.raises(ValueError, match="n_fft"):
        up.lmssq_stft(x, np.hanning(8), n_fft=n_fft)


@pytest.mark.parametrize("delta", [0, -1, 9, 1000, True, 2.0, np.float64(3), "3"])
def test_stft_delta_refusals_come_before_the_gpu(no_gpu, delta):
    with pytest.raises(ValueError, match="delta"):
        up.lmssq_stft(np.zeros(300), np.hanning(16), n_fft=16, delta=delta)       # F = 9: 1 .. 8


def test_stft_delta_is_capped_at_256(no_gpu):
    with pytest.raises(ValueError, match="delta"):
        up.lmssq_stft(np.zeros(300), np.hanning(16), n_fft=1024, delta=257)
    with pytest.raises(_Reached):
        up.lmssq_stft(np.zeros(300), np.hanning(16), n_fft=1024, delta=256)


def test_stft_other_refusals_come_before_the_gpu(no_gpu):
    x = np.random.default_rng(1).standard_normal(300)
    win = np.hanning(16)
    with pytest.raises(ValueError, match="padtype"):
        up.lmssq_stft(x, win, n_fft=16, padtype="foo")
    with pytest.raises(ValueError, match="window"):
        up.lmssq_stft(x, None, n_fft=16)
    with pytest.raises(ValueError, match="window"):
        up.lmssq_stft(x, "hann", n_fft=16)
    with pytest.raises(ValueError, match="squeezing"):
        up.lmssq_stft(x, win, n_fft=16, squeezing="abs")
    with pytest.raises(TypeError):
        up.lmssq_stft(np.zeros((2, 3, 40)), win, n_fft=16)


@pytest.mark.parametrize("kw", [dict(), dict(delta=1, get_bins=True, flipud=True),
                                dict(padtype="wrap", squeezing="lebesgue", modulated=False, hop_len=3, fs=2.0, gamma=1e-6)])
@pytest.mark.parametrize("shape,dtype", [((300,), np.float64), ((2, 300), np.float32)])
def test_well_formed_stft_calls_reach_the_gpu(no_gpu, kw, shape, dtype):
    x = np.random.default_rng(2).standard_normal(shape).astype(dtype)
    for n_fft in (16, 64, 4096):
        with pytest.raises(_Reached):
            up.lmssq_stft(x, np.hanning(16), n_fft=n_fft, **kw)


def test_stft_workspace_bytes():
    """0 for float64, the widened signals (batch N 8 bytes, no padding) for float32, -1 on a refused shape."""
    lib = _lib.load()
    err = lambda: lib.ssq_last_error().decode()                                      # noqa: E731
    for batch, N, n_fft, hop in ((1, 40, 64, 1), (3, 1000, 64, 7), (70000, 16, 16, 1), (2, 5000, 4096, 64)):
        assert lib.ssq_lmssq_stft_workspace_bytes(_lib.SSQ_F64, batch, N, n_fft, hop) == 0
        assert lib.ssq_lmssq_stft_workspace_bytes(_lib.SSQ_F32, batch, N, n_fft, hop) == 8 * batch * N
    for code in (_lib.SSQ_F32, _lib.SSQ_F64):
        for n_fft in (0, 8, 24, 8192):
            assert lib.ssq_lmssq_stft_workspace_bytes(code, 1, 1000, n_fft, 1) == -1 and "n_fft" in err()
        assert lib.ssq_lmssq_stft_workspace_bytes(code, 0, 1000, 64, 1) == -1 and "batch" in err()
        assert lib.ssq_lmssq_stft_workspace_bytes(code, 1, 1000, 64, 0) == -1 and "hop" in err()
        assert lib.ssq_lmssq_stft_workspace_bytes(code, 1, 0, 64, 1) == -1 and "n_signal" in err()
    assert lib.ssq_lmssq_stft_workspace_bytes(7, 1, 1000, 64, 1) == -1 and "dtype" in err()


def test_stft_c_entry_points_refuse_on_the_host():
    lib = _lib.load()
    err = lambda: lib.ssq_last_error().decode()                                      # noqa: E731
    x = np.zeros(100)
    x32 = np.zeros(100, dtype=np.float32)
    win = np.ones(24)
    out = np.zeros((13, 100), dtype=np.complex128)

    def host(n_fft=16, hop=1, fs=1.0, pad=0, sq=0, delta=2, x_=x, Tx=out):
        return lib.ssq_lmssq_stft_host(_lib.SSQ_F64, None if x_ is None else _vp(x_), 1, 100, _vp(win), n_fft, hop, fs, pad,
                                       sq, -1.0, 3, delta, None if Tx is None else _vp(Tx), None, _vp(out), None)

    def execute(n_fft=16, sq=0, delta=2, code=_lib.SSQ_F64, ws=0, work=None):
        xin = x if code == _lib.SSQ_F64 else x32
        return lib.ssq_lmssq_stft_exec(code, _vp(xin), 1, 100, _vp(win), n_fft, 1, 1.0, 0, sq, -1.0, 3, delta, _vp(out),
                                       _vp(out), None, work, ws, None)
    for call in (host, execute):
        assert call(n_fft=24) != 0 and "n_fft" in err()
        for delta in (0, -3, 9, 300):
            assert call(delta=delta) != 0 and "delta" in err()
        assert call(sq=7) != 0 and "squeezing" in err()
    assert host(pad=9) != 0 and "padtype" in err()
    assert host(fs=0.0) != 0 and "fs" in err()
    assert host(hop=0) != 0 and "hop" in err()
    assert host(x_=None) != 0 and "NULL" in err()
    assert host(Tx=None) != 0 and "NULL" in err()
    assert execute(code=_lib.SSQ_F32, ws=8 * 100 - 1, work=_vp(out)) != 0 and "workspace" in err()
    assert execute(code=_lib.SSQ_F32, ws=8 * 100, work=None) != 0 and "NULL" in err()
    if _lib.device_count() < 1:
        assert host() != 0 and "no HIP device" in err()
        assert execute() != 0 and "no HIP device" in err()


# -------------------------------------------------------------------------------------------------------- lmssq_cwt
@pytest.mark.parametrize("delta", [0, -1, 24, 1000, True, 2.0, "3"])
def test_cwt_delta_refusals_come_before_the_gpu(no_gpu, delta):
    with pytest.raises(ValueError, match="delta"):
        up.lmssq_cwt(np.zeros(300), "gmw", SCALES, delta=delta)                   # na = 24: 1 .. 23


def test_cwt_other_refusals_come_before_the_gpu(no_gpu):
    x = np.random.default_rng(1).standard_normal(300)
    with pytest.raises(ValueError, match="padtype"):
        up.lmssq_cwt(x, "gmw", SCALES, padtype="foo")
    with pytest.raises(ValueError, match="squeezing"):
        up.lmssq_cwt(x, "gmw", SCALES, squeezing="abs")
    with pytest.raises(ValueError):
        up.lmssq_cwt(x, "bump", SCALES)                                           # wavelet
    with pytest.raises(ValueError, match="order"):
        up.lmssq_cwt(x, ("gmw", {"order": 1}), SCALES)
    with pytest.raises(ValueError, match="scales"):
        up.lmssq_cwt(x, "gmw", "log")                                             # the string forms are not accepted
    with pytest.raises(ValueError, match="scales"):
        up.lmssq_cwt(x, "gmw", np.array([1.0, -2.0, 4.0]))
    with pytest.raises(ValueError, match="scales"):
        up.lmssq_cwt(x, "gmw", 4.0 * 2 ** (np.arange(2050) / 1024.0))             # 2 .. 2049 rows
    with pytest.raises(ValueError, match="gamma"):
        up.lmssq_cwt(x, "gmw", SCALES, gamma=float("nan"))
    with pytest.raises(ValueError):
        up.lmssq_cwt(np.zeros(1), "gmw", SCALES)
    with pytest.raises(TypeError):
        up.lmssq_cwt(list(x), "gmw", SCALES)


@pytest.mark.parametrize("kw", [dict(), dict(delta=1, get_w=True, get_rows=True, flipud=False),
                                dict(wavelet="morlet", padtype="wrap", squeezing="lebesgue", fs=2.0, gamma=1e-6, delta=23)])
@pytest.mark.parametrize("shape,dtype", [((300,), np.float64), ((2, 300), np.float32)])
def test_well_formed_cwt_calls_reach_the_gpu(no_gpu, kw, shape, dtype):
    x = np.random.default_rng(2).standard_normal(shape).astype(dtype)
    kw = dict(kw)
    with pytest.raises(_Reached):
        up.lmssq_cwt(x, kw.pop("wavelet", "gmw"), SCALES, **kw)
    x1 = np.zeros(1024, dtype=dtype)
    with pytest.raises(_Reached):
        up.lmssq_cwt(x1, "gmw", up.process_scales("log-piecewise", 1024, "gmw"))


def test_cwt_workspace_bytes():
    """One map a row: 16 P (batch + 2 R) bytes, a fifth of ssq_cwt2's chunk area; -1 on a refused shape."""
    lib = _lib.load()
    err = lambda: lib.ssq_last_error().decode()                                      # noqa: E731
    mn, mn2 = C.c_int64(0), C.c_int64(0)
    for code in (_lib.SSQ_F32, _lib.SSQ_F64):
        for batch, N, na in ((1, 300, 2), (3, 700, 48), (2, 1024, 2049)):
            P = up.p2up(N)[0]
            pref = lib.ssq_lmssq_cwt_workspace_bytes(code, batch, N, na, C.byref(mn))
            assert mn.value == 16 * P * (batch + 2)
            assert pref == 16 * P * (batch + 2 * batch * na)
            pref2 = lib.ssq_ssq_cwt2_workspace_bytes(code, batch, N, na, C.byref(mn2))
            assert pref2 - 16 * P * batch == 5 * (pref - 16 * P * batch)
        assert lib.ssq_lmssq_cwt_workspace_bytes(code, 1, 300, 1, None) == -1 and "na" in err()
        assert lib.ssq_lmssq_cwt_workspace_bytes(code, 1, 300, 2050, None) == -1 and "na" in err()
        assert lib.ssq_lmssq_cwt_workspace_bytes(code, 0, 300, 8, None) == -1 and "batch" in err()
        assert lib.ssq_lmssq_cwt_workspace_bytes(code, 1, 1, 8, None) == -1 and "n_signal" in err()
    assert lib.ssq_lmssq_cwt_workspace_bytes(7, 1, 300, 8, None) == -1 and "dtype" in err()


def test_cwt_c_entry_points_refuse_on_the_host():
    lib = _lib.load()
    err = lambda: lib.ssq_last_error().decode()                                      # noqa: E731
    N, na = 100, 8
    x = np.zeros(N)
    s = np.ascontiguousarray(4.0 * 2 ** (np.arange(na) / 4.0))
    rc = np.ones(na)
    f_asc = np.ascontiguousarray(np.linspace(0.01, 0.4, na))
    nu = np.ascontiguousarray(1.0 / s)
    out = np.zeros((na, N), dtype=np.complex128)
    w = np.zeros((na, N))

    def host(na_=na, delta=2, dt=1.0, pad=0, sq=0, gamma=-1.0, limit=0, nu_=nu, s_=s, Tx=out):
        return lib.ssq_lmssq_cwt_host(_lib.SSQ_F64, _vp(x), 1, N, 0, 3.0, 60.0, _vp(s_), na_, dt, _vp(rc), _vp(f_asc), 1, 0,
                                      pad, sq, gamma, 0, limit, delta, None if nu_ is None else _vp(nu_),
                                      None if Tx is None else _vp(Tx), _vp(out), None, None)

    def execute(na_=na, delta=2, dt=1.0, pad=0, sq=0, gamma=-1.0, nu_=nu, s_=s, ws=1 << 30):
        return lib.ssq_lmssq_cwt_exec(_lib.SSQ_F64, _vp(x), 1, N, 0, 3.0, 60.0, _vp(s_), na_, dt, _vp(rc), _vp(f_asc), 1, 0,
                                      pad, sq, gamma, 0, delta, None if nu_ is None else _vp(nu_), _vp(out), _vp(out), _vp(w),
                                      None, _vp(out), ws, None, None)
    for call in (host, execute):
        for delta in (0, -1, 8, 300):
            assert call(delta=delta) != 0 and "delta" in err()
        assert call(na_=1) != 0 and "na" in err()
        assert call(na_=2050) != 0 and "na" in err()
        assert call(dt=0.0) != 0 and "dt" in err()
        assert call(pad=9) != 0 and "padtype" in err()
        assert call(sq=7) != 0 and "squeezing" in err()
        assert call(gamma=float("nan")) != 0 and "gamma" in err()
        assert call(nu_=None) != 0 and "NULL" in err()
        assert call(nu_=np.zeros(na)) != 0 and "row_freqs_hz" in err()
        assert call(s_=-s) != 0 and "scales" in err()
    assert host(Tx=None) != 0 and "NULL" in err()
    assert host(limit=100) != 0 and "work_limit_bytes" in err()
    assert execute(ws=16 * up.p2up(N)[0] * 3 - 1) != 0 and "workspace" in err()      # min_bytes = 16 P (batch + 2)
    if _lib.device_count() < 1:
        assert host() != 0 and "no HIP device" in err()
        assert execute() != 0 and "no HIP device" in err()


# ------------------------------------------------------------------------------------------------------- lmsst_rows
def test_rows_refusals_come_before_the_gpu(no_gpu):
    A = np.random.default_rng(3).random((9, 20))
    for delta in (0, 9, 300, True, 1.0, None, "2"):
        with pytest.raises(ValueError, match="delta"):
            up.lmsst_rows(A, delta)
    for bad in (A.astype(np.int32), A.astype(np.complex128), A[0], A[None, None], list(A), np.zeros((1, 20)),
                np.zeros((2050, 3)), np.zeros((9, 0)), np.zeros((0, 9, 4))):
        with pytest.raises(ValueError):
            up.lmsst_rows(bad, 1)
    for good, delta in ((A, 1), (A, 8), (A.astype(np.float32), 3), (np.stack([A, A]), 2), (np.zeros((2049, 3)), 256),
                        (np.zeros((2, 5)), 1)):
        with pytest.raises(_Reached):
            up.lmsst_rows(good, delta)


def test_rows_c_entry_point_refuses_on_the_host():
    lib = _lib.load()
    err = lambda: lib.ssq_last_error().decode()                                      # noqa: E731
    A = np.zeros((9, 20))
    out = np.zeros((9, 20), dtype=np.int32)
    call = lambda dtype=_lib.SSQ_F64, B=1, R=9, n=20, delta=2, A_=A: lib.ssq_lmsst_rows_host(     # noqa: E731
        dtype, None if A_ is None else _vp(A_), B, R, n, delta, _vp(out))
    assert call(dtype=7) != 0 and "dtype" in err()
    assert call(B=0) != 0 and "batch" in err()
    assert call(R=1) != 0 and "n_rows" in err()
    assert call(R=2050) != 0 and "n_rows" in err()
    assert call(n=0) != 0 and "n_cols" in err()
    for delta in (0, 9, 257):
        assert call(delta=delta) != 0 and "delta" in err()
    assert call(A_=None) != 0 and "NULL" in err()
    if _lib.device_count() < 1:
        assert call() != 0 and "no HIP device" in err()
