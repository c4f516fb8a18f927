"""The two doors of the five fp64 CWT map pipelines (csrc/cwt_maps64.h): `ssq_cwt2`, `mssq_cwt`, `reassign_cwt`, `tssq_cwt`
and `tmssq_cwt` each have a host entry point and a device entry point (`*_exec`) that run one pipe struct through
`pipe_host` / `pipe_exec` (csrc/dev_buffers.h).  Here both are called through the C ABI on the same signals and every plane
of the device door must equal the host's bit for bit (`np.array_equal`): on a workspace of exactly `min_bytes` (one row a
chunk) and of the preferred size (one chunk), on the NULL stream and on a stream of the caller's, with `kernel_ms` given,
the optional outputs given and left out, and with the guard bytes behind every device buffer untouched.

Shape: 3 different signals of 30 samples (P = 64), 8 GMW scales at 4 to the octave: 24 rows.  Each signal carries an
impulse, which moves time targets and gives the walks of `mssq_cwt` and `tmssq_cwt` something to do."""
import ctypes as C
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.test_gpu_grid_limits import FS, GMW, Door, _cdt, _code, _vp, base_signals, cwt_grids, cwt_scales

pytestmark = pytest.mark.gpu

B, N, NA, NV = 3, 30, 8, 4
SHAPE = (B, NA, N)
# name -> (the planes in the entry points' order: (kind c / r / i, optional on the host, optional on the device),
#          the floats of kernel_ms, the indices in kernel_ms of the parts reported beside "all the kernels" in [0])
DOORS = {
    "ssq_cwt2": ([("c", 0, 0), ("c", 0, 0), ("r", 1, 0)], 1, ()),
    "mssq_cwt": ([("c", 0, 0), ("c", 0, 0), ("r", 1, 0), ("i", 1, 1), ("i", 1, 1)], 3, ()),
    "reassign_cwt": ([("r", 0, 0), ("c", 0, 0), ("r", 1, 1), ("r", 1, 1), ("i", 1, 1), ("i", 1, 1)], 2, (1,)),
    "tssq_cwt": ([("c", 0, 0), ("c", 0, 0), ("r", 1, 1), ("i", 1, 1)], 3, (1, 2)),
    "tmssq_cwt": ([("c", 0, 0), ("c", 0, 0), ("r", 1, 1), ("i", 1, 1)], 4, (1, 2, 3)),
}
WALKED = {"mssq_cwt": 3, "tmssq_cwt": 3}            # the plane the walk writes: rows, mm
CASES = [("ssq_cwt2", 2, 1), ("mssq_cwt", 1, 1), ("mssq_cwt", 1, 3), ("mssq_cwt", 2, 1), ("mssq_cwt", 2, 3),
         ("reassign_cwt", 1, 1), ("tssq_cwt", 1, 1), ("tssq_cwt", 2, 1),
         ("tmssq_cwt", 1, 1), ("tmssq_cwt", 1, 3), ("tmssq_cwt", 2, 1), ("tmssq_cwt", 2, 3)]
CASE_IDS = ["%s-o%d-i%d" % c for c in CASES]
RDTS = pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])


@functools.lru_cache(maxsize=None)
def signals(rdt):
    """[3, 30], read-only: three different base signals and on each, at another sample, an impulse six times its largest
    sample."""
    X = base_signals(N)[:B].copy()
    for b, at in enumerate((7, 15, 22)):
        X[b, at] += 6.0 * np.abs(X[b]).max()
    X = X.astype(rdt)
    X.setflags(write=False)
    return X


def _dtype(kind, rdt):
    return {"c": _cdt(rdt), "r": rdt, "i": np.int32}[kind]


def _arguments(name, order, n_iter, code, x):
    """-> (the arguments up to the outputs without the host's work_limit_bytes, where the limit goes among them, the arrays
    they point into)."""
    s, rowc, f, kind, f_idx = cwt_grids(NA, NV, N)
    wcode, p0, p1 = up._wavelet(GMW)
    head = (code, x, B, N, wcode, p0, p1)
    if name in ("ssq_cwt2", "mssq_cwt"):
        pre = head + (_vp(s), NA, 1 / FS, _vp(rowc), _vp(f), up.FREQS[kind], f_idx or 0, 0, 0, -1.0, up.VARIANT_FLIPUD)
        rho = np.ascontiguousarray(up.mssq_cwt_row_of_bin(GMW, s, f, fs=FS), dtype=np.int32)
        extra = (order, n_iter, _vp(rho)) if name == "mssq_cwt" else ()
        return pre + extra, len(pre), (s, rowc, f, rho)
    if name == "reassign_cwt":
        pre = head + (_vp(s), NA, 1 / FS, _vp(f), up.FREQS[kind], f_idx or 0, 0, -1.0, up.VARIANT_FLIPUD)
        return pre, len(pre), (s, f)
    nu = up.tssq_cwt_row_freqs(GMW, s)
    pre = head + (_vp(s), _vp(nu), NA, 1 / FS, 0, order, -1.0) + ((n_iter,) if name == "tmssq_cwt" else ())
    return pre, len(pre), (s, nu)


def work_bytes(name, order, rdt):
    """(min_bytes, the preferred size) of the device door's workspace"""
    lib, mn = _lib.load(), C.c_int64(0)
    fn = getattr(lib, "ssq_%s_workspace_bytes" % name)
    args = (_code(rdt), B, N, NA) + ((order,) if name in ("tssq_cwt", "tmssq_cwt") else ())
    pref = int(fn(*args, C.byref(mn)))
    assert 0 < mn.value < pref
    return mn.value, pref


@functools.lru_cache(maxsize=None)
def host(name, order, n_iter, rdt, give=True, limit=0):
    """The planes of the host entry point (None: an optional one that was left out); every one pre-filled."""
    X = signals(rdt)
    args, at, keep = _arguments(name, order, n_iter, _code(rdt), _vp(X))
    planes = []
    for kind, optional, _ in DOORS[name][0]:
        a = np.full(SHAPE, -7 if kind == "i" else np.nan, dtype=_dtype(kind, rdt))
        planes.append(a if give or not optional else None)
    fn = getattr(_lib.load(), "ssq_%s_host" % name)
    _lib.check(fn(*args[:at], limit, *args[at:], *[_vp(a) for a in planes]))
    for a in planes:
        if a is not None:
            assert a.dtype != np.int32 or not (a == -7).any(), "an int32 plane of %s keeps its pre-fill" % name
            a.setflags(write=False)
    return planes


def device(name, order, n_iter, rdt, ws, stream=False, give=True, ms_len=None):
    """The planes of the device entry point on a workspace of `ws` bytes, and kernel_ms (ms_len floats, pre-filled with NaN;
    None: kernel_ms is not given)."""
    lib = _lib.load()
    X = signals(rdt)
    ms = None if ms_len is None else np.full(ms_len, np.nan, dtype=np.float32)
    st = C.c_void_p()
    if stream:
        _lib.check(lib.ssq_stream_create(C.byref(st)))
    try:
        with Door() as d:
            dx, dws = d.buf(X.nbytes, X), d.buf(ws)
            args, _, keep = _arguments(name, order, n_iter, _code(rdt), dx.p)
            bufs = [d.buf(B * NA * N * np.dtype(_dtype(kind, rdt)).itemsize) if give or not optional else None
                    for kind, _, optional in DOORS[name][0]]
            fn = getattr(lib, "ssq_%s_exec" % name)
            _lib.check(fn(*args, *[b.p if b else None for b in bufs], dws.p, ws, st if stream else None,
                          None if ms is None else ms.ctypes.data_as(C.POINTER(C.c_float))))
            planes = [b.get(SHAPE, _dtype(kind, rdt)) if b else None for b, (kind, _, _) in zip(bufs, DOORS[name][0])]
    finally:
        if stream:
            lib.ssq_stream_destroy(st)
    return planes, ms


def assert_planes_equal(got, want, what):
    assert len(got) == len(want)
    for k, (a, w) in enumerate(zip(got, want)):
        if a is None or w is None:
            continue
        assert a.dtype == w.dtype and a.shape == w.shape, (what, k)
        assert np.array_equal(a, w, equal_nan=a.dtype.kind in "fc"), "%s: plane %d differs" % (what, k)


@RDTS
@pytest.mark.parametrize("name,order,n_iter", CASES, ids=CASE_IDS)
def test_device_door_equals_the_host_call(name, order, n_iter, rdt):
    """Every optional output given, kernel_ms given: min_bytes and the preferred size, the NULL stream and a stream of the
    caller's; then the host again under work_limit_bytes = min_bytes.  The first GPU run of ssq_mssq_cwt_exec and
    ssq_tmssq_cwt_exec.  Where there is a walk, the host's walked plane at n_iter = 3 must differ from n_iter = 1's in a
    kept cell: the walk does something on these signals."""
    want = host(name, order, n_iter, rdt)
    mn, pref = work_bytes(name, order, rdt)
    for ws in (mn, pref):
        for stream in (False, True):
            got, ms = device(name, order, n_iter, rdt, ws, stream=stream, ms_len=DOORS[name][1])
            assert_planes_equal(got, want, "%s, workspace %d, stream %s" % (name, ws, stream))
            assert np.isfinite(ms).all()
    assert_planes_equal(host(name, order, n_iter, rdt, limit=mn), want, "%s, work_limit_bytes = min_bytes" % name)
    if n_iter > 1:
        one, walked = host(name, order, 1, rdt)[WALKED[name]], want[WALKED[name]]
        assert ((one >= 0) & (walked != one)).any(), "the walk of %s moves nothing on these signals" % name


@RDTS
@pytest.mark.parametrize("name,order,n_iter", CASES, ids=CASE_IDS)
def test_optional_outputs_left_out(name, order, n_iter, rdt):
    """Both doors with every optional output NULL: Tx (or Rx) and Wx equal the run that was given them."""
    want = host(name, order, n_iter, rdt)
    bare = host(name, order, n_iter, rdt, give=False)
    assert bare[0] is not None and bare[1] is not None and any(a is None for a in bare)
    assert_planes_equal(bare[:2], want[:2], name + " host")
    got, _ = device(name, order, n_iter, rdt, work_bytes(name, order, rdt)[1], give=False)
    assert got[0] is not None and got[1] is not None
    assert_planes_equal(got[:2], want[:2], name + " exec")


@pytest.mark.parametrize("name", list(DOORS))
def test_kernel_ms_layout(name):
    """The documented count of floats (include/ssq_hip.h: ONE, THREE, TWO, THREE, FOUR): two floats more stay NaN; every
    float is finite and >= 0; "all the kernels" is at least each part reported beside it.  No magnitudes."""
    planes, count, parts = DOORS[name]
    _, ms = device(name, 2, 3, np.float64, work_bytes(name, 2, np.float64)[1], ms_len=count + 2)
    assert np.isnan(ms[count:]).all()
    assert np.isfinite(ms[:count]).all() and (ms[:count] >= 0).all()
    for k in parts:
        assert ms[0] >= ms[k], (name, k, ms)
