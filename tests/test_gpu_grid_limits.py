"""Every transform past the 65535 limit of a HIP grid's y and z dimensions.

Almost every kernel family puts "signal" or "signal x scale row" on grid.y or grid.z and crosses 65535 in its own way: a
host loop of launches over slices of 65535 signals, a capped grid whose blocks stride, a host slice of the batch, or a
refusal.  No other module has a batch, a row count or a plane count above a few hundred, so the second iteration of those
loops, every stride and every offset that goes with them run here alone.

The method is the same for every transform.  K = 7 base signals (two tones, a chirp and seeded noise; signal 3 is 37 times
larger, so that per-signal maxima differ) are repeated into a batch of B = 65535 + 8 signals, X[b] = base[b % 7].  Since
65535 = 1 and 65536 = 2 (mod 7), a kernel that confuses signal b with b +- 65535 or b +- 65536 reads ANOTHER base signal.
  1. every output plane of X[b] equals, bit for bit, that of base[b % 7] from a call on the 7 signals alone (one reshaped
     comparison over all B signals);
  2. the 7-signal result is held to the transform's NumPy model or oracle by the comparisons and tolerances of the
     transform's own test module (imported where they are functions; where they are expressions inside a test they are
     restated next to the name of that test);
  3. where the transform has a device entry point, the big batch also goes through it on buffers from `ssq_dev_malloc`,
     with a workspace of exactly the size its query reports and 4096 bytes of 0xA5 behind the workspace and behind every
     output, in the same allocation: the guards stay untouched and the outputs equal the host call's bit for bit.

One row-stride case uses another repetition than b % 7: see `CWT_SHAPES`."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import ssq_oracle as o
from oracle import upstream_oracle as u
from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.helpers import components_ref as cr
from tests.helpers import conceft_ref as cf
from tests.helpers import cwt_sst2_ref as c2
from tests.helpers import msst_ref as ms
from tests.helpers import reassign_cwt_ref as rc2
from tests.helpers import reassign_ref as rs
from tests.helpers import ridge_oracle as ro
from tests.helpers import ssqueeze_ref as sq
from tests.helpers import sst2_ref as s2
from tests.helpers import tssq_cwt_ref as tc
from tests.helpers import tsst_ref as ts

pytestmark = pytest.mark.gpu

K = 7
LIMIT = 65535                           # a HIP grid's y and z dimensions stop here
B_BIG = LIMIT + 8
# with K a divisor of 65535 (3, 5, 17, 257) or of 65536 the aliasing this module looks for would be invisible
assert LIMIT % K != 0 and (LIMIT + 1) % K != 0
GUARD = 4096
FS = 2.0                                # (the FS of tests/test_gpu_sst2.py and test_gpu_msst.py, whose helpers take it from there)
GMW = ("gmw", {"gamma": 3.0, "beta": 60.0})
S0 = c2.gmw_wc(3.0, 60.0) / np.pi       # the scale whose peak sits at Nyquist
EPS64 = float(np.finfo(np.float64).eps)
RDTS = pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])


# ------------------------------------------------------------------------------------------------------- the batches ----
@functools.lru_cache(maxsize=None)
def base_signals(N):
    """[K, N] float64, read-only: two tones, a linear chirp and seeded noise, all different; signal 3 times 37."""
    t = np.arange(N, dtype=np.float64)
    X = np.empty((K, N))
    for s in range(K):
        chirp, _ = s2.chirp(N, 0.08 + 0.01 * s, 0.38 - 0.02 * s)
        X[s] = (np.cos(2 * np.pi * (0.06 + 0.03 * s) * t) + 0.6 * np.cos(2 * np.pi * (0.43 - 0.02 * s) * t + 0.3 * s)
                + 0.8 * chirp + 0.05 * np.random.default_rng(100 + s).standard_normal(N))
    X[3] *= 37.0
    X.setflags(write=False)
    return X


def plain_index(B):
    return np.arange(B) % K


def tile(base, idx):
    return np.ascontiguousarray(base[idx])


def _bits_equal(a, b):
    """Elementwise: equal, or NaN in both (as tests/test_gpu_ridges.py::_same_bits treats NaN)."""
    if a.dtype.kind == "c":
        a, b = a.view(a.real.dtype), b.view(b.real.dtype)
    eq = a == b
    if a.dtype.kind == "f":
        eq |= np.isnan(a) & np.isnan(b)
    return eq


def assert_repeats(big, base, idx, what):
    """Every plane big[b] is base[idx[b]], in one comparison over the whole batch."""
    assert big.dtype == base.dtype and big.shape == (len(idx),) + base.shape[1:], what
    ok = _bits_equal(big, base[idx]).reshape(len(idx), -1).all(axis=1)
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, "%s: %d signals differ from their base signal, the first at b = %s" % (what, bad.size, bad[:8])


def assert_same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    ok = _bits_equal(a, b).reshape(a.shape[0], -1).all(axis=1)
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, "%s: %d signals differ, the first at b = %s" % (what, bad.size, bad[:8])


def _code(rdt):
    return _lib.SSQ_F32 if np.dtype(rdt) == np.float32 else _lib.SSQ_F64


def _cdt(rdt):
    return np.complex64 if np.dtype(rdt) == np.float32 else np.complex128


def _eps(rdt):
    return float(np.finfo(rdt).eps)


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def strong(V):
    return np.abs(V) >= 1e-2 * np.abs(V).max()


# --------------------------------------------------------------------------------------------------- the device door ----
class DevBuf:
    """`nbytes` of device memory from `ssq_dev_malloc` followed, in the same allocation, by GUARD bytes of 0xA5."""

    def __init__(self, nbytes, src=None):
        self.lib = _lib.load()
        self.n = int(nbytes)
        self.p = C.c_void_p()
        _lib.check(self.lib.ssq_dev_malloc(C.byref(self.p), self.n + GUARD))
        _lib.check(self.lib.ssq_dev_memset(self.p, 0xA5, self.n + GUARD, None))
        if src is not None:
            assert src.nbytes == self.n and src.flags.c_contiguous
            _lib.check(self.lib.ssq_memcpy_h2d(self.p, _vp(src), src.nbytes, None))
        _lib.check(self.lib.ssq_device_sync())

    def get(self, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes == self.n
        _lib.check(self.lib.ssq_memcpy_d2h(_vp(out), self.p, out.nbytes, None))
        _lib.check(self.lib.ssq_device_sync())
        return out

    def guard_untouched(self):
        g = np.empty(GUARD, dtype=np.uint8)
        _lib.check(self.lib.ssq_memcpy_d2h(_vp(g), C.c_void_p(self.p.value + self.n), GUARD, None))
        _lib.check(self.lib.ssq_device_sync())
        return bool((g == 0xA5).all())

    def free(self):
        if self.p:
            self.lib.ssq_dev_free(self.p)
            self.p = C.c_void_p()


class Door:
    """The buffers of one device call; on leaving, every guard must be as it was filled."""

    def __init__(self):
        self.bufs = []

    def buf(self, nbytes, src=None):
        self.bufs.append(DevBuf(nbytes, src))
        return self.bufs[-1]

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        try:
            if exc_type is None:
                _lib.check(_lib.load().ssq_device_sync())
                touched = [i for i, b in enumerate(self.bufs) if not b.guard_untouched()]
                assert not touched, "the guard behind buffer(s) %s was written" % touched
        finally:
            for b in self.bufs:
                b.free()
        return False


# ============================================================================= the second-order STFT family ============
N_ST, NFFT, HOP = 32, 16, 8             # n_fft = 16 is the smallest the family accepts: 9 x 4 cells a signal
F_ST, NFR_ST = NFFT // 2 + 1, (N_ST - 1) // HOP + 1
STFT_RUNS = [("sst2", 2), ("msst", 1), ("msst", 2), ("tsst", 1), ("tsst", 2), ("reassign", 1)]
STFT_IDS = ["ssq_stft2", "mssq_stft-o1", "mssq_stft-o2", "tssq_stft-o1", "tssq_stft-o2", "reassign_stft"]
MSST_ITER = 3
# 'reflect' for both dtypes, and one more run with 'wrap' (on the float32 path, which also carries the widened signals)
STFT_PADS = [(np.float64, "reflect"), (np.float32, "reflect"), (np.float32, "wrap")]
STFT_PAD_IDS = ["f64-reflect", "f32-reflect", "f32-wrap"]


def gwin():
    return s2.gauss_window(NFFT, 2.5)


@functools.lru_cache(maxsize=None)
def gwin_tables():
    """(g, g1, g2, tg, tg1) as the library builds them on the host: what the models of the family run on."""
    from tests.test_gpu_sst2 import lib_tables
    return lib_tables(gwin())


def stft_host(name, order, X, pad):
    """The planes of the host entry point: the result, Sx and every map or target the call can return."""
    kw = dict(n_fft=NFFT, hop_len=HOP, fs=FS, padtype=pad)
    if name == "sst2":
        out = up.ssq_stft2(X, gwin(), get_w=True, **kw)
        return [out[0], out[1], out[4]]
    if name == "msst":
        out = up.mssq_stft(X, gwin(), order=order, n_iter=MSST_ITER, get_w=True, get_bins=True, **kw)
        return [out[0], out[1], out[4], out[5]]
    if name == "tsst":
        out = up.tssq_stft(X, gwin(), order=order, get_tau=True, **kw)
        return [out[0], out[1], out[4]]
    out = up.reassign_stft(X, gwin(), get_w=True, get_tau=True, **kw)
    return [out[0], out[1], out[4], out[5]]


def stft_exec(name, order, X, pad):
    """The same planes through the device entry point, workspace of exactly `*_workspace_bytes`, guards everywhere."""
    lib = _lib.load()
    rdt = X.dtype.type
    code, cdt = _code(rdt), _cdt(rdt)
    B, N = X.shape
    shape = (B, F_ST, NFR_ST)
    cells = B * F_ST * NFR_ST
    cb, rb = cells * np.dtype(cdt).itemsize, cells * np.dtype(rdt).itemsize
    win = gwin()
    query = {"sst2": lib.ssq_ssq_stft2_workspace_bytes, "msst": lib.ssq_mssq_stft_workspace_bytes,
             "tsst": lib.ssq_tssq_stft_workspace_bytes, "reassign": lib.ssq_reassign_stft_workspace_bytes}[name]
    ws = int(query(code, B, N, NFFT, HOP))
    assert ws > 0
    pc = up.PAD_MODES[pad]
    with Door() as d:
        dx, dws, dS = d.buf(X.nbytes, X), d.buf(ws), d.buf(cb)
        if name == "sst2":
            dT, dw = d.buf(cb), d.buf(rb)
            rc = lib.ssq_ssq_stft2_exec(code, dx.p, B, N, _vp(win), NFFT, HOP, FS, pc, 0, -1.0, 3, dT.p, dS.p, dw.p, dws.p, ws,
                                        None)
            outs = [(dT, cdt), (dS, cdt), (dw, rdt)]
        elif name == "msst":
            dT, dw, db = d.buf(cb), d.buf(rb), d.buf(cells * 4)
            rc = lib.ssq_mssq_stft_exec(code, dx.p, B, N, _vp(win), NFFT, HOP, FS, pc, 0, -1.0, 3, order, MSST_ITER, dT.p, dS.p,
                                        dw.p, db.p, dws.p, ws, None)
            outs = [(dT, cdt), (dS, cdt), (dw, rdt), (db, np.int32)]
        elif name == "tsst":
            dT, dtau = d.buf(cb), d.buf(rb)
            rc = lib.ssq_tssq_stft_exec(code, dx.p, B, N, _vp(win), NFFT, HOP, FS, pc, order, -1.0, 3, dT.p, dS.p, dtau.p,
                                        dws.p, ws, None)
            outs = [(dT, cdt), (dS, cdt), (dtau, rdt)]
        else:
            dR, dw, dtau = d.buf(rb), d.buf(rb), d.buf(rb)
            rc = lib.ssq_reassign_stft_exec(code, dx.p, B, N, _vp(win), NFFT, HOP, FS, pc, -1.0, 3, dR.p, dS.p, dw.p, dtau.p,
                                            dws.p, ws, None)
            outs = [(dR, rdt), (dS, cdt), (dw, rdt), (dtau, rdt)]
        _lib.check(rc)
        return [b.get(shape, dt) for b, dt in outs]


@pytest.mark.parametrize("rdt,pad", STFT_PADS, ids=STFT_PAD_IDS)
@pytest.mark.parametrize("name,order", STFT_RUNS, ids=STFT_IDS)
def test_stft_family_past_the_limit(name, order, rdt, pad):
    """The host loops `b0 += 65535` of stft_sst2.hip, stft_msst.hip, stft_tsst.hip (the signal offset a kernel argument,
    `p.b0`) and stft_reassign.hip (`d_emax + b0`: signal 3's maximum sets the quantum of its Rx), on either door."""
    Xb = base_signals(N_ST).astype(rdt)
    idx = plain_index(B_BIG)
    X = tile(Xb, idx)
    small = stft_host(name, order, Xb, pad)
    big = stft_host(name, order, X, pad)
    for k, (a, s) in enumerate(zip(big, small)):
        assert_repeats(a, s, idx, "%s host plane %d" % (name, k))
    dev = stft_exec(name, order, X, pad)
    for k, (a, s) in enumerate(zip(dev, big)):
        assert_same(a, s, "%s device plane %d against the host call's" % (name, k))


def _sx_bound(rdt):
    """The project's STFT tolerances, of max|Sx| (the module docstrings of tests/test_gpu_sst2.py, _tsst.py, _reassign.py)."""
    return 1e-11 if rdt == np.float64 else 2e-6


@pytest.mark.parametrize("rdt,pad", STFT_PADS, ids=STFT_PAD_IDS)
@pytest.mark.parametrize("name,order", STFT_RUNS, ids=STFT_IDS)
def test_stft_family_base_batch_against_the_model(name, order, rdt, pad):
    """The 7-signal result every signal of the big batch is compared with, against the family's NumPy models on the
    library's own window tables.  The rules are those of tests/test_gpu_sst2.py, test_gpu_msst.py, test_gpu_tsst.py and
    test_gpu_reassign.py (test_parity_float64 / _float32 and the scatter tests): Sx within 1e-11 / 2e-6 of its maximum,
    a map within 10 x the model's own disagreement (FFT against DFT matrix in fp64, complex64 against complex128 for
    float32) on the bins with |V| >= 1e-2 max|V|, and the result as the scatter of the call's own maps within the bound
    that module derives.  Those modules already run n_fft = 16 (300-16-3, 1500-16-1), so the rules hold for this shape."""
    Xb = base_signals(N_ST)
    small = stft_host(name, order, Xb.astype(rdt), pad)
    tabs, win = gwin_tables(), gwin()
    f64 = rdt == np.float64
    kw = dict(hop_len=HOP, fs=FS, padtype=pad, tables=tabs)
    for b in range(K):
        x = Xb[b]
        if name in ("sst2", "msst"):
            from tests.test_gpu_msst import own_bins
            from tests.test_gpu_sst2 import bins_of
            Tx, Sx, w = small[0][b], small[1][b], small[2][b]
            V, wm, km, _ = ms.mssq_stft_ref(x, win, NFFT, order=order, n_iter=1, **kw)      # the one-step map
            other = ms.mssq_stft_ref(x, win, NFFT, order=order, n_iter=1, **dict(kw, **(
                dict(arith="dft") if f64 else dict(dtype=np.complex64))))[1]
            big = strong(V)
            tol = 10 * np.abs(other.astype(np.float64) - wm)[big].max()
            ew = np.abs(w.astype(np.float64) - wm)[big].max()
            kk, _, dw = bins_of(w, F_ST, False, rdt)
            _, vm, _ = bins_of(wm, F_ST, False, np.float64)
            tie = np.abs(vm - np.floor(vm) - 0.5) < 1e-9
            print("signal %d: Sx %.3g  w err %.3g (tol %.3g, %d strong bins)" % (b, np.abs(Sx - V).max() / np.abs(V).max(), ew,
                                                                               tol, big.sum()))
            assert np.abs(Sx - V).max() <= _sx_bound(rdt) * np.abs(V).max()
            assert ew <= tol
            if f64:
                assert np.array_equal(np.isinf(w), km == -1)
                assert int(((kk != km) & big & ~tie).sum()) == 0
            else:
                assert ((kk != km) & big).sum() <= 1e-3 * big.sum()
            if name == "msst":
                bins = small[3][b]
                assert np.array_equal(np.isinf(w), bins == -1)
                assert np.array_equal(bins, own_bins(w, F_ST, False, rdt, MSST_ITER)[0])
            else:
                bins = np.where(np.isfinite(w), kk, -1)
            ref = ms.scatter(Sx, bins, dw, "sum")
            tolT = 4 * _eps(rdt) * float(dw) * np.abs(Sx).sum(0).astype(np.float64)
            assert (np.abs(Tx.astype(np.complex128) - ref).max(0) <= tolT).all()
        elif name == "tsst":
            Tx, Sx, tau = small[0][b], small[1][b], small[2][b]
            V, taum, tgtm = ts.tsst_ref(x, win, NFFT, order=order, squeeze=False, **kw)[:3]
            other = ts.tsst_ref(x, win, NFFT, order=order, squeeze=False, **dict(kw, **(
                dict(arith="dft") if f64 else dict(dtype=np.complex64))))[1]
            big = strong(V)
            tol = 10 * np.abs(other.astype(np.float64) - taum)[big].max()
            et = np.abs(tau.astype(np.float64) - taum)[big].max()
            tgt, _ = ts.targets(tau, HOP, FS)
            _, vm = ts.targets(taum, HOP, FS)
            tie = np.abs(vm - np.floor(vm) - 0.5) < 1e-9
            print("signal %d: Sx %.3g  tau err %.3g s (tol %.3g, %d strong bins)" % (b, np.abs(Sx - V).max() / np.abs(V).max(),
                                                                                   et, tol, big.sum()))
            assert np.abs(Sx - V).max() <= _sx_bound(rdt) * np.abs(V).max()
            assert et <= tol
            if f64:
                assert np.array_equal(np.isinf(tau), tgtm == -1)
                assert int(((tgt != tgtm) & big & ~tie).sum()) == 0
            else:
                assert ((tgt != tgtm) & big).sum() <= 1e-3 * big.sum()
            # test_gpu_tsst.py::test_tx_is_the_scatter_of_the_calls_own_map
            keep = ~np.isposinf(tau)
            ref = ts.scatter(Sx, tgt, keep, HOP, NFFT, acc=np.longdouble)
            r, c = np.nonzero(keep)
            load = np.zeros(Sx.shape)
            np.add.at(load, (r, tgt[r, c]), np.abs(Sx[r, c]).astype(np.float64))
            assert not Tx[load == 0].any()
            assert (np.abs(Tx.astype(np.complex128) - ref) <= 8 * _eps(rdt) * load).all()
        else:
            from tests.test_gpu_reassign import own_targets, scatter_check
            Rx, Sx, w, tau = (p[b] for p in small)
            V, wm, taum, kkm, tgtm = rs.reassign_ref(x, win, NFFT, squeeze=False, **kw)[:5]
            _, wo, tauo = rs.reassign_ref(x, win, NFFT, squeeze=False, **dict(kw, **(
                dict(arith="dft") if f64 else dict(dtype=np.complex64))))[:3]
            big = strong(V)
            tolw = 10 * np.abs(wo.astype(np.float64) - wm)[big].max()
            tolt = 10 * np.abs(tauo.astype(np.float64) - taum)[big].max()
            ew = np.abs(w.astype(np.float64) - wm)[big].max()
            et = np.abs(tau.astype(np.float64) - taum)[big].max()
            keep, kk, tgt = own_targets(w, tau, HOP, FS)
            print("signal %d: Sx %.3g  w err %.3g (tol %.3g)  tau err %.3g (tol %.3g)"
                  % (b, np.abs(Sx - V).max() / np.abs(V).max(), ew, tolw, et, tolt))
            assert np.abs(Sx - V).max() <= _sx_bound(rdt) * np.abs(V).max()
            if f64:
                assert np.array_equal(np.isposinf(tau), kkm == -1) and np.array_equal(np.isposinf(w), kkm == -1)
            else:
                assert np.array_equal(keep, np.abs(V) > 10 * _eps(np.float32))
            assert ew <= tolw and et <= tolt
            assert (((kk != kkm) | (tgt != tgtm)) & big).sum() <= 1e-3 * big.sum()
            worst, total, clean = scatter_check(Rx, Sx, w, tau, HOP, FS)
            assert clean and worst <= 1 and total <= 1 and (Rx >= 0).all()
    if name == "reassign":
        # what makes `d_emax + b0` observable: signal 3's quantum is another power of two than its neighbours'
        from tests.test_gpu_reassign import quantum
        assert quantum(small[1][3]) > quantum(small[1][2]) and quantum(small[1][3]) > quantum(small[1][4])


# ==================================================================================== the fp64 CWT map family ==========
# name -> (batch, na, N, nv, the repetition).  'rows': batch > 65535 for the pad and scatter kernels and 131086 rows for
# the spectra and operator kernels.  'flush': rows = 65550 with the batch far below the limit: the second stride step of
# the workgroups y < 15 lands in ANOTHER SIGNAL (row 65535 + y belongs to signal 2184), mid-row-loop, which is the flush
# of cwt_flush_max.  2184 = 0 (mod 7), so under b % 7 signals 0 and 2184 would be the same base signal and a maximum
# carried from one to the other would change nothing; this shape therefore repeats the base signals as (3 + b + b // 1000)
# % 7: signal 0 is the large one (base 3) and signal 2184 is base 5, so a maximum that leaks across changes the quantum
# of signal 2184 and with it the bits of its Rx / Tx.  Its 30 scales are 16 to the octave (up to 3.5 x the smallest): at
# 8 to the octave the widest wavelets span several times the 16 samples and the MODEL's own two arithmetics put 2 % of the
# strong bins of tssq_cwt's order 2 within their disagreement of a rounding boundary, past the 1 % that
# tests/test_gpu_tssq_cwt.py allows a case to exempt; at 12 to the octave and above they put none there.
CWT_SHAPES = {
    "rows": (B_BIG, 2, 8, 1, plain_index),
    "flush": (2185, 30, 16, 16, lambda B: (3 + np.arange(B) + np.arange(B) // 1000) % K),
}
assert CWT_SHAPES["flush"][4](2185)[0] == 3 and CWT_SHAPES["flush"][4](2185)[2184] == 5
CWT_RUNS = [("sst2", 2), ("reassign", 1), ("tsst", 1), ("tsst", 2)]
CWT_IDS = ["ssq_cwt2", "reassign_cwt", "tssq_cwt-o1", "tssq_cwt-o2"]
CHUNK_ROWS = 4096                       # the rows per chunk of the small-workspace run of the 'flush' shape


def cwt_scales(na, nv):
    return S0 * 2.0 ** (np.arange(na) / nv)


def cwt_grids(na, nv, N):
    """(scales, row_const, f_asc, kind, f_idx) as the transforms derive them (upstream's Python, shared with `ssq_cwt`)."""
    code, p0, p1 = up._wavelet(GMW)
    return up._cwt_freq_grid(cwt_scales(na, nv), None, None, "peak", N, code, p0, p1, 1 / FS)


def cwt_maps(name, order):
    return 5 if name == "sst2" or (name == "tsst" and order == 2) else (3 if name == "reassign" else 2)


def cwt_host(name, order, X, na, nv):
    kw = dict(scales=cwt_scales(na, nv), fs=FS)
    if name == "sst2":
        out = up.ssq_cwt2(X, GMW, get_w=True, **kw)
        return [out[0], out[1], out[4]]
    if name == "reassign":
        out = up.reassign_cwt(X, GMW, get_w=True, get_tau=True, get_targets=True, **kw)
        return [out[0], out[1], out[4], out[5], out[6], out[7]]
    out = up.tssq_cwt(X, GMW, order=order, get_tau=True, get_targets=True, **kw)
    return [out[0], out[1], out[4], out[5]]


def cwt_work_bytes(name, order, B, na, N, R):
    """The documented layout: the head (the maxima to a multiple of 16 bytes, then 16 bytes a cell for reassign_cwt and 20
    for tssq_cwt, to a multiple of 16; none for ssq_cwt2), then 16 P (batch + 2 maps R)."""
    P = c2.p2up(N)[0]
    cell = {"sst2": 0, "reassign": 16, "tsst": 20}[name]
    head = ((8 * B + 15) // 16 * 16 + (cell * B * na * N + 15) // 16 * 16) if cell else 0
    return head + 16 * P * (B + 2 * cwt_maps(name, order) * R)


def cwt_exec(name, order, X, na, nv, R):
    """The device entry point on a workspace for R rows a chunk (R = all rows: one chunk, which is what the preferred
    size of the query gives and what makes the kernels stride)."""
    lib = _lib.load()
    rdt = X.dtype.type
    code, cdt = _code(rdt), _cdt(rdt)
    B, N = X.shape
    s, rowc, f, kind, f_idx = cwt_grids(na, nv, N)
    wcode, p0, p1 = up._wavelet(GMW)
    shape = (B, na, N)
    cells = B * na * N
    cb, rb = cells * np.dtype(cdt).itemsize, cells * np.dtype(rdt).itemsize
    mn = C.c_int64(0)
    if name == "sst2":
        pref = int(lib.ssq_ssq_cwt2_workspace_bytes(code, B, N, na, C.byref(mn)))
    elif name == "reassign":
        pref = int(lib.ssq_reassign_cwt_workspace_bytes(code, B, N, na, C.byref(mn)))
    else:
        pref = int(lib.ssq_tssq_cwt_workspace_bytes(code, B, N, na, order, C.byref(mn)))
    ws = cwt_work_bytes(name, order, B, na, N, R)
    # all rows in one chunk must be what the query prefers: otherwise no kernel strides and the test proves nothing
    assert mn.value <= ws <= pref and cwt_work_bytes(name, order, B, na, N, B * na) == pref
    with Door() as d:
        dx, dws, dW = d.buf(X.nbytes, X), d.buf(ws), d.buf(cb)
        if name == "sst2":
            dT, dw = d.buf(cb), d.buf(rb)
            rc = lib.ssq_ssq_cwt2_exec(code, dx.p, B, N, wcode, p0, p1, _vp(s), na, 1 / FS, _vp(rowc), _vp(f), up.FREQS[kind],
                                       f_idx or 0, 0, 0, -1.0, up.VARIANT_FLIPUD, dT.p, dW.p, dw.p, dws.p, ws, None, None)
            outs = [(dT, cdt), (dW, cdt), (dw, rdt)]
        elif name == "reassign":
            dR, dw, dtau, dk, dm = d.buf(rb), d.buf(rb), d.buf(rb), d.buf(cells * 4), d.buf(cells * 4)
            rc = lib.ssq_reassign_cwt_exec(code, dx.p, B, N, wcode, p0, p1, _vp(s), na, 1 / FS, _vp(f), up.FREQS[kind],
                                           f_idx or 0, 0, -1.0, up.VARIANT_FLIPUD, dR.p, dW.p, dw.p, dtau.p, dk.p, dm.p, dws.p,
                                           ws, None, None)
            outs = [(dR, rdt), (dW, cdt), (dw, rdt), (dtau, rdt), (dk, np.int32), (dm, np.int32)]
        else:
            nu = up.tssq_cwt_row_freqs(GMW, s)
            dT, dtau, dm = d.buf(cb), d.buf(rb), d.buf(cells * 4)
            rc = lib.ssq_tssq_cwt_exec(code, dx.p, B, N, wcode, p0, p1, _vp(s), _vp(nu), na, 1 / FS, 0, order, -1.0, dT.p, dW.p,
                                       dtau.p, dm.p, dws.p, ws, None, None)
            outs = [(dT, cdt), (dW, cdt), (dtau, rdt), (dm, np.int32)]
        _lib.check(rc)
        return [b.get(shape, dt) for b, dt in outs]


@RDTS
@pytest.mark.parametrize("shape", list(CWT_SHAPES))
@pytest.mark.parametrize("name,order", CWT_RUNS, ids=CWT_IDS)
def test_cwt_map_family_past_the_limit(name, order, shape, rdt):
    """cwt_maps64.h (the pad kernel's stride over signals, the spectra kernel's stride over rows), the operator kernels
    of cwt_sst2.hip, cwt_reassign.hip and cwt_tsst.hip (`rl += gridDim.y`, and the flush of a signal's maximum inside the
    stride) and their scatter and read-out kernels (stride over signals), on either door; the 'flush' shape once more in
    chunks of 4096 rows, which must not change a bit."""
    B, na, N, nv, index = CWT_SHAPES[shape]
    Xb = base_signals(N).astype(rdt)
    idx = index(B)
    X = tile(Xb, idx)
    small = cwt_host(name, order, Xb, na, nv)
    big = cwt_host(name, order, X, na, nv)
    for k, (a, s) in enumerate(zip(big, small)):
        assert_repeats(a, s, idx, "%s host plane %d" % (name, k))
    dev = cwt_exec(name, order, X, na, nv, B * na)
    for k, (a, s) in enumerate(zip(dev, big)):
        assert_same(a, s, "%s device plane %d against the host call's" % (name, k))
    if shape == "flush":
        chunked = cwt_exec(name, order, X, na, nv, CHUNK_ROWS)
        for k, (a, s) in enumerate(zip(chunked, dev)):
            assert_same(a, s, "%s plane %d in chunks of %d rows against one chunk" % (name, k, CHUNK_ROWS))


def _cwt_tables(s, P):
    """(T0, T1) [na, P] as the library evaluates them on the host (`ssq_ssq_cwt2_tables`): what the models run on."""
    from tests.test_gpu_cwt_sst2 import lib_tables
    return lib_tables(GMW, s, P)


@RDTS
@pytest.mark.parametrize("shape", list(CWT_SHAPES))
@pytest.mark.parametrize("name,order", CWT_RUNS, ids=CWT_IDS)
def test_cwt_map_family_base_batch_against_the_model(name, order, shape, rdt):
    """The 7-signal result against the NumPy models on the library's own wavelet tables, by the rules of
    tests/test_gpu_cwt_sst2.py, test_gpu_reassign_cwt.py and test_gpu_tssq_cwt.py (test_parity_float64 / _float32, the
    scatter tests and `ssqueeze` of the call's own outputs): fp64 maps within 10 x the model's FFT-against-DFT
    disagreement on the bins with |W| >= 1e-2 max|W|; float32 maps within that bound plus one float32 ulp of the model on
    the float32-rounded input; no strong target differs outside the bins whose model position is within the allowed
    error of a rounding boundary (or, for tssq_cwt order 2, of the thresholds that choose between d2 and d1)."""
    _, na, N, nv, _ = CWT_SHAPES[shape]
    Xb = base_signals(N)
    small = cwt_host(name, order, Xb.astype(rdt), na, nv)
    s, rowc, f, kind, f_idx = cwt_grids(na, nv, N)
    P = c2.p2up(N)[0]
    tabs = _cwt_tables(s, P)
    f64 = rdt == np.float64
    mw = ("gmw", 3.0, 60.0)
    gam = 10 * _eps(rdt)
    if name == "sst2":                                    # test_gpu_cwt_sst2.py::test_tx_is_ssqueeze_of_the_calls_own_outputs
        ref, _ = up.ssqueeze(small[1], small[2], scales=cwt_scales(na, nv), wavelet=GMW, maprange="peak", ssq_freqs=None,
                             squeezing="sum", flipud=True, fs=FS)
        assert ref.dtype == small[0].dtype and np.array_equal(small[0], ref)
    for b in range(K):
        x = Xb[b]
        xr = x if f64 else x.astype(np.float32).astype(np.float64)
        if name == "sst2":
            Tx, Wx, w2 = (p[b] for p in small)
            W, w2m, binm, _, dd = c2.cwt_sst2_ref(x, mw, s, f, kind, f_idx, rowc, dt=1 / FS, gamma=10 * EPS64, tabs=tabs,
                                                  details=True)
            Wd, w2d = c2.cwt_sst2_ref(x, mw, s, f, kind, f_idx, rowc, dt=1 / FS, gamma=10 * EPS64, arith="dft", tabs=tabs)[:2]
            big = strong(W)
            tolW, tolw = 10 * np.abs(W - Wd).max() / np.abs(W).max(), 10 * np.abs(w2m - w2d)[big].max()
            if f64:
                kk, _ = c2.bin_positions(w2, f, kind, f_idx)
                tie = np.abs(dd["v"] - np.floor(dd["v"]) - 0.5) < 1e-9
                assert np.abs(Wx - W).max() <= tolW * np.abs(W).max()
                assert np.array_equal(np.isinf(w2), np.isinf(w2m))
                assert np.abs(w2 - w2m)[big].max() <= tolw
                assert int(((kk != binm) & big & ~tie).sum()) == 0 and (tie & big).sum() <= 1e-3 * big.sum()
            else:
                Wf, w2f = c2.cwt_sst2_ref(xr, mw, s, f, kind, f_idx, rowc, dt=1 / FS, gamma=gam, tabs=tabs)[:2]
                bigf = strong(Wf)
                assert np.isfinite(w2[bigf]).all()
                err = np.abs(w2.astype(np.float64)[bigf] - w2f[bigf])
                ulp = np.spacing(w2f[bigf].astype(np.float32)).astype(np.float64)
                assert np.abs(Wx - Wf).max() <= 2 * _eps(np.float32) * np.abs(Wf).max()
                assert (err <= tolw + ulp).all()
        elif name == "reassign":
            from tests.test_gpu_reassign_cwt import scatter_check
            Rx, Wx, w, tau, kk, mm = (p[b] for p in small)
            kwm = dict(dt=1 / FS, flipud=True, tabs=tabs, squeeze=False)
            W, wm, taum, kkm, mmm = rc2.reassign_cwt_ref(x, mw, s, f, kind, f_idx, **kwm)[:5]
            _, wd, taud = rc2.reassign_cwt_ref(x, mw, s, f, kind, f_idx, arith="dft", **kwm)[:3]
            big = strong(W)
            tolw, tolt = 10 * np.abs(wm - wd)[big].max(), 10 * np.abs(taum - taud)[big].max()
            with np.errstate(all="ignore"):               # test_gpu_reassign_cwt.py::near_a_boundary
                lo, hi = (c2.bin_positions(np.maximum(wm + e, 0), f, kind, f_idx)[1] for e in (-tolw, tolw))
                v = c2.bin_positions(wm, f, kind, f_idx)[1]
                tie = np.abs(v - np.floor(v) - 0.5) <= np.maximum(np.abs(hi - lo), 1e-9)
                vt = taum * FS
                tie |= np.abs(vt - np.floor(vt) - 0.5) <= max(tolt * FS, 1e-9)
            if f64:
                assert np.array_equal(np.isposinf(w), kkm == -1) and np.array_equal(np.isposinf(tau), kkm == -1)
                assert np.abs(w - wm)[big].max() <= tolw and np.abs(tau - taum)[big].max() <= tolt
                assert int((((kk != kkm) | (mm != mmm)) & big & ~tie).sum()) == 0
                assert (tie & big).sum() <= 1e-3 * big.sum()
            else:
                Wf, wf, tauf = rc2.reassign_cwt_ref(xr, mw, s, f, kind, f_idx, rdt=np.float32, **kwm)[:3]
                bigf = strong(Wf)
                assert np.abs(Wx - Wf).max() <= 10 * np.abs(Wf.astype(np.complex64) - Wf).max()
                assert np.isfinite(w[bigf]).all() and np.isfinite(tau[bigf]).all()
                ew = np.abs(w[bigf].astype(np.float64) - wf[bigf].astype(np.float64))
                et = np.abs(tau[bigf].astype(np.float64) - tauf[bigf].astype(np.float64))
                assert (ew <= tolw + np.spacing(np.abs(wf[bigf])).astype(np.float64)).all()
                assert (et <= tolt + np.spacing(np.abs(tauf[bigf])).astype(np.float64)).all()
                assert (((kk != kkm) | (mm != mmm)) & big).sum() <= 1e-3 * big.sum()
            # test_targets_follow_the_reported_maps and test_rx_is_the_scatter_of_the_calls_own_maps
            gone = np.isposinf(w)
            assert np.array_equal(kk == -1, gone) and np.array_equal(mm == -1, gone)
            refk = sq.bins(w.astype(np.float64), sq.bin_params(f, kind != "linear"), na - 1, True)
            differ = ((kk != refk) & ~gone).sum() / max((~gone).sum(), 1)
            assert differ == 0 if f64 else differ <= 1e-3
            assert np.array_equal(mm[~gone], rc2.time_targets(tau, 1 / FS)[~gone])
            worst, total, clean = scatter_check(Rx, Wx, kk, mm)
            assert clean and worst <= 1 and total <= 1 and (Rx >= 0).all()
        else:
            from tests.test_gpu_tssq_cwt import scatter_check
            Tx, Wx, tau, mm = (p[b] for p in small)
            kwm = dict(dt=1 / FS, order=order, tabs=tabs, squeeze=False, details=True)
            W, taum, mmm, _, dm = tc.tssq_cwt_ref(x, mw, s, **kwm)
            _, taud, _, _, dd = tc.tssq_cwt_ref(x, mw, s, arith="dft", **kwm)
            big = strong(W)
            tolt = 10 * np.abs(taum - taud)[big].max()                     # test_gpu_tssq_cwt.py::fp64_bounds
            rel = 0.0
            if order == 2:
                an, ad = np.abs(dm["num"]), np.abs(dd["num"])
                rel = 10 * float((np.abs(an - ad) / np.maximum(an, gam ** 2))[big].max())
            bound = np.full(W.shape, tolt)
            if not f64:
                W, taum, mmm, _, dm = tc.tssq_cwt_ref(xr, mw, s, rdt=np.float32, **kwm)
                big = strong(W)
                with np.errstate(all="ignore"):
                    bt = tolt + np.spacing(np.abs(taum)).astype(np.float64)
                bound = np.where(np.isfinite(bt), bt, tolt)
                assert np.abs(Wx - W).max() <= 10 * np.abs(W.astype(np.complex64) - W).max()
            with np.errstate(all="ignore"):               # test_gpu_tssq_cwt.py::exemptions
                v = taum.astype(np.float64) * FS
                tie = np.abs(v - np.floor(v) - 0.5) <= np.maximum(bound * FS, 1e-12)
                flip = np.zeros(W.shape, dtype=bool)
                if order == 2:
                    flip = np.abs(np.abs(dm["d2"]) - N) <= bound * FS
                    flip |= np.abs(np.abs(dm["num"]) - gam ** 2) <= rel * gam ** 2
            ok = big & ~flip
            assert np.array_equal(np.isposinf(tau), np.isposinf(taum))
            assert (np.abs(tau.astype(np.float64) - taum.astype(np.float64))[ok] <= bound[ok]).all()
            assert int(((mm != mmm) & big & ~tie & ~flip).sum()) == 0
            assert ((tie | flip) & big).sum() <= 1e-2 * big.sum()
            # test_targets_follow_the_reported_tau and test_tx_is_the_scatter_of_the_calls_own_maps
            gone = np.isposinf(tau)
            assert np.array_equal(mm == -1, gone)
            assert np.array_equal(mm[~gone], rc2.time_targets(tau, 1 / FS)[~gone])
            worst, row, clean = scatter_check(Tx, Wx, mm, up.tssq_cwt_row_freqs(GMW, s))
            assert clean and worst <= 1 and row <= 1


# ======================================================================================================= ConceFT ======
CF_NA, CF_N, CF_J = 2, 8, 2
CF_VECTORS = np.array([[1.0, 0.5 + 0.25j], [0.3 - 0.2j, 1.0]])       # M = 2 fixed vectors


def conceft_host(X):
    out = up.conceft_cwt(X, GMW, scales=cwt_scales(CF_NA, 1), orders=CF_J, vectors=CF_VECTORS, fs=FS, get_Wx=True, get_w=True)
    return [out[0], out[3], out[4]]


@RDTS
def test_conceft_past_the_limit(rdt):
    """cwt_conceft.hip: the squeeze kernel's stride over the signals of a slice (and the classic CWT plan under it, which
    loops over signals on the host), on either door."""
    lib = _lib.load()
    Xb = base_signals(CF_N).astype(rdt)
    idx = plain_index(B_BIG)
    X = tile(Xb, idx)
    small, big = conceft_host(Xb), conceft_host(X)
    for k, (a, s) in enumerate(zip(big, small)):
        assert_repeats(a, s, idx, "conceft_cwt host plane %d" % k)
    code, cdt = _code(rdt), _cdt(rdt)
    B, N, na, J = B_BIG, CF_N, CF_NA, CF_J
    s, rowc, f, kind, f_idx = cwt_grids(na, 1, N)
    _, p0, p1 = up._wavelet(GMW)
    adm = np.array([up.gmw_adm_ssq(p0, p1, k) for k in range(J)])
    r, c = up._conceft_gauge(CF_VECTORS, adm)                         # what `conceft_cwt` hands the library
    M = r.shape[0]
    polys = np.ascontiguousarray(up.gmw_order_coefficients(p0, p1, range(J), average=False))
    ws = int(lib.ssq_conceft_cwt_workspace_bytes(code, B, N, na, J, None))
    assert ws > 0
    cells = B * na * N
    with Door() as d:
        dx, dws = d.buf(X.nbytes, X), d.buf(ws)
        dT, dW, dw = d.buf(cells * np.dtype(cdt).itemsize), d.buf(J * cells * np.dtype(cdt).itemsize), d.buf(
            M * cells * np.dtype(rdt).itemsize)
        _lib.check(lib.ssq_conceft_cwt_exec(code, dx.p, B, N, p0, p1, _vp(polys), polys.shape[1], J, _vp(r), M,
                                            float(adm[0] / c.sum()), _vp(s), na, 1 / FS, _vp(rowc), _vp(f), up.FREQS[kind],
                                            f_idx or 0, 0, -1.0, up.VARIANT_FLIPUD, dT.p, dW.p, dw.p, dws.p, ws, None, None))
        dev = [dT.get((B, na, N), cdt), dW.get((B, J, na, N), cdt), dw.get((B, M, na, N), rdt)]
    for k, (a, s_) in enumerate(zip(dev, big)):
        assert_same(a, s_, "conceft_cwt device plane %d against the host call's" % k)


@RDTS
def test_conceft_base_batch_against_the_model(rdt):
    """The 7-signal result against tests/helpers/conceft_ref.py on the call's own planes, by the rules of
    tests/test_gpu_conceft.py: test_planes_are_cwt_higher_orders (bitwise), test_bins_float64 (no strong coefficient
    outside a tie lands in another bin), test_w_float32 (its forward-error bound) and test_column_sums."""
    Xb = base_signals(CF_N).astype(rdt)
    Txs, Wxs, ws_ = conceft_host(Xb)
    na, N, J = CF_NA, CF_N, CF_J
    s, rowc, f, kind, f_idx = cwt_grids(na, 1, N)
    _, p0, p1 = up._wavelet(GMW)
    adm = np.array([up.gmw_adm_ssq(p0, p1, k) for k in range(J)])
    r, c = cf.gauge(CF_VECTORS, adm)
    M = r.shape[0]
    scale = adm[0] / c.sum()
    for b in range(K):
        Tx, Wx, w = Txs[b], Wxs[b], ws_[b]
        Wp, _, dWp = up.cwt_higher_order(Xb[b], GMW, order=range(J), average=False, derivative=True, scales=s, fs=FS)
        W, dW = np.stack(Wp).astype(np.complex128), np.stack(dWp).astype(np.complex128)
        assert np.array_equal(Wx, np.stack(Wp))
        _, Wm, wm = cf.squeeze_planes(W, dW, r, c, adm[0], f, rowc, kind != "linear", True, 10 * _eps(rdt), details=True)
        for m in range(M):
            big = np.abs(Wm[m]) >= 1e-2 * np.abs(Wm[m]).max()
            if rdt == np.float64:
                assert np.array_equal(np.isinf(w[m]), np.isinf(wm[m]))
                fin = np.isfinite(wm[m])
                with np.errstate(all="ignore"):
                    kg, _ = c2.bin_positions(w[m], f, kind, f_idx)
                    km, v = c2.bin_positions(wm[m], f, kind, f_idx)
                    tie = np.abs(v - np.floor(v) - 0.5) < 1e-9
                assert int(((kg != km) & big & fin & ~tie).sum()) == 0
            else:
                assert np.isfinite(w[m][big]).all()
                dWm = cf.combine(dW, r[m])
                sW = sum(abs(r[m, j]) * np.abs(W[j]) for j in range(J))
                sdW = sum(abs(r[m, j]) * np.abs(dW[j]) for j in range(J))
                a = np.abs(Wm[m])
                bound = (J + 4) * _eps(np.float32) * (sdW * a + np.abs(dWm) * sW) / (2 * np.pi * a * a)
                bound = bound + np.spacing(wm[m].astype(np.float32)).astype(np.float64)
                with np.errstate(invalid="ignore"):
                    assert ((np.abs(w[m].astype(np.float64) - wm[m]) / bound)[big] <= 1.0).all()
        U = (Wx.astype(np.complex128) * rowc[None, :, None]).sum(1)
        want = scale * (r.sum(0)[:, None] * U).sum(0)
        terms = sum(np.abs(cf.combine(Wx.astype(np.complex128), r[m])) for m in range(M)) * (rowc * scale)[:, None]
        tol = M * na * _eps(rdt) * terms.sum(0) + M * na * 10 * _eps(rdt)
        assert (np.abs(Tx.astype(np.complex128).sum(0) - want) <= tol).all()


# =============================================================== ssqueeze, phase_cwt, phase_stft on a held transform ====
def held_cwt(rdt):
    """(Wx, dWx) [K, 2, 8] of the base signals and their scales."""
    s = cwt_scales(2, 1)
    Wx, _, dWx = up.cwt(base_signals(8).astype(rdt), GMW, scales=s, fs=FS, derivative=True)
    return Wx, dWx, s


def _squeeze_cwt_host(W, dW, s, g):
    kw = dict(scales=s, fs=FS, ssq_freqs="log", maprange="peak", wavelet=GMW, flipud=True)
    w = up.phase_cwt(W, dW, gamma=g)
    return [w, up.ssqueeze(W, w, **kw)[0], up.ssqueeze(W, None, dWx=dW, gamma=g, **kw)[0]]


@RDTS
def test_ssqueeze_and_phase_cwt_past_the_limit(rdt):
    """ssqueeze.hip: the phase kernel's stride over planes and the squeeze kernel's stride over signals (from `w`); from
    `dWx` the CWT form launches once per signal on the host.  On either door ([65543, 2, 8])."""
    lib = _lib.load()
    Wb, dWb, s = held_cwt(rdt)
    idx = plain_index(B_BIG)
    W, dW = tile(Wb, idx), tile(dWb, idx)
    g = 10 * _eps(rdt)
    small, big = _squeeze_cwt_host(Wb, dWb, s, g), _squeeze_cwt_host(W, dW, s, g)
    for name, a, b in zip(("phase_cwt", "ssqueeze from w", "ssqueeze from dWx"), big, small):
        assert_repeats(a, b, idx, name)
    code, cdt = _code(rdt), _cdt(rdt)
    B, F, N = W.shape
    wcode, p0, p1 = up._wavelet(GMW)
    f = np.ascontiguousarray(up._ssq_freqs(s, N, wcode, p0, p1, 1 / FS, "peak", "log", s), dtype=np.float64)
    rowc = np.ascontiguousarray(up._row_const(s, "log", 1), dtype=np.float64).astype(rdt)
    cells = B * F * N
    with Door() as d:
        dWd, ddW, dc = d.buf(W.nbytes, W), d.buf(dW.nbytes, dW), d.buf(rowc.nbytes, rowc)
        dw, dT1, dT2 = d.buf(cells * np.dtype(rdt).itemsize), d.buf(W.nbytes), d.buf(W.nbytes)
        _lib.check(lib.ssq_phase_exec(code, dWd.p, ddW.p, None, B, F, N, g, dw.p, None))
        _lib.check(lib.ssq_ssqueeze_w_exec(code, dWd.p, dw.p, B, F, N, dc.p, _vp(f), up.FREQS["log"], 0, 0, 1, dT1.p, None))
        _lib.check(lib.ssq_ssqueeze_dwx_exec(code, dWd.p, ddW.p, None, B, F, N, dc.p, _vp(f), up.FREQS["log"], 0, 0, 1, g,
                                             dT2.p, None))
        _lib.check(lib.ssq_device_sync())
        dev = [dw.get((B, F, N), rdt), dT1.get((B, F, N), cdt), dT2.get((B, F, N), cdt)]
    for name, a, b in zip(("ssq_phase_exec", "ssq_ssqueeze_w_exec", "ssq_ssqueeze_dwx_exec"), dev, big):
        assert_same(a, b, name + " against the host call's")


@RDTS
def test_ssqueeze_and_phase_cwt_base_batch_against_the_restatement(rdt):
    """tests/test_gpu_ssqueeze.py's comparisons (`_check_w`, `_close_tx`) on the 7 held transforms: the phase against
    tests/helpers/ssqueeze_ref.py and the fused `ssq_cwt`'s get_w, both squeezes against the restatement / the fused Tx."""
    from tests.test_gpu_ssqueeze import _check_w, _close_tx
    Wb, dWb, s = held_cwt(rdt)
    g = 10 * _eps(rdt)
    w, Tw, Td = _squeeze_cwt_host(Wb, dWb, s, g)
    N = Wb.shape[-1]
    wcode, p0, p1 = up._wavelet(GMW)
    f = np.asarray(up._ssq_freqs(s, N, wcode, p0, p1, 1 / FS, "peak", "log", s))
    rowc = sq.row_const(s, "log", 1)
    Tf, _, _, _, wf = up.ssq_cwt(base_signals(8).astype(rdt), GMW, scales=s, fs=FS, maprange="peak", flipud=True, get_w=True)
    for b in range(K):
        _check_w(w[b], Wb[b], dWb[b], wf[b], sq.phase_cwt(Wb[b], dWb[b], g), g, rdt)
        R = sq.ssqueeze(Wb[b].astype(np.complex128), w[b].astype(np.float64), f, rowc, "log", "sum", True)
        _close_tx(Tw[b], R, rdt)
        _close_tx(Td[b], Tf[b], rdt)


@RDTS
def test_ssqueeze_and_phase_stft_at_the_limit(rdt):
    """The STFT form: `phase_stft` strides over planes at any batch; `ssqueeze` from dSx runs `launch_reassign_cols` with
    the batch on grid.y and refuses above 65535 with the documented message: 65535 signals pass, 65536 do not."""
    from tests.test_gpu_ssqueeze import _check_w, _close_tx
    Xb = base_signals(N_ST).astype(rdt)
    win = gwin()
    Tf, Sb, _, Sfs, wf, dSb = up.ssq_stft(Xb, win, n_fft=NFFT, hop_len=HOP, fs=FS, get_w=True, get_dWx=True)
    idx = plain_index(LIMIT + 1)
    S, dS = tile(Sb, idx), tile(dSb, idx)
    ws_, wb = up.phase_stft(Sb, dSb, Sfs), up.phase_stft(S, dS, Sfs)
    assert_repeats(wb, ws_, idx, "phase_stft")
    Ts = up.ssqueeze(Sb, None, ssq_freqs=Sfs, Sfs=Sfs, dWx=dSb, transform="stft")[0]
    Tb = up.ssqueeze(S[:LIMIT], None, ssq_freqs=Sfs, Sfs=Sfs, dWx=dS[:LIMIT], transform="stft")[0]
    assert_repeats(Tb, Ts, idx[:LIMIT], "ssqueeze from dSx at 65535 signals")
    with pytest.raises(ValueError, match="STFT: batch must be <= 65535"):
        up.ssqueeze(S, None, ssq_freqs=Sfs, Sfs=Sfs, dWx=dS, transform="stft")
    g = 10 * _eps(rdt)
    for b in range(K):
        _check_w(ws_[b], Sb[b], dSb[b], wf[b], sq.phase_stft(Sb[b], dSb[b], Sfs, g), g, rdt, scale=float(Sfs[-1]))
        _close_tx(Ts[b], Tf[b], rdt)


# =========================================================================================== component inversion =======
@pytest.mark.parametrize("dt", [np.complex128, np.complex64], ids=["c128", "c64"])
def test_issq_components_past_the_limit(dt):
    """issq_components.hip: grid.y = min(batch, 65535) with a stride over signals (B = 65543, F = 4, N = 8, K = 1), through
    `issq_cwt` / `issq_stft` with cc, cw and through `ssq_issq_components_exec`; the base planes against
    tests/helpers/components_ref.py by tests/test_gpu_components.py::_check."""
    from tests.test_gpu_components import _check
    lib = _lib.load()
    F, N = 4, 8
    rng = np.random.default_rng(5)
    Tb = (rng.standard_normal((K, F, N)) + 1j * rng.standard_normal((K, F, N))).astype(dt)
    Tb[3] *= 37
    ccb = rng.integers(-1, F + 1, size=(K, N)).astype(np.int64)
    cwb = rng.integers(0, 3, size=(K, N)).astype(np.int64)
    idx = plain_index(B_BIG)
    T, cc, cw = tile(Tb, idx), tile(ccb, idx), tile(cwb, idx)
    win = np.hanning(2 * (F - 1)) + 0.05
    adm = up.adm_ssq("gmw")
    for call, ref in ((lambda A, c, w: up.issq_cwt(A, "gmw", cc=c, cw=w), lambda A, c, w: cr.issq_cwt(A, c, w, adm)),
                      (lambda A, c, w: up.issq_stft(A, win, cc=c, cw=w), lambda A, c, w: cr.issq_stft(A, c, w, win))):
        small, big = call(Tb, ccb, cwb), call(T, cc, cw)
        assert big.shape == (B_BIG, 2, N)
        assert_repeats(big, small, idx, "component inversion")
        for b in range(K):
            _check(small[b], ref(Tb[b], ccb[b], cwb[b]), Tb[b])
    want = up.issq_cwt(T, "gmw", cc=cc, cw=cw)
    code = _lib.SSQ_F32 if dt == np.complex64 else _lib.SSQ_F64
    with Door() as d:
        dT, dcc, dcw, dx = d.buf(T.nbytes, T), d.buf(cc.nbytes, cc), d.buf(cw.nbytes, cw), d.buf(B_BIG * 2 * N * 8)
        _lib.check(lib.ssq_issq_components_exec(code, dT.p, B_BIG, F, N, dcc.p, dcw.p, 0, 1, 2.0 / adm, dx.p, None))
        _lib.check(lib.ssq_device_sync())
        got = dx.get((B_BIG, 2, N), np.float64)
    assert_same(got, want, "ssq_issq_components_exec against issq_cwt")


# ================================================================================================ batched inverses =====
def _spread_bound(gpu, ref64, ref_own):
    """No existing tolerance covers a float32 row-sum inverse: 4 x the spread between the reference in float64 and in
    the call's dtype (one factor of two for the order of the sum, one for fused multiply-add)."""
    return np.abs(gpu.astype(np.float64) - ref64).max(), 4 * np.abs(ref_own.astype(np.float64) - ref64).max()


@pytest.mark.parametrize("dt", [np.complex128, np.complex64], ids=["c128", "c64"])
def test_row_sum_inverses_past_the_limit(dt):
    """api_upstream.hip: `issq_stft`, `issq_cwt` and `icwt` on [65543, F, N] go through the device in slices of at most
    65535 signals (`issq_batch_typed`).  The base planes against oracle/upstream_oracle.py: fp64 within 1e-12 of max|x|
    (tests/test_gpu_upstream.py, the inverses against the restatement); complex64 within 4 x the spread between the
    restatement in float64 and in float32.  That spread, on these planes and relative to max|x|: issq_stft 2.8e-8 ..
    9.3e-8, issq_cwt 3.4e-8 .. 1.0e-7, icwt 3.6e-8 .. 1.3e-7 over the 7 base planes (sums of 9 resp. 4 float32 terms)."""
    rdt = np.float32 if dt == np.complex64 else np.float64
    rng = np.random.default_rng(6)
    idx = plain_index(B_BIG)
    sc = cwt_scales(4, 2)
    win = gwin()
    shapes = {"issq_stft": (NFFT // 2 + 1, 16), "issq_cwt": (4, 8), "icwt": (4, 8)}
    calls = {"issq_stft": (lambda A: up.issq_stft(A, win), lambda A: u.issq_stft(A, win)),
             "issq_cwt": (lambda A: up.issq_cwt(A, GMW), lambda A: u.issq_cwt(A, GMW)),
             "icwt": (lambda A: up.icwt(A, GMW, scales=sc), lambda A: u.icwt(A, GMW, scales=sc))}
    for name, (F, N) in shapes.items():
        Tb = (rng.standard_normal((K, F, N)) + 1j * rng.standard_normal((K, F, N))).astype(dt)
        Tb[3] *= 37
        call, ref = calls[name]
        small, big = call(Tb), call(tile(Tb, idx))
        assert big.shape == (B_BIG, N) and big.dtype == rdt
        assert_repeats(big, small, idx, name)
        for b in range(K):
            r64 = ref(Tb[b].astype(np.complex128))
            if rdt == np.float64:
                assert np.abs(small[b] - r64).max() <= 1e-12 * np.abs(r64).max(), name
            else:
                # the restatement is linear, a weighted column sum of Re: its weights (from unit planes), applied in float32
                unit = np.array([ref(np.where(np.arange(F)[:, None] == i, 1.0 + 0j, 0j) * np.ones((F, 1)))[0] for i in range(F)])
                own = (Tb[b].real * unit.astype(np.float32)[:, None]).sum(axis=0, dtype=np.float32)
                err, bound = _spread_bound(small[b], r64, own)
                assert err <= bound, "%s: error %.3g against 4 x the spread %.3g" % (name, err, bound / 4)


@pytest.mark.parametrize("dt", [np.complex128, np.complex64], ids=["c128", "c64"])
def test_istft_past_the_limit(dt, monkeypatch):
    """`istft` on [65543, 9, 4] (n_fft = 16, hop_len = 4, N = 16).  The streaming kernel refuses more than 65535 signals a
    launch (istft_fused.hip): the host entry point slices the batch for it (api_upstream.hip, `istft_batch_fused`) and the
    device entry point loops over launches; the three-kernel path runs one signal at a time at any batch.  Held on the
    kernel by SSQ_ISTFT_FUSED=1 (the shape has too few tiles to be routed there by itself), every signal equals its base
    signal bit for bit on either door; the device door also runs the three-kernel path on the whole batch.  The base
    batch against `upstream_oracle.istft` by the bound of tests/test_gpu_inverse_batch.py::test_fused_istft_against_the_
    oracle: e_new <= 4 e_old + 4 eps max|x|, e_old the error of the three-kernel path."""
    lib = _lib.load()
    rdt = np.float32 if dt == np.complex64 else np.float64
    n_fft, hop, N = 16, 4, 16
    F, nfr = n_fft // 2 + 1, (N - 1) // hop + 1
    win = np.hanning(n_fft) + 0.1
    Xb = base_signals(N)
    Sb = np.stack([u.stft(Xb[b], win, n_fft=n_fft, hop_len=hop) for b in range(K)]).astype(dt)
    idx = plain_index(B_BIG)
    S = tile(Sb, idx)
    kw = dict(n_fft=n_fft, hop_len=hop, N=N)
    monkeypatch.setenv("SSQ_ISTFT_FUSED", "0")
    old = up.istft(Sb, win, **kw)
    monkeypatch.setenv("SSQ_ISTFT_FUSED", "1")
    fused = C.c_int(-1)
    lib.ssq_istft_batch_workspace_bytes(_code(rdt), B_BIG, nfr, n_fft, hop, N, C.byref(fused))
    assert fused.value == 1
    small, big = up.istft(Sb, win, **kw), up.istft(S, win, **kw)
    assert_repeats(big, small, idx, "istft, streaming kernel, host slices")
    eps = _eps(rdt)
    for b in range(K):
        ref = u.istft(Sb[b], win, **kw)
        e_old = np.abs(old[b] - ref).max()
        assert np.abs(small[b] - ref).max() <= 4 * e_old + 4 * eps * np.abs(ref).max()
    for path, want in ((1, small), (0, old)):
        with Door() as d:
            dS, dx = d.buf(S.nbytes, S), d.buf(B_BIG * N * np.dtype(rdt).itemsize)
            _lib.check(lib.ssq_istft_batch_exec(_code(rdt), dS.p, B_BIG, nfr, _vp(win), n_fft, hop, N, 1, 1, path, dx.p, None))
            got = dx.get((B_BIG, N), rdt)
        assert_repeats(got, want, idx, "ssq_istft_batch_exec, path %d" % path)


# ================================================================================================= ridge extraction ====
def test_ridges_at_the_limit():
    """ridge.hip puts the batch on grid.x / grid.y unsliced and refuses above 65535 in `check_shape`, which both
    `ssq_extract_ridges_host` and `ssq_ridge_track_host` call first: 65536 signals of F = 4, N = 8 are refused with the
    limit in the message, 65535 give every signal the ridges of tests/helpers/ridge_oracle.py on its base plane."""
    from tests.test_gpu_ridges import _same_bits, _track_gpu
    F, N = 4, 8
    rng = np.random.default_rng(8)
    Tb = (rng.standard_normal((K, F, N)) + 1j * rng.standard_normal((K, F, N)))
    Tb[3] *= 37
    scales = np.exp(np.linspace(0.5, 2, F))
    idx = plain_index(LIMIT + 1)
    T = tile(Tb, idx)
    with pytest.raises(ValueError, match="65535"):
        up.extract_ridges(T, scales, penalty=2.0, n_ridges=2, bw=1)
    got = up.extract_ridges(T[:LIMIT], scales, penalty=2.0, n_ridges=2, bw=1, get_params=True)
    small = up.extract_ridges(Tb, scales, penalty=2.0, n_ridges=2, bw=1, get_params=True)
    for a, s in zip(got, small):
        assert_repeats(a, s, idx[:LIMIT], "extract_ridges at 65535 signals")
    for b in range(K):                                                # tests/test_gpu_ridges.py::_oracle_match
        ref = ro.extract_ridges(Tb[b], scales, penalty=2.0, n_ridges=2, bw=1, get_params=True)
        assert np.array_equal(small[0][b], ref[0])
        assert small[1].dtype == ref[1].dtype and np.array_equal(small[1][b], ref[1])
        assert np.allclose(small[2][b], ref[2], rtol=1e-12, atol=0)
    cost_b = rng.standard_normal((K, F, N)) ** 2 * 3
    cost = tile(cost_b, idx)
    m = ro.metric(scales, np.float64)
    with pytest.raises(_lib.SsqHipError, match="65535"):
        _track_gpu(cost, m, 2.0, np.float64, np.float64)
    pen, ridge = _track_gpu(cost[:LIMIT], m, 2.0, np.float64, np.float64)
    P = ro.penalty_matrix(m, 2.0, np.float64)
    for b in range(K):                                                # tests/test_gpu_ridges.py::test_dp_is_exact
        pen_o, ridge_o = ro.track(cost_b[b], P, np.float64(ro.EPS64))
        assert _same_bits(pen[b], pen_o) and np.array_equal(ridge[b], ridge_o)
    assert_repeats(pen, pen[:K].copy(), idx[:LIMIT], "ridge_track forward cost")
    assert_repeats(ridge, ridge[:K].copy(), idx[:LIMIT], "ridge_track ridges")


# ============================================================================ first-order transforms through plans ======
# name -> (n_fft, N, hop, force_generic, variant).  The fused kernels start at n_fft = 64 (stft_fused.hip::fused_supported),
# so the fused plan is the smallest of those; n_fft = 16 without `force_generic` is routed to the generic kernels by the
# plan itself, n_fft = 12 by `force_generic`, and an upstream-variant plan runs the per-signal device FFT and then
# `launch_reassign_cols`.  The last three reach stft_generic.hip with the batch on grid.z / grid.y.
PLANS = {
    "fused-64": (64, 64, 16, 0, 0),
    "routed-16": (16, 32, 8, 0, 0),
    "generic-12": (12, 32, 8, 1, 0),
    "upstream-16": (16, 32, 8, 0, 3),
}


def plan_run(plan, kind, X, F, nfr):
    lib = _lib.load()
    B = X.shape[0]
    cdt = _cdt(X.dtype.type)
    ws = int(lib.ssq_stft_plan_workspace_bytes(plan, B, kind))
    assert ws >= 0
    with Door() as d:
        dx, dout, dws = d.buf(X.nbytes, X), d.buf(B * F * nfr * np.dtype(cdt).itemsize), d.buf(ws)
        _lib.check(lib.ssq_stft_plan_exec(plan, kind, dx.p, B, dout.p, dws.p, ws, None))
        _lib.check(lib.ssq_device_sync())
        return dout.get((B, F, nfr), cdt)


@RDTS
@pytest.mark.parametrize("name", list(PLANS))
def test_first_order_plans_past_the_limit(name, rdt):
    """`ssq_stft_plan_exec` on 65543 device-resident signals (the door of batch.py and of the chunked front end), outputs
    SX and TX: every signal equals its base signal's bit for bit, whichever kernels the plan was routed to.  The 7-signal
    run against oracle/ssq_oracle.py (upstream variant: upstream_oracle.py) by the rules of tests/test_gpu_stft.py::
    _check_ssq_f64 / _check_ssq_f32 and tests/test_gpu_upstream.py::_check_ssq_stft: Sx within 1e-11 / 2e-6 of its maximum;
    Tx against the oracle's Sx re-accumulated under the plan's own bins (its WK output) within 1e-10 of its maximum in
    fp64, float32 against its own Sx within 2e-5; fp64 bins differ from the oracle's at half-bin ties or on tiny bins only."""
    lib = _lib.load()
    n_fft, N, hop, force, variant = PLANS[name]
    F, nfr = n_fft // 2 + 1, (N - 1) // hop + 1
    win = np.hanning(n_fft) + 0.1
    Xb = base_signals(N).astype(rdt)
    idx = plain_index(B_BIG)
    X = tile(Xb, idx)
    plan = C.c_void_p()
    _lib.check(lib.ssq_stft_plan_create_v(C.byref(plan), _code(rdt), N, _vp(win), n_fft, hop, 1.0, 0, 0, -1.0, force, variant))
    try:
        assert lib.ssq_stft_plan_is_fused(plan) == (1 if name == "fused-64" else 0)
        small = {k: plan_run(plan, k, Xb, F, nfr) for k in (_lib.OUT_SX, _lib.OUT_TX, _lib.OUT_WK)}
        for k in (_lib.OUT_SX, _lib.OUT_TX):
            assert_repeats(plan_run(plan, k, X, F, nfr), small[k], idx, "%s output kind %d" % (name, k))
    finally:
        lib.ssq_stft_plan_destroy(plan)
    f64 = rdt == np.float64
    for b in range(K):
        x = Xb[b].astype(np.float64)
        Sx, Tx, wk = (small[k][b] for k in (_lib.OUT_SX, _lib.OUT_TX, _lib.OUT_WK))
        if variant:
            _, So, _, Sfo, im = u.ssq_stft(x, win, n_fft=n_fft, hop_len=hop, fs=1.0, return_intermediates=True)
            dw, ko, wo = float(im["const"]), im["k"], im["w"]
            keep_o = ko >= 0
        else:
            _, _, im = o.ssq_stft(x, win, n_fft=n_fft, hop_len=hop, fs=1.0, return_intermediates=True)
            So, dw, ko, wo = im["Sx"], float(im["dw"]), im["k"], im["w"]
            keep_o = ~np.isinf(wo)
        smax = np.abs(So).max()
        assert np.abs(Sx - So).max() <= _sx_bound(rdt) * smax
        kg = wk.imag.astype(np.int64)
        keep_g = wk.imag >= 0
        if f64:
            flip = keep_o != keep_g
            assert np.abs(So[flip]).max(initial=0.0) <= 1e-6 * smax + 1e-12
            mism = keep_o & keep_g & (kg != ko)
            if mism.any():
                tq = wo[mism] / dw
                near_tie = np.abs(tq - np.floor(tq) - 0.5) < 1e-9 * np.maximum(1.0, np.abs(tq))
                assert (near_tie | (np.abs(So[mism]) <= 1e-6 * smax)).all()
            assert mism.mean() <= 1e-3
            ref = o.accumulate_tx(So, np.where(keep_g, kg, 0), keep_g, dw, F)
            assert np.abs(Tx - ref).max() <= 1e-10 * max(np.abs(ref).max(), 1e-300)
        else:
            ref = o.accumulate_tx(Sx.astype(np.complex128), np.where(keep_g, kg, 0), keep_g, float(np.float32(dw)), F)
            assert np.abs(Tx - ref).max() <= 2e-5 * np.abs(ref).max()


# ================================================================================== more scales than the limit =========
def test_cwt_refuses_more_scales_than_its_grid():
    """cwt_kernels.hip puts `na` on grid.y of its table kernels; `ssq_cwt_plan_create*` refuses na > 32767 before any
    launch (api_cwt.hip), so the limit of the grid is never reached: 65536 linear scales are refused with the limit in the
    message, not with a raw launch error, and the largest grid the plan accepts, 32767 scales, matches the oracle on its
    first and last rows (1e-11 of max|Wx|, tests/test_gpu_upstream.py)."""
    x = base_signals(8)[0]
    with pytest.raises(ValueError, match="32767"):
        up.cwt(x, GMW, scales=np.linspace(2.0, 4.0, LIMIT + 1), fs=FS)
    sc = np.linspace(2.0, 4.0, 32767)
    Wx, _ = up.cwt(x, GMW, scales=sc, fs=FS)
    rows = [0, 1, 32765, 32766]
    Wo, _ = u.cwt(x, GMW, scales=sc[rows], fs=FS)
    assert np.abs(Wx[rows] - Wo).max() <= 1e-11 * np.abs(Wo).max()


# ======================================================================================================== refusals =====
def test_refusals_name_what_they_refuse():
    """The limits the library refuses at rather than crosses, each before any launch."""
    lib = _lib.load()

    def err():
        return lib.ssq_last_error().decode()
    with Door() as d:
        p = d.buf(64)
        # frontend.hip: the chunked front end's halo fill (channels on grid.y) and relayout (rows on grid.y, chunks on grid.z)
        assert lib.ssq_chunk_halo_fill(_lib.SSQ_F32, p.p, LIMIT + 1, 1, 1, 0, None) != 0 and "too many channels" in err()
        assert lib.ssq_chunks_relayout(_lib.SSQ_F32, p.p, 1, 1, LIMIT + 1, 1, 0, 1, p.p, 1, 0, 1, 0, None) != 0
        assert "too many rows or chunks" in err()
        assert lib.ssq_chunks_relayout(_lib.SSQ_F32, p.p, 1, LIMIT + 1, 1, 1, 0, 1, p.p, LIMIT + 1, 0, 1, 0, None) != 0
        assert "too many rows or chunks" in err()
        # ridge.hip, device door
        assert lib.ssq_ridges_workspace_bytes(_lib.SSQ_F64, LIMIT + 1, 4, 8) == -1 and "65535" in err()
        # ssqueeze.hip, device door of the STFT form
        f = np.linspace(0.0, 1.0, 4)
        assert lib.ssq_ssqueeze_dwx_exec(_lib.SSQ_F64, p.p, p.p, p.p, LIMIT + 1, 4, 1, p.p, _vp(f), up.FREQS["linear"], 0, 0,
                                         0, 1e-9, p.p, None) != 0
        assert "STFT: batch must be <= 65535" in err()
