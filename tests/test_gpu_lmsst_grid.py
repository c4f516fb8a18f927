"""GPU tests of `upstream.lmssq_stft` and `upstream.lmssq_cwt` past the 65535 grid-dimension limit, on the shapes and the
doors tests/test_gpu_grid_limits.py uses for `mssq_stft` (65543 signals of 32 samples, n_fft 16) and for the CWT map
family (65543 signals x 2 scales = 131086 rows of 8 samples): stft_lmsst.hip's `for_signal_runs` (the signal offset a
kernel argument, `p.b0`), cwt_maps64.h's strides over signals and rows with a map set of W alone, and the strides of
cwt_lmsst.hip's Wx and plane kernels.  The first, the last and the signals on either side of the limit are held to single
calls; every signal to its base signal in a batch of 7."""
import ctypes as C

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests import test_gpu_grid_limits as g

pytestmark = pytest.mark.gpu

PROBES = (0, g.LIMIT - 1, g.LIMIT, g.B_BIG - 1)         # the first, the two on either side of a launch's end, the last
STFT_DELTA = 3
CWT_DELTA = 1


def stft_host(X, pad):
    out = up.lmssq_stft(X, g.gwin(), n_fft=g.NFFT, hop_len=g.HOP, fs=g.FS, padtype=pad, delta=STFT_DELTA, get_bins=True)
    return [out[0], out[1], out[4]]


def stft_exec(X, pad):
    lib = _lib.load()
    rdt = X.dtype.type
    code, cdt = g._code(rdt), g._cdt(rdt)
    B, N = X.shape
    shape = (B, g.F_ST, g.NFR_ST)
    cells = B * g.F_ST * g.NFR_ST
    cb = cells * np.dtype(cdt).itemsize
    ws = int(lib.ssq_lmssq_stft_workspace_bytes(code, B, N, g.NFFT, g.HOP))
    assert ws == (8 * B * N if rdt == np.float32 else 0)
    with g.Door() as d:
        dx, dT, dS, db = d.buf(X.nbytes, X), d.buf(cb), d.buf(cb), d.buf(cells * 4)
        dws = d.buf(ws) if ws else None
        _lib.check(lib.ssq_lmssq_stft_exec(code, dx.p, B, N, g._vp(g.gwin()), g.NFFT, g.HOP, g.FS, up.PAD_MODES[pad], 0, -1.0, 3,
                                           STFT_DELTA, dT.p, dS.p, db.p, dws.p if dws else None, ws, None))
        return [dT.get(shape, cdt), dS.get(shape, cdt), db.get(shape, np.int32)]


@pytest.mark.parametrize("rdt,pad", g.STFT_PADS, ids=g.STFT_PAD_IDS)
def test_lmssq_stft_past_the_limit(rdt, pad):
    Xb = g.base_signals(g.N_ST).astype(rdt)
    idx = g.plain_index(g.B_BIG)
    X = g.tile(Xb, idx)
    small = stft_host(Xb, pad)
    big = stft_host(X, pad)
    for k, (a, s) in enumerate(zip(big, small)):
        g.assert_repeats(a, s, idx, "lmssq_stft host plane %d" % k)
    for b in PROBES:
        one = stft_host(X[b], pad)
        for k in range(3):
            assert np.array_equal(big[k][b], one[k]), (b, k)
    assert (small[2] >= 0).any() and (small[2] != np.arange(g.F_ST)[None, :, None])[small[2] >= 0].any()   # (something moved)
    dev = stft_exec(X, pad)
    for k, (a, s) in enumerate(zip(dev, big)):
        g.assert_same(a, s, "lmssq_stft device plane %d against the host call's" % k)


def cwt_host(X, na, nv):
    out = up.lmssq_cwt(X, g.GMW, scales=g.cwt_scales(na, nv), fs=g.FS, delta=CWT_DELTA, get_w=True, get_rows=True)
    return [out[0], out[1], out[4], out[5]]


def cwt_exec(X, na, nv):
    """The device door on the preferred workspace: every row in one chunk, which is what makes the kernels stride."""
    lib = _lib.load()
    rdt = X.dtype.type
    code, cdt = g._code(rdt), g._cdt(rdt)
    B, N = X.shape
    s, rowc, f, kind, f_idx = g.cwt_grids(na, nv, N)
    wcode, p0, p1 = up._wavelet(g.GMW)
    nu_hz = np.ascontiguousarray(up.tssq_cwt_row_freqs(g.GMW, s) * g.FS)
    shape = (B, na, N)
    cells = B * na * N
    cb, rb = cells * np.dtype(cdt).itemsize, cells * np.dtype(rdt).itemsize
    mn = C.c_int64(0)
    ws = int(lib.ssq_lmssq_cwt_workspace_bytes(code, B, N, na, C.byref(mn)))
    assert ws == 16 * g.c2.p2up(N)[0] * (B + 2 * B * na) and mn.value <= ws
    with g.Door() as d:
        dx, dws, dT, dW, dw, dr = d.buf(X.nbytes, X), d.buf(ws), d.buf(cb), d.buf(cb), d.buf(rb), d.buf(cells * 4)
        _lib.check(lib.ssq_lmssq_cwt_exec(code, dx.p, B, N, wcode, p0, p1, g._vp(s), na, 1 / g.FS, g._vp(rowc), g._vp(f),
                                          up.FREQS[kind], f_idx or 0, 0, 0, -1.0, up.VARIANT_FLIPUD, CWT_DELTA, g._vp(nu_hz),
                                          dT.p, dW.p, dw.p, dr.p, dws.p, ws, None, None))
        return [dT.get(shape, cdt), dW.get(shape, cdt), dw.get(shape, rdt), dr.get(shape, np.int32)]


@g.RDTS
def test_lmssq_cwt_past_the_limit(rdt):
    B, na, N, nv, index = g.CWT_SHAPES["rows"]
    assert B * na > g.LIMIT
    Xb = g.base_signals(N).astype(rdt)
    idx = index(B)
    X = g.tile(Xb, idx)
    small = cwt_host(Xb, na, nv)
    big = cwt_host(X, na, nv)
    for k, (a, s) in enumerate(zip(big, small)):
        g.assert_repeats(a, s, idx, "lmssq_cwt host plane %d" % k)
    for b in (0, g.LIMIT // na, g.LIMIT // na + 1, g.LIMIT - 1, g.LIMIT, B - 1):  # rows and signals on either side of 65535
        one = cwt_host(X[b], na, nv)
        for k in range(4):
            assert np.array_equal(big[k][b], one[k]), (b, k)
    assert (small[3] >= 0).any()
    dev = cwt_exec(X, na, nv)
    for k, (a, s) in enumerate(zip(dev, big)):
        g.assert_same(a, s, "lmssq_cwt device plane %d against the host call's" % k)
