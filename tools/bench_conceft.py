#!/usr/bin/env python
"""Kernel time of ConceFT's fused squeeze (`ssq_conceft_cwt_exec`, its kernel_ms: the stage-2 kernel alone, HIP events
around its launches, everything resident on the device) beside what the same M squeezes cost before it existed:

    (a) conceft_kernel_ms   the fused kernel: the 2 J planes read once per chunk of 8 draws, every draw combined, binned
                            and summed in registers, one Tx written
    (b) m_squeezes_ms       M x the time of `ssq_ssqueeze_dwx_exec` on ONE device-resident plane pair of the same shape
                            (its clear of Tx and its kernel, HIP events): the M squeezes alone, the combinations free
    (c) python_loop_s       the wall clock of the loop a user had to write: `cwt_higher_order(..., average=False,
                            derivative=True)` to the host, the combinations in numpy, `upstream.ssqueeze(W, dWx=dW)` per
                            draw, the sum; measured at `--loop-draws` draws (once: it is seconds long) and linear in M

    python tools/bench_conceft.py [--batch 4] [--n 65536] [--na 128] [--nv 16] [--orders 3] [--reps 7] [--out FILE]

GMW(3, 60), log scales from the Nyquist peak at nv 16, M in {8, 20, 64}, float32 and float64.  The signals are a chirp
(long runs of rows in one bin: the best case for combining runs) and white noise (the worst).  Per dtype, signal and M:
median and min..max over `--reps` repeats after two warm-up runs, (a) and (b) alternating inside every repeat."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from ssqueeze_rs_amd import _lib  # noqa: E402
from ssqueeze_rs_amd import upstream as up  # noqa: E402

GAMMA, BETA = 3.0, 60.0
GMW = ("gmw", {"gamma": GAMMA, "beta": BETA})
DRAWS = (8, 20, 64)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _stats(ts):
    return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]


def signals(batch, n, dtype):
    t = np.arange(n, dtype=np.float64)
    chirp = np.cos(2 * np.pi * (0.02 * t + 0.5 * (0.4 / n) * t * t))
    rng = np.random.default_rng(0)
    return {"chirp": np.ascontiguousarray(np.tile(chirp, (batch, 1)).astype(dtype)),
            "noise": np.ascontiguousarray(rng.standard_normal((batch, n)).astype(dtype))}


class DevBufs:
    def __init__(self, lib, sizes):
        self.lib, self.bufs = lib, [C.c_void_p() for _ in sizes]
        for d, n in zip(self.bufs, sizes):
            _lib.check(lib.ssq_dev_malloc(C.byref(d), int(n)))

    def free(self):
        for d in self.bufs:
            if d:
                self.lib.ssq_dev_free(d)


def run(x, na, nv, J, reps):
    """-> {M: ((a) stats, (b) stats)} in ms."""
    lib = _lib.load()
    B, N = x.shape
    f32 = x.dtype == np.float32
    code = _lib.SSQ_F32 if f32 else _lib.SSQ_F64
    csz = 8 if f32 else 16
    scales = (BETA / GAMMA) ** (1 / GAMMA) / np.pi * 2.0 ** (np.arange(na) / nv)
    wcode, p0, p1 = up._wavelet(GMW)
    s, rc, f, kind, f_idx = up._cwt_freq_grid(scales, None, None, "peak", N, wcode, p0, p1, 1.0)
    adm = np.array([up.gmw_adm_ssq(GAMMA, BETA, k) for k in range(J)])
    polys = np.ascontiguousarray(up.gmw_order_coefficients(p0, p1, range(J), average=False))
    mn = C.c_int64(0)
    ws = int(lib.ssq_conceft_cwt_workspace_bytes(code, B, N, na, J, C.byref(mn)))
    per_slice = min(B, ws // mn.value)
    last = B - ((B - 1) // per_slice) * per_slice          # signals of the last slice: its planes stay in the workspace
    cells = B * na * N
    rcT = np.ascontiguousarray(rc.astype(x.dtype))
    d = DevBufs(lib, (x.nbytes, cells * csz, ws, rcT.nbytes, na * N * csz))   # x, Tx, workspace, row weights, the pair's Tx
    out = {}
    try:
        dx, dTx, dwork, drc, dT2 = d.bufs
        _lib.check(lib.ssq_memcpy_h2d(dx, _vp(x), x.nbytes, None))
        _lib.check(lib.ssq_memcpy_h2d(drc, _vp(rcT), rcT.nbytes, None))
        ev = [C.c_void_p() for _ in range(2)]
        for e in ev:
            _lib.check(lib.ssq_event_create(C.byref(e)))
        for M in DRAWS:
            r, c = up._conceft_gauge(up.conceft_vectors(M, J, 0, adm), adm)
            scale = float(adm[0] / c.sum())
            ms = C.c_float(0)
            ta, tb = [], []
            for i in range(2 + reps):
                _lib.check(lib.ssq_conceft_cwt_exec(code, dx, B, N, p0, p1, _vp(polys), polys.shape[1], J, _vp(r), M, scale,
                                                    _vp(s), na, 1.0, _vp(rc), _vp(f), up.FREQS[kind], f_idx or 0, 0, -1.0,
                                                    up.VARIANT_FLIPUD, dTx, None, None, dwork, ws, None, C.byref(ms)))
                # the parent's squeeze of ONE resident plane pair [na, N]: the order-0 W and dW of the last slice's first
                # signal, where stage 1 left them in the workspace (W of the slice, then dW of the slice)
                W0 = dwork
                dW0 = C.c_void_p(dwork.value + last * J * na * N * csz)
                _lib.check(lib.ssq_event_record(ev[0], None))
                _lib.check(lib.ssq_ssqueeze_dwx_exec(code, W0, dW0, None, 1, na, N, drc, _vp(f), up.FREQS[kind],
                                                     f_idx or 0, 0, 1, 10 * float(np.finfo(x.dtype).eps), dT2, None))
                _lib.check(lib.ssq_event_record(ev[1], None))
                _lib.check(lib.ssq_event_sync(ev[1]))
                one = C.c_float(0)
                _lib.check(lib.ssq_event_elapsed_ms(ev[0], ev[1], C.byref(one)))
                if i >= 2:
                    ta.append(ms.value)
                    tb.append(one.value * B * M)               # one signal's plane pair x the batch x the draws
            out[M] = (_stats(ta), _stats(tb))
        for e in ev:
            lib.ssq_event_destroy(e)
    finally:
        d.free()
    return out


def python_loop(x, na, nv, J, M):
    """The loop of the issue, end to end on the host side -> seconds."""
    B, N = x.shape
    scales = (BETA / GAMMA) ** (1 / GAMMA) / np.pi * 2.0 ** (np.arange(na) / nv)
    adm = np.array([up.gmw_adm_ssq(GAMMA, BETA, k) for k in range(J)])
    r, c = up._conceft_gauge(up.conceft_vectors(M, J, 0, adm), adm)
    t0 = time.perf_counter()
    W, _, dW = up.cwt_higher_order(x, GMW, order=range(J), average=False, derivative=True, scales=scales)
    Tx = None
    for m in range(M):
        Wm = sum(r[m, j].astype(W[0].dtype) * W[j] for j in range(J))
        dWm = sum(r[m, j].astype(W[0].dtype) * dW[j] for j in range(J))
        T, _ = up.ssqueeze(Wm, dWx=dWm, scales=scales, wavelet=GMW, maprange="peak", flipud=True)
        Tx = T if Tx is None else Tx + T
    Tx *= adm[0] / c.sum()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--n", type=int, default=1 << 16)
    ap.add_argument("--na", type=int, default=128)
    ap.add_argument("--nv", type=int, default=16)
    ap.add_argument("--orders", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop-draws", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    lines = []
    for dt in (np.float32, np.float64):
        for name, x in signals(a.batch, a.n, dt).items():
            res = run(x, a.na, a.nv, a.orders, a.reps)
            loop_s = python_loop(x, a.na, a.nv, a.orders, a.loop_draws) if a.loop_draws > 0 else None
            for M in DRAWS:
                ka, kb = res[M]
                rec = dict(dtype=np.dtype(dt).name, signal=name, batch=a.batch, n=a.n, na=a.na, orders=a.orders, draws=M,
                           reps=a.reps, conceft_kernel_ms=ka, m_squeezes_ms=kb,
                           ratio_b_over_a=round(kb[0] / ka[0], 2) if ka[0] > 0 else None)
                if loop_s is not None and M == a.loop_draws:
                    rec["python_loop_s"] = round(loop_s, 2)
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_conceft.py: [median, min, max] over the timed repeats.  conceft_kernel_ms (a): the fused "
                    "squeeze kernel of ssq_conceft_cwt_exec alone.  m_squeezes_ms (b): batch x draws x the time of "
                    "ssq_ssqueeze_dwx_exec (clear + kernel) on one resident [na, n] plane pair, measured in the same repeat.  "
                    "ratio_b_over_a: the medians.  python_loop_s (c): wall clock of cwt_higher_order to the host, numpy "
                    "combinations and one upstream.ssqueeze per draw, once, at the draws of that line.\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
