#!/usr/bin/env python
"""Kernel time of the reassigned scalogram (`ssq_reassign_cwt_exec`: padding, the forward transform, three product
spectra and inverse transforms a row, the operator, the scatter and the read-out; HIP events around the launches,
everything resident on the device) beside the second-order synchrosqueezed CWT (`ssq_ssq_cwt2_exec`, five inverse
transforms a row) at the same shape on the same run, and the scatter kernel alone with its rate of 64-bit integer
atomic adds to device memory (one per kept bin).

    python tools/bench_reassign_cwt.py [--batch 4] [--n 65536] [--na 128] [--reps 9] [--out FILE]

GMW(3, 60), log scales from the Nyquist peak down to N/4 samples per cycle (tools/bench_cwt_sst2.py's grids).  Per dtype
and signal: median and min..max over `--reps` runs after two warm-up runs.  The signals set the scatter's address
pattern: 'noise' (targets spread over a few cells around every source), 'chirp' (a wave's 64 lanes add to consecutive
cells of a row or two) and 'impulse' (every lane of a wave adds to the one column of the impulse: same-address adds,
the slow case)."""
import argparse
import ctypes as C
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from ssqueeze_rs_amd import _lib  # noqa: E402

GAMMA, BETA = 3.0, 60.0


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _stats(ts):
    return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]


def _grids(N, na):
    wc = (BETA / GAMMA) ** (1 / GAMMA)
    scales = wc / np.pi * 2.0 ** np.linspace(0, np.log2(N / 8), na)
    nv = 1.0 / np.diff(np.log2(scales))[0]
    f = (1.0 / N) * np.power(N / 2.0, np.arange(na) / (na - 1))      # 'maximal' log frequencies
    return np.ascontiguousarray(scales), np.full(na, np.log(2) / nv), np.ascontiguousarray(f)


def signals(B, N, dt):
    rng = np.random.default_rng(0)
    t = np.arange(N, dtype=np.float64)
    chirp = np.cos(2 * np.pi * (0.02 * t + 0.5 * (0.43 / N) * t * t))
    imp = np.zeros((B, N))
    imp[:, N // 2] = 1.0
    return {"noise": rng.standard_normal((B, N)).astype(dt), "chirp": np.tile(chirp, (B, 1)).astype(dt),
            "impulse": imp.astype(dt)}


def _run(x, na, reps, which):
    """-> ([median, min, max] of every float of kernel_ms, workspace bytes, kept bins or None)."""
    lib = _lib.load()
    B, N = x.shape
    code = _lib.SSQ_F32 if x.dtype == np.float32 else _lib.SSQ_F64
    scales, rc, f = _grids(N, na)
    cells = B * na * N
    cbytes, rbytes = cells * 2 * x.dtype.itemsize, cells * x.dtype.itemsize
    if which == "reassign":
        ws = int(lib.ssq_reassign_cwt_workspace_bytes(code, B, N, na, None))
        sizes = (x.nbytes, rbytes, cbytes, 4 * cells, ws)              # x, Rx, Wx, kk, workspace
    else:
        ws = int(lib.ssq_ssq_cwt2_workspace_bytes(code, B, N, na, None))
        sizes = (x.nbytes, cbytes, cbytes, rbytes, ws)                 # x, Tx, Wx, w2, workspace
    bufs = [C.c_void_p() for _ in sizes]
    kept = None
    try:
        for d, n in zip(bufs, sizes):
            _lib.check(lib.ssq_dev_malloc(C.byref(d), n))
        _lib.check(lib.ssq_memcpy_h2d(bufs[0], _vp(x), x.nbytes, None))
        ms, ts = (C.c_float * 2)(), []
        for i in range(2 + reps):
            if which == "reassign":
                _lib.check(lib.ssq_reassign_cwt_exec(code, bufs[0], B, N, 0, GAMMA, BETA, _vp(scales), na, 1.0, _vp(f), 0, 0, 0,
                                                     -1.0, 4, bufs[1], bufs[2], None, None, bufs[3], None, bufs[4], ws, None,
                                                     ms))
            else:
                _lib.check(lib.ssq_ssq_cwt2_exec(code, bufs[0], B, N, 0, GAMMA, BETA, _vp(scales), na, 1.0, _vp(rc), _vp(f), 0,
                                                 0, 0, 0, -1.0, 4, bufs[1], bufs[2], bufs[3], bufs[4], ws, None, ms))
            if i >= 2:
                ts.append((ms[0], ms[1]))
        if which == "reassign":
            kk = np.empty(cells, dtype=np.int32)
            _lib.check(lib.ssq_memcpy_d2h(_vp(kk), bufs[3], kk.nbytes, None))
            _lib.check(lib.ssq_device_sync())
            kept = int((kk >= 0).sum())
    finally:
        for d in bufs:
            if d:
                lib.ssq_dev_free(d)
    return [_stats([t[k] for t in ts]) for k in range(2)], ws, kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--n", type=int, default=1 << 16)
    ap.add_argument("--na", type=int, default=128)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    lines = []
    for dt in (np.float32, np.float64):
        for name, x in signals(a.batch, a.n, dt).items():
            (total, scat), ws, kept = _run(x, a.na, a.reps, "reassign")
            rec = dict(dtype=np.dtype(dt).name, signal=name, batch=a.batch, n=a.n, na=a.na, reps=a.reps,
                       reassign_cwt_kernels_ms=total, scatter_ms=scat, kept_bins=kept,
                       atomics_per_s=float("%.4g" % (kept / (scat[0] * 1e-3))) if scat[0] > 0 else None,
                       reassign_cwt_workspace_MB=round(ws / 2 ** 20, 1))
            if name == "noise":
                (t2, _), ws2, _ = _run(x, a.na, a.reps, "cwt2")
                rec.update(ssq_cwt2_kernels_ms=t2, ssq_cwt2_workspace_MB=round(ws2 / 2 ** 20, 1),
                           ratio_to_ssq_cwt2=round(total[0] / t2[0], 3))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_reassign_cwt.py: [median, min, max] ms over the timed runs; scatter_ms: the scatter kernel "
                    "alone (one 64-bit integer atomic add to device memory per kept bin); ratio_to_ssq_cwt2: all kernels, "
                    "same shape, same run\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
