#!/usr/bin/env python
"""Kernel time of the time-reassigned synchrosqueezed CWT (`ssq_tssq_cwt_exec`: padding, the forward transform, two
(order 1) or five (order 2) product spectra and inverse transforms a row, the operator, the scatter and the read-out; HIP
events around the launches, everything resident on the device) beside the second-order synchrosqueezed CWT
(`ssq_ssq_cwt2_exec`, five inverse transforms a row) and the reassigned scalogram (`ssq_reassign_cwt_exec`, three) at the
same shape on the same run, and the scatter kernel alone with its rate of fixed-point parts added (two per kept bin; the
kernel merges a wave's adjacent lanes that name one cell before the 64-bit integer atomic adds to device memory, so the
adds it issues are fewer).

    python tools/bench_tssq_cwt.py [--batch 4] [--n 65536] [--na 128] [--reps 9] [--out FILE]

GMW(3, 60), log scales from the Nyquist peak down to N/4 samples per cycle (tools/bench_reassign_cwt.py's grids and
signals).  Per dtype, signal and order: median and min..max over `--reps` runs after two warm-up runs.  The signals set
the scatter's address pattern: 'noise' (targets spread over a few cells around every source), 'chirp' (order 2: a row's
sources add to the few columns where the sweep crosses it) and 'impulse' (every lane of a wave names the one column of
the impulse: one run of 64)."""
import argparse
import ctypes as C
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from ssqueeze_rs_amd import _lib  # noqa: E402
from tools.bench_reassign_cwt import BETA, GAMMA, _grids, _run, signals  # noqa: E402


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _stats(ts):
    return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]


def _run_tssq(x, na, reps, order):
    """-> ([median, min, max] of the three floats of kernel_ms, workspace bytes, kept bins)."""
    lib = _lib.load()
    B, N = x.shape
    code = _lib.SSQ_F32 if x.dtype == np.float32 else _lib.SSQ_F64
    scales = _grids(N, na)[0]
    nu = np.ascontiguousarray((BETA / GAMMA) ** (1 / GAMMA) / (2 * np.pi * scales))
    cells = B * na * N
    cbytes = cells * 2 * x.dtype.itemsize
    ws = int(lib.ssq_tssq_cwt_workspace_bytes(code, B, N, na, order, None))
    sizes = (x.nbytes, cbytes, cbytes, 4 * cells, ws)                  # x, Tx, Wx, mm, workspace
    bufs = [C.c_void_p() for _ in sizes]
    try:
        for d, n in zip(bufs, sizes):
            _lib.check(lib.ssq_dev_malloc(C.byref(d), n))
        _lib.check(lib.ssq_memcpy_h2d(bufs[0], _vp(x), x.nbytes, None))
        ms, ts = (C.c_float * 3)(), []
        for i in range(2 + reps):
            _lib.check(lib.ssq_tssq_cwt_exec(code, bufs[0], B, N, 0, GAMMA, BETA, _vp(scales), _vp(nu), na, 1.0, 0, order, -1.0,
                                             bufs[1], bufs[2], None, bufs[3], bufs[4], ws, None, ms))
            if i >= 2:
                ts.append((ms[0], ms[1], ms[2]))
        mm = np.empty(cells, dtype=np.int32)
        _lib.check(lib.ssq_memcpy_d2h(_vp(mm), bufs[3], mm.nbytes, None))
        _lib.check(lib.ssq_device_sync())
        kept = int((mm >= 0).sum())
    finally:
        for d in bufs:
            if d:
                lib.ssq_dev_free(d)
    return [_stats([t[k] for t in ts]) for k in range(3)], ws, kept


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
            rec = dict(dtype=np.dtype(dt).name, signal=name, batch=a.batch, n=a.n, na=a.na, reps=a.reps)
            for order in (1, 2):
                (total, scat, before), ws, kept = _run_tssq(x, a.na, a.reps, order)
                rec.update({"order%d_kernels_ms" % order: total, "order%d_before_scatter_ms" % order: before,
                            "order%d_scatter_ms" % order: scat, "order%d_kept_bins" % order: kept,
                            "order%d_adds_per_s" % order: float("%.4g" % (2 * kept / (scat[0] * 1e-3))) if scat[0] > 0 else None,
                            "order%d_workspace_MB" % order: round(ws / 2 ** 20, 1)})
            (tr, sr), wsr, keptr = _run(x, a.na, a.reps, "reassign")
            rec.update(reassign_cwt_kernels_ms=tr, reassign_cwt_scatter_ms=sr, reassign_cwt_kept_bins=keptr,
                       reassign_cwt_adds_per_s=float("%.4g" % (keptr / (sr[0] * 1e-3))) if sr[0] > 0 else None)
            if name == "noise":
                (t2, _), ws2, _ = _run(x, a.na, a.reps, "cwt2")
                rec.update(ssq_cwt2_kernels_ms=t2)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_tssq_cwt.py: [median, min, max] ms over the timed runs; orderK_before_scatter_ms: padding, "
                    "transforms, spectra and operator; orderK_scatter_ms: the scatter kernel alone; orderK_adds_per_s: two fixed-"
                    "point parts a kept bin over that time (runs of adjacent lanes on one cell are merged before the 64-bit "
                    "integer atomic adds to device memory); reassign_cwt_* and ssq_cwt2_*: the siblings at the same shape in the "
                    "same run (reassign_cwt_kernels_ms less its scatter_ms still holds its read-out)\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
