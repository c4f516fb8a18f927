#!/usr/bin/env python
"""Kernel time of the second-order synchrosqueezed CWT (`ssq_ssq_cwt2_exec`: padding, the forward transform, the product
spectra, the inverse transforms, the operator and the scatter; HIP events around the launches, everything resident on
the device), and for float64 the wall time of the Python call `upstream.ssq_cwt2` next to the first-order
`upstream.ssq_cwt` at the same shape (host arrays in and out: the transfers are inside both).

    python tools/bench_cwt_sst2.py [--batch 4] [--n 65536] [--na 128] [--reps 9] [--out FILE]

GMW(3, 60), log scales from the Nyquist peak down to N/4 samples per cycle.  Per dtype: median and min..max over
`--reps` runs after two warm-up runs.  The second-order call writes Wx, w2 and Tx and moves five inverse transforms per
row through its workspace."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time

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


def second_order(x, na, reps):
    lib = _lib.load()
    B, N = x.shape
    code = _lib.SSQ_F32 if x.dtype == np.float32 else _lib.SSQ_F64
    scales, rc, f = _grids(N, na)
    map_bytes = B * na * N * 2 * x.dtype.itemsize
    ws = int(lib.ssq_ssq_cwt2_workspace_bytes(code, B, N, na, None))
    bufs = [C.c_void_p() for _ in range(5)]
    d_x, d_Tx, d_Wx, d_w2, d_ws = bufs
    try:
        for d, n in zip(bufs, (x.nbytes, map_bytes, map_bytes, map_bytes // 2, ws)):
            _lib.check(lib.ssq_dev_malloc(C.byref(d), n))
        _lib.check(lib.ssq_memcpy_h2d(d_x, _vp(x), x.nbytes, None))
        ms, ts = C.c_float(0), []
        for i in range(2 + reps):
            _lib.check(lib.ssq_ssq_cwt2_exec(code, d_x, B, N, 0, GAMMA, BETA, _vp(scales), na, 1.0, _vp(rc), _vp(f), 0, 0, 0, 0,
                                             -1.0, 4, d_Tx, d_Wx, d_w2, d_ws, ws, None, C.byref(ms)))
            if i >= 2:
                ts.append(ms.value)
    finally:
        for d in bufs:
            if d:
                lib.ssq_dev_free(d)
    return _stats(ts), ws


def host_calls(x, na, reps):
    """Wall time of the two Python calls, host arrays in and out (PCIe both ways inside): `upstream.ssq_cwt2` and the
    first-order `upstream.ssq_cwt`, whose upstream-variant plan takes its frequencies through the host entry only."""
    from ssqueeze_rs_amd import upstream as up
    scales, _, _ = _grids(x.shape[1], na)
    kw = dict(wavelet=("gmw", {"gamma": GAMMA, "beta": BETA}), scales=scales, maprange="maximal")
    out = []
    for fn in (up.ssq_cwt2, up.ssq_cwt):
        ts = []
        for i in range(2 + reps):
            t0 = time.perf_counter()
            fn(x, **kw)
            if i >= 2:
                ts.append((time.perf_counter() - t0) * 1e3)
        out.append(_stats(ts))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--n", type=int, default=1 << 16)
    ap.add_argument("--na", type=int, default=128)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    lines = []
    for dt in (np.float32, np.float64):
        x = rng.standard_normal((a.batch, a.n)).astype(dt)
        t2, ws = second_order(x, a.na, a.reps)
        rec = dict(dtype=np.dtype(dt).name, batch=a.batch, n=a.n, na=a.na, reps=a.reps, ssq_cwt2_kernels_ms=t2,
                   ssq_cwt2_workspace_MB=round(ws / 2 ** 20, 1))
        if dt == np.float64:
            rec["ssq_cwt2_host_call_ms"], rec["ssq_cwt_host_call_ms"] = host_calls(x, a.na, a.reps)
            rec["host_call_ratio"] = round(rec["ssq_cwt2_host_call_ms"][0] / rec["ssq_cwt_host_call_ms"][0], 2)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_cwt_sst2.py: [median, min, max] ms over the timed runs; host_call_ratio = second order / first order, wall time of the Python calls (fp64)\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
