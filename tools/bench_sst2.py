#!/usr/bin/env python
"""Kernel time of the second-order synchrosqueezed STFT (`ssq_ssq_stft2_exec`: clearing Tx, the operator kernel and the
scatter, HIP events around the launches, everything resident on the device) next to the first-order fused kernel
(`SsqStftBatch`'s plan, HIP events around `ssq_stft_plan_exec`) at the same shape.

    python tools/bench_sst2.py [--batch 64] [--n 262144] [--n-fft 1024] [--hop 256] [--reps 9] [--out FILE]

Per dtype: median and min..max over `--reps` runs after two warm-up runs.  The second-order call writes Sx, the map
(w2, bin) and Tx; the first-order one writes Tx alone, so the two are not the same traffic."""
import argparse
import ctypes as C
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from ssqueeze_rs_amd import _lib  # noqa: E402
from ssqueeze_rs_amd.batch import SsqStftBatch  # noqa: E402


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _stats(ts):
    return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]


def second_order(x, win, n_fft, hop, reps):
    lib = _lib.load()
    B, N = x.shape
    code = _lib.SSQ_F32 if x.dtype == np.float32 else _lib.SSQ_F64
    F, nfr = n_fft // 2 + 1, (N - 1) // hop + 1
    map_bytes = B * F * nfr * 2 * x.dtype.itemsize
    ws = int(lib.ssq_ssq_stft2_workspace_bytes(code, B, N, n_fft, hop))
    bufs = [C.c_void_p() for _ in range(4)]
    d_x, d_Tx, d_Sx, d_ws = bufs
    try:
        for d, n in zip(bufs, (x.nbytes, map_bytes, map_bytes, ws)):
            _lib.check(lib.ssq_dev_malloc(C.byref(d), n))
        _lib.check(lib.ssq_memcpy_h2d(d_x, _vp(x), x.nbytes, None))
        ms, ts = C.c_float(0), []
        for i in range(2 + reps):
            _lib.check(lib.ssq_ssq_stft2_exec(code, d_x, B, N, _vp(win), n_fft, hop, 1.0, 0, 0, -1.0, 3, d_Tx, d_Sx, None,
                                              d_ws, ws, C.byref(ms)))
            if i >= 2:
                ts.append(ms.value)
    finally:
        for d in bufs:
            if d:
                lib.ssq_dev_free(d)
    return _stats(ts)


def first_order(x, win, n_fft, hop, reps):
    lib = _lib.load()
    B, N = x.shape
    p = SsqStftBatch(N, win, n_fft, hop, dtype=x.dtype, max_batch=B)
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    try:
        _lib.check(lib.ssq_event_create(C.byref(ev0)))
        _lib.check(lib.ssq_event_create(C.byref(ev1)))
        _lib.check(lib.ssq_memcpy_h2d(p.d_x, _vp(x), x.nbytes, None))
        ms, ts = C.c_float(0), []
        for i in range(2 + reps):
            _lib.check(lib.ssq_event_record(ev0, None))
            _lib.check(lib.ssq_stft_plan_exec(p.plan, _lib.OUT_TX, p.d_x, B, p.d_out, p.d_ws, p.ws_bytes, None))
            _lib.check(lib.ssq_event_record(ev1, None))
            _lib.check(lib.ssq_event_sync(ev1))
            _lib.check(lib.ssq_event_elapsed_ms(ev0, ev1, C.byref(ms)))
            if i >= 2:
                ts.append(ms.value)
    finally:
        for e in (ev0, ev1):
            if e:
                lib.ssq_event_destroy(e)
        p.close()
    return _stats(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--n-fft", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    u = np.arange(a.n_fft) - a.n_fft // 2
    win = np.exp(-0.5 * (u / (a.n_fft / 10.0)) ** 2)
    lines = []
    for dt in (np.float32, np.float64):
        x = rng.standard_normal((a.batch, a.n)).astype(dt)
        rec = dict(dtype=np.dtype(dt).name, batch=a.batch, n=a.n, n_fft=a.n_fft, hop=a.hop, reps=a.reps,
                   ssq_stft2_kernels_ms=second_order(x, win, a.n_fft, a.hop, a.reps),
                   ssq_stft_fused_ms=first_order(x, win, a.n_fft, a.hop, a.reps))
        rec["ratio"] = round(rec["ssq_stft2_kernels_ms"][0] / rec["ssq_stft_fused_ms"][0], 2)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_sst2.py: [median, min, max] ms over the timed runs; ratio = second order / first order\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
