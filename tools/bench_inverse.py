#!/usr/bin/env python
"""Timing of the batched `upstream.istft` against a Python loop of 2-D calls (the only way before the batch entry
point existed): host arrays in and out and, separately, the kernels alone on device-resident buffers, fused kernel
against the three-kernel path, with the Sx-read roofline of each shape beside them.

    python tools/bench_inverse.py [--n 1048576] [--n-fft 1024] [--hops 256,16] [--batches 1,16] [--reps 7]

Per (dtype, hop, B): median and min..max over `--reps` timed runs after two warm-up runs of each side.  The host
figures include the host-to-device copy of Sx, which dominates them.  The kernel figures (`--kernel-only` prints
only those) come from `ssq_istft_batch_exec`: HIP events around the launches, Sx and x resident on the device, tables
and workspace set up before the first event.  The roofline is (bytes of Sx + bytes of x) / HBM rate, 8 TB/s peak as
in DESIGN 4.x; `fused_frac` is roofline / fused kernel time."""
import ctypes as C
import argparse
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from ssqueeze_rs_amd import _lib, upstream as up  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def _time(fn, reps):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def _kernel_ms(lib, code, d_S, B, nfr, win, n_fft, hop, n, path, d_x, reps):
    ms = C.c_float(0)
    ts = []
    for i in range(2 + reps):
        _lib.check(lib.ssq_istft_batch_exec(code, d_S, B, nfr, win.ctypes.data_as(C.c_void_p), n_fft, hop, n, 1, 1, path,
                                            d_x, C.byref(ms)))
        if i >= 2:
            ts.append(ms.value)
    return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]


def kernels(S, win, n_fft, hop, n, reps):
    """Fused kernel and three-kernel path on the same device-resident Sx [B, n_fft//2+1, n_frames] -> dict of ms."""
    lib = _lib.load()
    code = _lib.SSQ_F32 if S.dtype == np.complex64 else _lib.SSQ_F64
    B, _, nfr = S.shape
    d_S, d_x = C.c_void_p(), C.c_void_p()
    x_bytes = B * n * S.dtype.itemsize // 2
    _lib.check(lib.ssq_dev_malloc(C.byref(d_S), S.nbytes))
    try:
        _lib.check(lib.ssq_dev_malloc(C.byref(d_x), x_bytes))
        _lib.check(lib.ssq_memcpy_h2d(d_S, S.ctypes.data_as(C.c_void_p), S.nbytes, None))
        _lib.check(lib.ssq_device_sync())
        out = {}
        for name, path in (("fused", 1), ("three", 0)):
            out[name] = _kernel_ms(lib, code, d_S, B, nfr, win, n_fft, hop, n, path, d_x, reps)
        return out
    finally:
        lib.ssq_dev_free(d_x)
        lib.ssq_dev_free(d_S)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--n-fft", type=int, default=1024)
    ap.add_argument("--hops", default="256,16")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    win = np.hanning(a.n_fft) + 0.1
    for cdt in (np.complex64, np.complex128):
        for hop in [int(h) for h in a.hops.split(",")]:
            nfr = (a.n - 1) // hop + 1
            nf = a.n_fft // 2 + 1
            for B in [int(b) for b in a.batches.split(",")]:
                if B * nf * nfr * np.dtype(cdt).itemsize > 24e9:
                    print(json.dumps({"dtype": np.dtype(cdt).name, "hop": hop, "B": B, "skipped": "Sx over 24 GB of host memory"}))
                    continue
                S = (rng.standard_normal((B, nf, nfr), dtype=np.float32) + 1j).astype(cdt)
                kw = dict(n_fft=a.n_fft, hop_len=hop, N=a.n)
                sx_b, x_b = S.nbytes, B * a.n * np.dtype(cdt).itemsize // 2
                roof = 1e3 * (sx_b + x_b) / HBM_BYTES_PER_S
                row = {"dtype": np.dtype(cdt).name, "n": a.n, "n_fft": a.n_fft, "hop": hop, "B": B}
                if not a.kernel_only:
                    loop = _time(lambda: [up.istft(S[b], win, **kw) for b in range(B)], a.reps)
                    batch = _time(lambda: up.istft(S, win, **kw), a.reps)
                    row.update({"loop_2d_ms": [round(1e3 * v, 3) for v in loop],
                                "batched_ms": [round(1e3 * v, 3) for v in batch],
                                "speedup_median": round(loop[0] / batch[0], 3)})
                k = kernels(S, win, a.n_fft, hop, a.n, a.reps)
                row.update({"kernel_fused_ms": k["fused"], "kernel_three_ms": k["three"],
                            "kernel_speedup_median": round(k["three"][0] / k["fused"][0], 3),
                            "roofline_ms": round(roof, 4), "fused_frac": round(roof / k["fused"][0], 4)})
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
