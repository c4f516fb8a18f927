"""Time ssq_issq_components_exec (issq_components.hip) with HIP events: F = 256 rows, N = 2**16 columns, B = 1 and
B = 64 signals, fp32 and fp64, K = 1 and 4 curves of half-width 8.  Prints one JSON line per case with the bytes the
kernel must move (Tx once, cc and cw, the float64 output) and the rate against the 8 TB/s HBM peak and the ~6.3 TB/s
a streaming copy reaches.

    python tools/bench_components.py [--reps 5] [--n 65536] [--f 256] [--batches 1,64] [--ks 1,4]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssqueeze_rs_amd import _lib  # noqa: E402

PEAK_TBS, STREAM_TBS = 8.0, 6.3


def _ok(rc):
    _lib.check(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 16)
    ap.add_argument("--f", type=int, default=256)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--ks", default="1,4")
    ap.add_argument("--cw", type=int, default=8)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    F, N = a.f, a.n
    rng = np.random.default_rng(0)
    for dt, code in ((np.complex64, _lib.SSQ_F32), (np.complex128, _lib.SSQ_F64)):
        one = np.ascontiguousarray((rng.standard_normal((F, N)) + 1j * rng.standard_normal((F, N))).astype(dt))
        for B in (int(b) for b in a.batches.split(",")):
            for K in (int(k) for k in a.ks.split(",")):
                cc = np.ascontiguousarray(rng.integers(0, F, size=(B, N, K)), dtype=np.int64)
                cw = np.full_like(cc, a.cw)
                ptrs = []

                def alloc(n):
                    p = C.c_void_p()
                    _ok(lib.ssq_dev_malloc(C.byref(p), int(n)))
                    ptrs.append(p)
                    return p
                try:
                    dT = alloc(one.nbytes * B)
                    for b in range(B):
                        _ok(lib.ssq_memcpy_h2d(C.c_void_p(dT.value + b * one.nbytes), one.ctypes.data_as(C.c_void_p),
                                               one.nbytes, None))
                    dcc, dcw = alloc(cc.nbytes), alloc(cw.nbytes)
                    _ok(lib.ssq_memcpy_h2d(dcc, cc.ctypes.data_as(C.c_void_p), cc.nbytes, None))
                    _ok(lib.ssq_memcpy_h2d(dcw, cw.ctypes.data_as(C.c_void_p), cw.nbytes, None))
                    x_bytes = 8 * B * (K + 1) * N
                    dx = alloc(x_bytes)
                    ev0, ev1 = C.c_void_p(), C.c_void_p()
                    _ok(lib.ssq_event_create(C.byref(ev0)))
                    _ok(lib.ssq_event_create(C.byref(ev1)))

                    def run():
                        _ok(lib.ssq_issq_components_exec(code, dT, B, F, N, dcc, dcw, 0, K, 1.0, dx, None))
                    run()
                    _ok(lib.ssq_device_sync())
                    times = []
                    for _ in range(a.reps):
                        _ok(lib.ssq_event_record(ev0, None))
                        run()
                        _ok(lib.ssq_event_record(ev1, None))
                        _ok(lib.ssq_event_sync(ev1))
                        ms = C.c_float()
                        _ok(lib.ssq_event_elapsed_ms(ev0, ev1, C.byref(ms)))
                        times.append(ms.value)
                    lib.ssq_event_destroy(ev0)
                    lib.ssq_event_destroy(ev1)
                    moved = one.nbytes * B + cc.nbytes + cw.nbytes + x_bytes
                    ms = float(np.median(times))
                    tbs = moved / (ms * 1e-3) / 1e12
                    print(json.dumps({"dtype": np.dtype(dt).name, "F": F, "N": N, "B": B, "K": K, "cw": a.cw,
                                      "ms_median": round(ms, 4), "ms_all": [round(t, 4) for t in times],
                                      "bytes": int(moved), "tb_s": round(tbs, 3),
                                      "of_peak_8": round(tbs / PEAK_TBS, 3),
                                      "of_stream_6_3": round(tbs / STREAM_TBS, 3)}), flush=True)
                finally:
                    for p in ptrs:
                        lib.ssq_dev_free(p)


if __name__ == "__main__":
    main()
