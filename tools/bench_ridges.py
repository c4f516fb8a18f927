"""Time ssq_ridges_exec (ridge.hip) with HIP events: F = 256 rows, N = 2**16 columns, B = 1 and B = 256 signals, fp32
and fp64, one ridge, on real input (|x|**2 is one multiply, so the time is the DP's).  Prints one JSON line per case
with the forward DP's VALU bound for comparison: F*F pairs * k ops / (128 lanes-ops per CU-cycle) per step at 2.4 GHz,
k = 5 (sub, mul, mul, add, min) for the recomputed penalty, fp64 at half the fp32 rate.

    python tools/bench_ridges.py [--reps 3] [--n 65536] [--f 256] [--batches 1,256]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssqueeze_rs_amd import _lib  # noqa: E402


def _ok(rc):
    _lib.check(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", type=int, default=1 << 16)
    ap.add_argument("--f", type=int, default=256)
    ap.add_argument("--batches", default="1,256")
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    F, N = a.f, a.n
    rng = np.random.default_rng(0)
    for dt, code in ((np.float32, _lib.SSQ_F32), (np.float64, _lib.SSQ_F64)):
        x = np.ascontiguousarray(rng.standard_normal((F, N)).astype(dt))
        metric = np.log(np.exp(np.linspace(0.5, 6, F))).astype(dt)
        for B in (int(b) for b in a.batches.split(",")):
            ptrs = []

            def alloc(n):
                p = C.c_void_p()
                _ok(lib.ssq_dev_malloc(C.byref(p), int(n)))
                ptrs.append(p)
                return p
            try:
                dT = alloc(x.nbytes * B)
                for b in range(B):
                    _ok(lib.ssq_memcpy_h2d(C.c_void_p(dT.value + b * x.nbytes), x.ctypes.data_as(C.c_void_p),
                                           x.nbytes, None))
                dm = alloc(metric.nbytes)
                _ok(lib.ssq_memcpy_h2d(dm, metric.ctypes.data_as(C.c_void_p), metric.nbytes, None))
                di = alloc(8 * B * N)
                wsb = lib.ssq_ridges_workspace_bytes(code, B, F, N)
                dw = alloc(wsb)
                ev0, ev1 = C.c_void_p(), C.c_void_p()
                _ok(lib.ssq_event_create(C.byref(ev0)))
                _ok(lib.ssq_event_create(C.byref(ev1)))

                def run():
                    _ok(lib.ssq_ridges_exec(code, code, 0, dT, B, F, N, dm, None, 2.0, 1, 15.0, di, None, None, None,
                                            dw, wsb, None))
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
                k = 5
                bound_ms = (N - 1) * F * F * k / 128 / 2.4e9 * 1e3 * (2 if dt == np.float64 else 1)
                print(json.dumps({"dtype": np.dtype(dt).name, "F": F, "N": N, "B": B, "ms_median": float(np.median(times)),
                                  "ms_all": [round(t, 3) for t in times], "valu_bound_ms_per_signal_per_cu": round(bound_ms, 2),
                                  "workspace_gib": round(wsb / 2**30, 2)}), flush=True)
            finally:
                for p in ptrs:
                    lib.ssq_dev_free(p)


if __name__ == "__main__":
    main()
