"""Time the upstream-variant cwt with higher-order GMWs on warm device plans: order 0 against an averaged order set (one
transform with the averaged wavelet table) and against `average=False` (one plan with a row group per order).
    python tools/bench_cwt_order.py [--log2n 20] [--na 256] [--dtype f32|f64] [--orders 0,1,2] [--steps 5]
Prints one JSON line per case: ms per call (Wx only, L1 norm, unpadded) and the ratio to order 0."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssqueeze_rs_amd import _lib, upstream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2n", type=int, default=20)
ap.add_argument("--na", type=int, default=256)
ap.add_argument("--dtype", default="f32")
ap.add_argument("--orders", default="0,1,2")
ap.add_argument("--steps", type=int, default=5)
a = ap.parse_args()
lib = _lib.load()
_lib.require_gpu()
N, na = 1 << a.log2n, a.na
code = _lib.SSQ_F32 if a.dtype == "f32" else _lib.SSQ_F64
es = 4 if code == _lib.SSQ_F32 else 8
gamma, beta = 3.0, 60.0
orders = [int(k) for k in a.orders.split(",")]
scales = np.ascontiguousarray(2.0 ** np.linspace(1, a.log2n - 1, na))
vp = lambda arr: arr.ctypes.data_as(C.c_void_p)                                   # noqa: E731
x = np.random.default_rng(0).standard_normal(N).astype(np.float32 if code == _lib.SSQ_F32 else np.float64)


def make_plan(polys):
    plan = C.c_void_p()
    if polys is None:
        _lib.check(lib.ssq_cwt_plan_create_v(C.byref(plan), code, N, _lib.WAVELET["gmw"], gamma, beta, vp(scales), na, 1.0,
                                             0, upstream.VARIANT_UPSTREAM))
        return plan, 1
    polys = np.ascontiguousarray(polys)
    _lib.check(lib.ssq_cwt_plan_create_gmwk(C.byref(plan), code, N, gamma, beta, vp(polys), polys.shape[1],
                                            polys.shape[0], vp(scales), na, 1.0, 0, upstream.VARIANT_UPSTREAM))
    return plan, polys.shape[0]


def time_plan(polys):
    plan, groups = make_plan(polys)
    wsb = lib.ssq_cwt_plan_workspace_bytes(plan, 1)
    dx, dW, ws, st = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    e0, e1 = C.c_void_p(), C.c_void_p()
    _lib.check(lib.ssq_dev_malloc(C.byref(dx), N * es))
    _lib.check(lib.ssq_dev_malloc(C.byref(dW), groups * na * N * 2 * es))
    _lib.check(lib.ssq_dev_malloc(C.byref(ws), wsb))
    _lib.check(lib.ssq_stream_create(C.byref(st)))
    _lib.check(lib.ssq_event_create(C.byref(e0)))
    _lib.check(lib.ssq_event_create(C.byref(e1)))
    _lib.check(lib.ssq_memcpy_h2d(dx, vp(x), N * es, st))
    run = lambda: _lib.check(lib.ssq_cwt_plan_exec_cwt(plan, dx, 1, 1, 0, dW, None, ws, wsb, st))   # noqa: E731
    run()                                                                                           # warm
    _lib.check(lib.ssq_stream_sync(st))
    ms = []
    for _ in range(a.steps):
        _lib.check(lib.ssq_event_record(e0, st))
        run()
        _lib.check(lib.ssq_event_record(e1, st))
        _lib.check(lib.ssq_event_sync(e1))
        t = C.c_float(0)
        _lib.check(lib.ssq_event_elapsed_ms(e0, e1, C.byref(t)))
        ms.append(t.value)
    for h in (dx, dW, ws):
        lib.ssq_dev_free(h)
    lib.ssq_event_destroy(e0)
    lib.ssq_event_destroy(e1)
    lib.ssq_stream_destroy(st)
    lib.ssq_cwt_plan_destroy(plan)
    return float(np.median(ms)), float(np.min(ms))


base = time_plan(None)
cases = [("order=0", base),
         (f"order={tuple(orders)} averaged", time_plan(upstream.gmw_order_coefficients(gamma, beta, orders))),
         (f"order={tuple(orders)} average=False",
          time_plan(upstream.gmw_order_coefficients(gamma, beta, orders, average=False)))]
for name, (med, mn) in cases:
    print(json.dumps(dict(case=name, dtype=a.dtype, N=f"2^{a.log2n}", na=na, ms_median=round(med, 3), ms_min=round(mn, 3),
                          ratio_to_order0=round(med / base[0], 3), steps=a.steps)), flush=True)
