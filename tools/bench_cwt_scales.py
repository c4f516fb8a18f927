"""Cost of the upstream ssq_cwt reassignment on a log-piecewise scale grid against the exponential grid of the same
length and range (and, at small N only, a linear grid: upstream's "poor scheme" has ~max_scale/min_scale rows).
    python tools/bench_cwt_scales.py [--log2n 20] [--dtype f32|f64] [--steps 5] [--linear]
One warm host call per step (ssq_ssq_cwt_host_rows, Tx only); prints one JSON line per grid with the median ms per call.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_cwt_scales.py ...` for the per-kernel device
times: cwt_reassign_kernel (exponential: one constant) against cwt_reassign_rows_kernel (per-row weights, two-segment
bins)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssqueeze_rs_amd import _lib, upstream as up  # noqa: E402
from ssqueeze_rs_amd._rs import _call, _cdtype, _ptr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2n", type=int, default=20)
ap.add_argument("--dtype", default="f32")
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--linear", action="store_true")
a = ap.parse_args()
lib = _lib.load()
_lib.require_gpu()
N = 1 << a.log2n
code = _lib.SSQ_F32 if a.dtype == "f32" else _lib.SSQ_F64
x = np.ascontiguousarray(np.random.default_rng(0).standard_normal((1, N)).astype(
    np.float32 if code == _lib.SSQ_F32 else np.float64))
wcode, p0, p1 = up._wavelet("gmw")
pw = up.process_scales("log-piecewise", N, "gmw").reshape(-1)
grids = {"log-piecewise": pw, "log": 2.0 ** np.linspace(np.log2(pw[0]), np.log2(pw[-1]), len(pw))}
if a.linear:
    grids["linear"] = up.process_scales("linear", N, "gmw").reshape(-1)
for name, s in grids.items():
    s = np.ascontiguousarray(s)
    _, kind, nv, _ = up._scales(s)
    const = up._row_const(s, kind, nv)
    f = np.ascontiguousarray(up._ssq_freqs(s, N, wcode, p0, p1, 1.0, "peak", kind))
    f_idx = up.logscale_transition_idx(f) if kind == "log-piecewise" else 0
    Tx = _lib.pinned_empty((1, len(s), N), _cdtype(code))

    def run():
        _call(lib.ssq_ssq_cwt_host_rows(code, _ptr(x), 1, N, wcode, p0, p1, _ptr(s), len(s), 1.0, _ptr(const), _ptr(f),
                                        up.FREQS[kind], f_idx, _lib.PAD["reflect"], 0, -1.0,
                                        up.VARIANT_UPSTREAM | up.VARIANT_FLIPUD, _ptr(Tx), None, None, None))
    run()
    ms = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        run()
        ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(grid=name, kind=kind, dtype=a.dtype, N=N, na=len(s), ms_median=float(np.median(ms)),
                          ms_min=float(np.min(ms)))), flush=True)
    del Tx
