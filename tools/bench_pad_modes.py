"""Time the upstream-variant ssq_stft and ssq_cwt plans once per pad type (include/ssq_hip.h: SSQ_PAD_*), so the cost
of the index arithmetic in the padded loads (csrc/pad_index.h) can be read next to 'reflect'.
    python tools/bench_pad_modes.py [--steps 10] [--batch 64]
ssq_stft: batch x 2^20, n_fft 1024, hop 256, fp32 (the unfused kernels: what upstream plans run).
ssq_cwt: BASELINE config 4's shape (1 x 2^20, Morlet, 256 log scales, fp32), as `upstream.ssq_cwt` on host arrays (one
call per timing) and its forward transform alone on device buffers.
Prints one JSON line per (transform, pad type): median and min / max of `--repeat` timings of `--steps` calls each."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssqueeze_rs_amd import _lib  # noqa: E402
from ssqueeze_rs_amd.synth import synth_signal  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--log2n", type=int, default=20)
a = ap.parse_args()
lib = _lib.load()
PADS = ("reflect", "zero", "symmetric", "replicate", "wrap")        # codes 0 .. 4
UPSTREAM, MODULATED = 1, 2
N, B, es = 1 << a.log2n, a.batch, 4
vp = C.c_void_p


def dev(nbytes):
    p = vp()
    _lib.check(lib.ssq_dev_malloc(C.byref(p), max(int(nbytes), 16)))
    return p


def timed(run):
    run()
    _lib.check(lib.ssq_device_sync())
    ms = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            run()
        _lib.check(lib.ssq_device_sync())
        ms.append((time.perf_counter() - t0) / a.steps * 1e3)
    return {"ms_median": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms)}


# ---- ssq_stft ----
n_fft, hop = 1024, 256
nf, nfr = n_fft // 2 + 1, (N - 1) // hop + 1
x = np.stack([synth_signal(N, b % 8, np.float32) for b in range(min(B, 8))])
dx = dev(B * N * es)
for b in range(B):
    _lib.check(lib.ssq_memcpy_h2d(vp(dx.value + b * N * es), x[b % x.shape[0]].ctypes.data_as(vp), N * es, None))
dT = dev(B * nf * nfr * 2 * es)
win = np.hanning(n_fft)
for code, name in enumerate(PADS):
    plan = vp()
    _lib.check(lib.ssq_stft_plan_create_v(C.byref(plan), _lib.SSQ_F32, N, win.ctypes.data_as(vp), n_fft, hop, 1.0, code,
                                          0, -1.0, 0, UPSTREAM | MODULATED))
    wsb = lib.ssq_stft_plan_workspace_bytes(plan, B, _lib.OUT_TX)
    ws = dev(wsb)
    r = timed(lambda: _lib.check(lib.ssq_stft_plan_exec(plan, _lib.OUT_TX, dx, B, dT, ws, wsb, None)))
    print(json.dumps({"workload": f"upstream ssq_stft f32 batch={B} x 2^{a.log2n} n_fft={n_fft} hop={hop}",
                      "padtype": name, **r}), flush=True)
    _lib.check(lib.ssq_dev_free(ws))
    _lib.check(lib.ssq_stft_plan_destroy(plan))
_lib.check(lib.ssq_dev_free(dT))

# ---- ssq_cwt, C4 shape ----
# An upstream plan's ssq exec needs the frequencies and row weights that only the host entry point hands it, so ssq_cwt
# is timed as users call it, `upstream.ssq_cwt` on host arrays (the read-back of Tx and Wx, 2 x 2 GB, is in the figure),
# and the forward transform that holds every padded load (Wx and dWx, ssq_cwt_plan_exec_cwt) on device buffers.
from ssqueeze_rs_amd import upstream as up  # noqa: E402

na = 256
scales = 2.0 ** np.linspace(1, a.log2n - 1, na)
dW, dD = dev(na * N * 2 * es), dev(na * N * 2 * es)
for code, name in enumerate(PADS):
    plan = vp()
    _lib.check(lib.ssq_cwt_plan_create_v(C.byref(plan), _lib.SSQ_F32, N, _lib.WAVELET["morlet"], 13.4, 0.0,
                                         scales.ctypes.data_as(vp), na, 1.0, code, UPSTREAM))
    wsb = lib.ssq_cwt_plan_workspace_bytes(plan, 1)
    ws = dev(wsb)
    r = timed(lambda: _lib.check(lib.ssq_cwt_plan_exec_cwt(plan, dx, 1, 1, 0, dW, dD, ws, wsb, None)))
    print(json.dumps({"workload": f"upstream cwt (Wx, dWx) morlet na={na} 1 x 2^{a.log2n} f32, device buffers",
                      "padtype": name, **r}), flush=True)
    _lib.check(lib.ssq_dev_free(ws))
    _lib.check(lib.ssq_cwt_plan_destroy(plan))
_lib.check(lib.ssq_dev_free(dW))
_lib.check(lib.ssq_dev_free(dD))
_lib.check(lib.ssq_dev_free(dx))
a.steps = 1
for name in PADS:
    r = timed(lambda: up.ssq_cwt(x[0], "morlet", scales=scales, padtype=name))
    print(json.dumps({"workload": f"upstream.ssq_cwt morlet na={na} 1 x 2^{a.log2n} f32, host arrays",
                      "padtype": name, **r}), flush=True)
