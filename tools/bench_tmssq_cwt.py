#!/usr/bin/env python
"""Kernel time of the time-reassigned multisynchrosqueezed CWT (`ssq_tmssq_cwt_exec`: the operator part, the walk kernel,
the scatter kernel and all kernels, HIP events around the launches, everything resident on the device) next to
`ssq_tssq_cwt_exec` in the same run on the same buffers.

    python tools/bench_tmssq_cwt.py [--batch 4] [--n 65536] [--na 128] [--signals noise,chirp,impulse]
                                    [--reps 9] [--out FILE]

Per signal, dtype and order: `tssq_cwt` first, then n_iter 1, 4 and 16; median and min..max over `--reps` runs after two
warm-up runs.  GMW(3, 60), log scales from the Nyquist peak down to N / 4 samples per cycle (tools/bench_tssq_cwt.py's
grid).  Signals: white noise, the chirp 0.02 -> 0.45 cycles/sample, and one impulse a signal.  From the one-step map
of the float64 call's first signal the tool also counts, in numpy, the chain steps of the walk that fell outside the stage
of the tile they started in (`tmssq_cwt_tile_cols`): the reads the kernel takes from device memory instead of LDS, as a
share of all walked steps at n_iter 4 and 16."""
import argparse
import ctypes as C
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from ssqueeze_rs_amd import _lib  # noqa: E402
from ssqueeze_rs_amd import upstream as up  # noqa: E402

N_ITERS = (1, 4, 16)
GMW = ("gmw", {"gamma": 3.0, "beta": 60.0})


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _stats(ts):
    return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]


def far_share(t1, n_iters):
    """{n_iter: walked steps read outside the stage / all walked steps} of the one-step map t1 [na, N]."""
    T, halo = up.tmssq_cwt_tile_cols()
    N = t1.shape[-1]
    j = np.arange(N, dtype=np.int64)[None, :]
    lo, hi = j // T * T - halo, np.minimum(j // T * T + T, N) + halo
    t1 = t1.astype(np.int64)
    c, live = t1.copy(), t1 >= 0
    far = steps = 0
    out = {}
    for k in range(2, max(n_iters) + 1):
        far += int((live & ((c < lo) | (c >= hi))).sum())
        steps += int(live.sum())
        nxt = np.take_along_axis(t1, np.maximum(c, 0), axis=-1)
        live &= (nxt >= 0) & (nxt != c)
        c = np.where(live, nxt, c)
        if k in n_iters:
            out[k] = round(far / max(steps, 1), 4)
    return out


def run(x, scales, nu, reps):
    lib = _lib.load()
    B, N = x.shape
    na = len(scales)
    code = _lib.SSQ_F32 if x.dtype == np.float32 else _lib.SSQ_F64
    map_bytes = B * na * N * 2 * x.dtype.itemsize
    ws = int(lib.ssq_tmssq_cwt_workspace_bytes(code, B, N, na, 2, None))
    ws1 = int(lib.ssq_tssq_cwt_workspace_bytes(code, B, N, na, 2, None))        # the same rows per chunk for both
    assert ws >= ws1 > 0
    bufs = [C.c_void_p() for _ in range(5)]
    d_x, d_Tx, d_Wx, d_mm, d_ws = bufs
    rec = {}
    try:
        for d, n in zip(bufs, (x.nbytes, map_bytes, map_bytes, 4 * B * na * N, ws)):
            _lib.check(lib.ssq_dev_malloc(C.byref(d), n))
        _lib.check(lib.ssq_memcpy_h2d(d_x, _vp(x), x.nbytes, None))
        ms3, ms4 = (C.c_float * 3)(), (C.c_float * 4)()
        front = (code, d_x, B, N, 0, 3.0, 60.0, _vp(scales), _vp(nu), na, 1.0, 0)
        for order in (2, 1):
            ts = [[], [], []]
            for i in range(2 + reps):
                _lib.check(lib.ssq_tssq_cwt_exec(*front, order, -1.0, d_Tx, d_Wx, None, d_mm, d_ws, ws1, None, ms3))
                if i >= 2:
                    for k in range(3):
                        ts[k].append(ms3[k])
            rec["order%d_tssq_cwt_ms" % order] = dict(total=_stats(ts[0]), operator=_stats(ts[2]), scatter=_stats(ts[1]))
            if x.dtype == np.float64:                          # the one-step map of the first signal, still in d_mm
                t1 = np.empty((na, N), dtype=np.int32)
                _lib.check(lib.ssq_memcpy_d2h(_vp(t1), d_mm, t1.nbytes, None))
                rec["order%d_far_share" % order] = far_share(t1, (4, 16))
            for n_iter in N_ITERS:
                ts = [[], [], [], []]
                for i in range(2 + reps):
                    _lib.check(lib.ssq_tmssq_cwt_exec(*front, order, -1.0, n_iter, d_Tx, d_Wx, None, None, d_ws, ws, None, ms4))
                    if i >= 2:
                        for k in range(4):
                            ts[k].append(ms4[k])
                rec["order%d_iter%d_ms" % (order, n_iter)] = dict(total=_stats(ts[0]), operator=_stats(ts[1]),
                                                                  walk=_stats(ts[2]), scatter=_stats(ts[3]))
    finally:
        for d in bufs:
            if d:
                lib.ssq_dev_free(d)
    return rec


def make_signal(kind, batch, n, rng):
    if kind == "noise":
        return rng.standard_normal((batch, n))
    if kind == "chirp":
        t = np.arange(n, dtype=np.float64)
        ph = 2 * np.pi * (0.02 * t + 0.5 * (0.45 - 0.02) / n * t * t)
        return np.tile(np.cos(ph), (batch, 1))
    x = np.zeros((batch, n))
    x[np.arange(batch), n // 2 + 1000 * np.arange(batch)] = 1.0
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--n", type=int, default=1 << 16)
    ap.add_argument("--na", type=int, default=128)
    ap.add_argument("--signals", default="noise,chirp,impulse")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    wc = (60.0 / 3.0) ** (1 / 3.0)
    scales = np.ascontiguousarray(wc / np.pi * 2.0 ** np.linspace(0, np.log2(a.n / 8), a.na))
    nu = up.tssq_cwt_row_freqs(GMW, scales)
    T, halo = up.tmssq_cwt_tile_cols()
    lines = []
    for kind in a.signals.split(","):
        x64 = make_signal(kind, a.batch, a.n, rng)
        for dt in (np.float32, np.float64):
            rec = dict(dtype=np.dtype(dt).name, signal=kind, batch=a.batch, n=a.n, na=a.na, reps=a.reps, tile=T,
                       halo=halo)
            rec.update(run(np.ascontiguousarray(x64.astype(dt)), scales, nu, a.reps))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("# tools/bench_tmssq_cwt.py: [median, min, max] ms over the timed runs; total: all kernels (with the read-out);\n"
                    "# operator: everything before the walk; far_share: walked steps read from device memory / all walked steps\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
