#!/usr/bin/env python
"""Kernel time of the multisynchrosqueezed STFT (`ssq_mssq_stft_exec`: the operator kernel, the walk kernel, clearing Tx
and the scatter, HIP events around the launches, everything resident on the device) next to `ssq_ssq_stft2_exec` in the
same run on the same buffers.

    python tools/bench_msst.py [--batch 64] [--n 262144] [--n-fft 1024] [--hop 256] [--reps 9] [--out FILE]

Per dtype: `ssq_stft2` first, then orders 1 and 2 at n_iter 1, 4 and 16; median and min..max over `--reps` runs after two
warm-up runs, of the whole call and of its three parts (operator, walk, scatter).  Two differences are reported per order:
n_iter 4 against `ssq_stft2` (the price of the walk pass) and n_iter 16 against n_iter 4 (the price of the extra steps)."""
import argparse
import ctypes as C
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from ssqueeze_rs_amd import _lib  # noqa: E402

N_ITERS = (1, 4, 16)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _stats(ts):
    return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]


def run(x, win, n_fft, hop, reps):
    lib = _lib.load()
    B, N = x.shape
    code = _lib.SSQ_F32 if x.dtype == np.float32 else _lib.SSQ_F64
    F, nfr = n_fft // 2 + 1, (N - 1) // hop + 1
    map_bytes = B * F * nfr * 2 * x.dtype.itemsize
    ws = int(lib.ssq_mssq_stft_workspace_bytes(code, B, N, n_fft, hop))
    assert ws == int(lib.ssq_ssq_stft2_workspace_bytes(code, B, N, n_fft, hop))
    bufs = [C.c_void_p() for _ in range(4)]
    d_x, d_Tx, d_Sx, d_ws = bufs
    rec = {}
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
        rec["ssq_stft2_ms"] = _stats(ts)
        ms3 = (C.c_float * 3)()
        for order in (2, 1):
            for n_iter in N_ITERS:
                ts = [[], [], [], []]
                for i in range(2 + reps):
                    _lib.check(lib.ssq_mssq_stft_exec(code, d_x, B, N, _vp(win), n_fft, hop, 1.0, 0, 0, -1.0, 3, order, n_iter,
                                                      d_Tx, d_Sx, None, None, d_ws, ws, ms3))
                    if i >= 2:
                        for k in range(3):
                            ts[k].append(ms3[k])
                        ts[3].append(ms3[0] + ms3[1] + ms3[2])
                rec["order%d_iter%d_ms" % (order, n_iter)] = dict(total=_stats(ts[3]), operator=_stats(ts[0]), walk=_stats(ts[1]),
                                                                  scatter=_stats(ts[2]))
            t = {n: rec["order%d_iter%d_ms" % (order, n)]["total"][0] for n in N_ITERS}
            rec["order%d_walk_pass_ms" % order] = round(t[4] - rec["ssq_stft2_ms"][0], 4)
            rec["order%d_extra_steps_ms" % order] = round(t[16] - t[4], 4)
    finally:
        for d in bufs:
            if d:
                lib.ssq_dev_free(d)
    return rec


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
        rec = dict(dtype=np.dtype(dt).name, batch=a.batch, n=a.n, n_fft=a.n_fft, hop=a.hop, reps=a.reps)
        rec.update(run(x, win, a.n_fft, a.hop, a.reps))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_msst.py: [median, min, max] ms over the timed runs; total = operator + walk + scatter (Tx cleared\n"
                    "# with the scatter); walk_pass = n_iter 4 - ssq_stft2, extra_steps = n_iter 16 - n_iter 4 (medians of totals)\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
