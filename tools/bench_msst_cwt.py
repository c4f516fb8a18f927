#!/usr/bin/env python
"""Kernel time of the multisynchrosqueezed CWT (`ssq_mssq_cwt_exec`: the fp64 map pipeline with the operator, the walk
kernel, clearing Tx and the scatter; HIP events around the launches, everything resident on the device) next to
`ssq_ssq_cwt2_exec` in the same process on the same buffers.

    python tools/bench_msst_cwt.py [--batch 4] [--n 65536] [--na 128] [--reps 9] [--out FILE]

GMW(3, 60), log scales from the Nyquist peak down to N/4 samples per cycle on 'maximal' log frequencies
(tools/bench_cwt_sst2.py's grids).  Per dtype and signal (linear chirps, white noise): `ssq_cwt2` first, then orders 1 and 2
at n_iter 1, 4 and 16; median and min..max over `--reps` runs after two warm-up runs, of the whole call and of its three
parts (pipeline + operator, walk, scatter).  Per order two differences of the totals' medians: n_iter 4 against `ssq_cwt2`
(the price of the walk pass) and n_iter 16 against n_iter 4 (the price of the extra steps); and the walk's median at
n_iter 4 as a share of `ssq_cwt2` and of the scatter in the same run."""
import argparse
import ctypes as C
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from ssqueeze_rs_amd import _lib  # noqa: E402
from ssqueeze_rs_amd import upstream as up  # noqa: E402

GAMMA, BETA = 3.0, 60.0
N_ITERS = (1, 4, 16)
HEAD = ("# tools/bench_msst_cwt.py: [median, min, max] ms over the timed runs; total = operator (the map pipeline with the\n"
        "# operator kernel) + walk + scatter (Tx cleared with the scatter); walk_pass = n_iter 4 - ssq_cwt2, extra_steps =\n"
        "# n_iter 16 - n_iter 4 (medians of totals); walk_share_of_*: the walk's median at n_iter 4 over ssq_cwt2's and over\n"
        "# the scatter's in the same run\n")


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


def signals(kind, batch, n, dt):
    if kind == "noise":
        return np.random.default_rng(0).standard_normal((batch, n)).astype(dt)
    t = np.arange(n, dtype=np.float64)
    rows = []
    for b in range(batch):                                           # linear chirps, a different sweep per signal
        f0, f1 = 0.01 * (b + 1), 0.45 - 0.05 * b
        rows.append(np.cos(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) / n * t * t)))
    return np.stack(rows).astype(dt)


def run(x, na, reps):
    lib = _lib.load()
    B, N = x.shape
    code = _lib.SSQ_F32 if x.dtype == np.float32 else _lib.SSQ_F64
    scales, rc, f = _grids(N, na)
    rho = up.mssq_cwt_row_of_bin(("gmw", {"gamma": GAMMA, "beta": BETA}), scales, f)
    map_bytes = B * na * N * 2 * x.dtype.itemsize
    ws = int(lib.ssq_mssq_cwt_workspace_bytes(code, B, N, na, None))
    assert ws >= int(lib.ssq_ssq_cwt2_workspace_bytes(code, B, N, na, None))
    bufs = [C.c_void_p() for _ in range(5)]
    d_x, d_Tx, d_Wx, d_w, d_ws = bufs
    rec = {"workspace_MB": round(ws / 2 ** 20, 1)}
    try:
        for d, n in zip(bufs, (x.nbytes, map_bytes, map_bytes, map_bytes // 2, ws)):
            _lib.check(lib.ssq_dev_malloc(C.byref(d), n))
        _lib.check(lib.ssq_memcpy_h2d(d_x, _vp(x), x.nbytes, None))
        ms, ts = C.c_float(0), []
        for i in range(2 + reps):
            _lib.check(lib.ssq_ssq_cwt2_exec(code, d_x, B, N, 0, GAMMA, BETA, _vp(scales), na, 1.0, _vp(rc), _vp(f), 0, 0, 0, 0,
                                             -1.0, 4, d_Tx, d_Wx, d_w, d_ws, ws, None, C.byref(ms)))
            if i >= 2:
                ts.append(ms.value)
        rec["ssq_cwt2_ms"] = _stats(ts)
        ms3 = (C.c_float * 3)()
        for order in (2, 1):
            for n_iter in N_ITERS:
                ts = [[], [], [], []]
                for i in range(2 + reps):
                    _lib.check(lib.ssq_mssq_cwt_exec(code, d_x, B, N, 0, GAMMA, BETA, _vp(scales), na, 1.0, _vp(rc), _vp(f), 0, 0,
                                                     0, 0, -1.0, 4, order, n_iter, _vp(rho), d_Tx, d_Wx, d_w, None, None, d_ws, ws,
                                                     None, ms3))
                    if i >= 2:
                        for k in range(3):
                            ts[k].append(ms3[k])
                        ts[3].append(ms3[0] + ms3[1] + ms3[2])
                rec["order%d_iter%d_ms" % (order, n_iter)] = dict(total=_stats(ts[3]), operator=_stats(ts[0]), walk=_stats(ts[1]),
                                                                  scatter=_stats(ts[2]))
            t = {n: rec["order%d_iter%d_ms" % (order, n)] for n in N_ITERS}
            rec["order%d_walk_pass_ms" % order] = round(t[4]["total"][0] - rec["ssq_cwt2_ms"][0], 4)
            rec["order%d_extra_steps_ms" % order] = round(t[16]["total"][0] - t[4]["total"][0], 4)
            rec["order%d_walk_share_of_ssq_cwt2" % order] = round(t[4]["walk"][0] / rec["ssq_cwt2_ms"][0], 4)
            rec["order%d_walk_share_of_scatter" % order] = round(t[4]["walk"][0] / t[4]["scatter"][0], 4)
    finally:
        for d in bufs:
            if d:
                lib.ssq_dev_free(d)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--n", type=int, default=1 << 16)
    ap.add_argument("--na", type=int, default=128)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    lines = []
    for dt in (np.float32, np.float64):
        for kind in ("chirp", "noise"):
            rec = dict(dtype=np.dtype(dt).name, signal=kind, batch=a.batch, n=a.n, na=a.na, reps=a.reps)
            rec.update(run(signals(kind, a.batch, a.n, dt), a.na, a.reps))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(HEAD + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
