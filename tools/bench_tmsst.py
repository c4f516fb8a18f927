#!/usr/bin/env python
"""Kernel time of the time-reassigned multisynchrosqueezed STFT (`ssq_tmssq_stft_exec`: the operator kernel, the walk
kernel and the time scatter, HIP events around the launches, everything resident on the device) next to
`ssq_tssq_stft_exec` in the same run on the same buffers.

    python tools/bench_tmsst.py [--batch 64] [--n 262144] [--n-fft 1024] [--hops 64,256] [--signal noise|impulses]
                                [--reps 9] [--out FILE]

Per dtype and hop: `tssq_stft` first (orders 2 and 1), then orders 2 and 1 at n_iter 1, 4 and 16; median and min..max over
`--reps` runs after two warm-up runs, of the whole call and of its three parts (operator, walk, scatter).  Two
differences are reported per order: n_iter 4 against `tssq_stft` (the price of the walk pass and of the wider scatter) and
n_iter 16 against n_iter 4.  `--signal noise` (the default) moves nearly every coefficient as far as the clamp allows,
the scatter's worst case; `--signal impulses` is an impulse every 4096 samples, whose map is a fixed point after one step,
so a workgroup of the scatter trims its walk to one window whatever n_iter."""
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
    ws = int(lib.ssq_tmssq_stft_workspace_bytes(code, B, N, n_fft, hop, max(N_ITERS)))
    assert ws >= int(lib.ssq_tssq_stft_workspace_bytes(code, B, N, n_fft, hop)) > 0
    bufs = [C.c_void_p() for _ in range(4)]
    d_x, d_Tx, d_Sx, d_ws = bufs
    rec = dict(reach=(n_fft // 2 - 1) // hop + 1)
    try:
        for d, n in zip(bufs, (x.nbytes, map_bytes, map_bytes, ws)):
            _lib.check(lib.ssq_dev_malloc(C.byref(d), n))
        _lib.check(lib.ssq_memcpy_h2d(d_x, _vp(x), x.nbytes, None))
        ms2, ms3 = (C.c_float * 2)(), (C.c_float * 3)()
        for order in (2, 1):
            ts = [[], [], []]
            for i in range(2 + reps):
                _lib.check(lib.ssq_tssq_stft_exec(code, d_x, B, N, _vp(win), n_fft, hop, 1.0, 0, order, -1.0, 3, d_Tx, d_Sx, None,
                                                  d_ws, ws, ms2))
                if i >= 2:
                    ts[0].append(ms2[0])
                    ts[1].append(ms2[1])
                    ts[2].append(ms2[0] + ms2[1])
            rec["order%d_tssq_stft_ms" % order] = dict(total=_stats(ts[2]), operator=_stats(ts[0]), scatter=_stats(ts[1]))
            for n_iter in N_ITERS:
                ts = [[], [], [], []]
                for i in range(2 + reps):
                    _lib.check(lib.ssq_tmssq_stft_exec(code, d_x, B, N, _vp(win), n_fft, hop, 1.0, 0, order, -1.0, 3, n_iter,
                                                       d_Tx, d_Sx, None, None, d_ws, ws, ms3))
                    if i >= 2:
                        for k in range(3):
                            ts[k].append(ms3[k])
                        ts[3].append(ms3[0] + ms3[1] + ms3[2])
                rec["order%d_iter%d_ms" % (order, n_iter)] = dict(total=_stats(ts[3]), operator=_stats(ts[0]), walk=_stats(ts[1]),
                                                                  scatter=_stats(ts[2]))
            t = {n: rec["order%d_iter%d_ms" % (order, n)]["total"][0] for n in N_ITERS}
            rec["order%d_iter4_over_tssq_ms" % order] = round(t[4] - rec["order%d_tssq_stft_ms" % order]["total"][0], 4)
            rec["order%d_iter16_over_iter4_ms" % order] = round(t[16] - t[4], 4)
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
    ap.add_argument("--hops", default="64,256")
    ap.add_argument("--signal", choices=("noise", "impulses"), default="noise")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    u = np.arange(a.n_fft) - a.n_fft // 2
    win = np.exp(-0.5 * (u / (a.n_fft / 10.0)) ** 2)
    lines = []
    for dt in (np.float32, np.float64):
        if a.signal == "noise":
            x = rng.standard_normal((a.batch, a.n)).astype(dt)
        else:
            x = np.zeros((a.batch, a.n), dtype=dt)
            x[:, 2048::4096] = 1.0
        for hop in (int(h) for h in a.hops.split(",")):
            rec = dict(dtype=np.dtype(dt).name, signal=a.signal, batch=a.batch, n=a.n, n_fft=a.n_fft, hop=hop, reps=a.reps)
            rec.update(run(x, win, a.n_fft, hop, a.reps))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("# tools/bench_tmsst.py --signal %s: [median, min, max] ms over the timed runs; total = operator + walk + scatter;\n"
                    "# reach = H, the scatter's reach is n_iter H; iter4_over_tssq, iter16_over_iter4: differences of the medians of totals\n"
                    % a.signal)
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
