#!/usr/bin/env python
"""Kernel times of the time-reassigned synchrosqueezed STFT (`ssq_tssq_stft_exec`: the operator kernel and the time
scatter, HIP events around the launches, everything resident on the device), orders 1 and 2, next to the second-order
frequency-reassigned transform (`ssq_ssq_stft2_exec`) at the same shapes.

    python tools/bench_tsst.py [--batch 64] [--n 262144] [--n-fft 1024] [--hops 1,64] [--reps 5] [--out FILE]

At hop 1 the maps of 64 signals of 2^18 samples do not fit the device (513 x 262144 bins a signal, 34 B a bin in
float64), so the batch runs in resident slices of `--slice-gib` and the slices' times are added: a signal's result and
cost do not depend on the slice it is in.  Per kernel: median and min..max over `--reps` passes after one warm-up
pass, and the achieved bytes/s against the ALGORITHMIC traffic (operator: the signal in, Sx and one int16 target a bin
out; scatter: the int16 target, Sx and Tx once a bin -- the halo re-read of the targets, at most 2 x 2 B, is not
counted)."""
import argparse
import ctypes as C
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from ssqueeze_rs_amd import _lib  # noqa: E402


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _stats(ts):
    return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]


def run(x, win, n_fft, hop, reps, slice_bytes):
    """-> dict of [median, min, max] ms: tssq order 1 / 2 operator and scatter, ssq_stft2 kernels."""
    lib = _lib.load()
    B, N = x.shape
    code = _lib.SSQ_F32 if x.dtype == np.float32 else _lib.SSQ_F64
    F, nfr = n_fft // 2 + 1, (N - 1) // hop + 1
    csize = 2 * x.dtype.itemsize
    per = 3 * F * nfr * csize + 8 * N                      # Tx, Sx and ssq_stft2's map: the larger workspace of the two
    S = int(max(1, min(B, slice_bytes // per)))
    map_bytes = S * F * nfr * csize
    ws = max(int(lib.ssq_tssq_stft_workspace_bytes(code, S, N, n_fft, hop)),
             int(lib.ssq_ssq_stft2_workspace_bytes(code, S, N, n_fft, hop)))
    bufs = [C.c_void_p() for _ in range(4)]
    d_x, d_Tx, d_Sx, d_ws = bufs
    acc = {k: [0.0] * (1 + reps) for k in ("o1_operator", "o1_scatter", "o2_operator", "o2_scatter", "ssq_stft2")}
    try:
        for d, n in zip(bufs, (S * N * x.dtype.itemsize, map_bytes, map_bytes, ws)):
            _lib.check(lib.ssq_dev_malloc(C.byref(d), n))
        ms2, ms1 = (C.c_float * 2)(), C.c_float(0)
        for b0 in range(0, B, S):
            xs = np.ascontiguousarray(x[b0:b0 + S])
            nb = xs.shape[0]
            _lib.check(lib.ssq_memcpy_h2d(d_x, _vp(xs), xs.nbytes, None))
            for i in range(1 + reps):
                for order in (1, 2):
                    _lib.check(lib.ssq_tssq_stft_exec(code, d_x, nb, N, _vp(win), n_fft, hop, 1.0, 0, order, -1.0, 3, d_Tx,
                                                      d_Sx, None, d_ws, ws, ms2))
                    acc["o%d_operator" % order][i] += ms2[0]
                    acc["o%d_scatter" % order][i] += ms2[1]
                _lib.check(lib.ssq_ssq_stft2_exec(code, d_x, nb, N, _vp(win), n_fft, hop, 1.0, 0, 0, -1.0, 3, d_Tx, d_Sx,
                                                  None, d_ws, ws, C.byref(ms1)))
                acc["ssq_stft2"][i] += ms1.value
    finally:
        for d in bufs:
            if d:
                lib.ssq_dev_free(d)
    out = {k: _stats(v[1:]) for k, v in acc.items()}
    cells = B * F * nfr
    op_bytes = B * N * (8 if code == _lib.SSQ_F64 else 4 + 8 + 8) + cells * (csize + 2)
    sc_bytes = cells * (2 + 2 * csize)
    out["slice_signals"] = S
    out["operator_GBps"] = {o: round(op_bytes / out["o%d_operator" % o][0] / 1e6, 1) for o in (1, 2)}
    out["scatter_GBps"] = {o: round(sc_bytes / out["o%d_scatter" % o][0] / 1e6, 1) for o in (1, 2)}
    out["ratio_o2_to_ssq_stft2"] = round((out["o2_operator"][0] + out["o2_scatter"][0]) / out["ssq_stft2"][0], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--n-fft", type=int, default=1024)
    ap.add_argument("--hops", default="1,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slice-gib", type=float, default=24.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    u = np.arange(a.n_fft) - a.n_fft // 2
    win = np.exp(-0.5 * (u / (a.n_fft / 10.0)) ** 2)
    lines = []
    for dt in (np.float32, np.float64):
        x = rng.standard_normal((a.batch, a.n)).astype(dt)
        for hop in (int(h) for h in a.hops.split(",")):
            rec = dict(dtype=np.dtype(dt).name, batch=a.batch, n=a.n, n_fft=a.n_fft, hop=hop, reps=a.reps)
            rec.update(run(x, win, a.n_fft, hop, a.reps, int(a.slice_gib * 2 ** 30)))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            if a.out:                                        # (rewritten after every shape: a long run leaves what it has)
                with open(a.out, "w") as f:
                    f.write("# tools/bench_tsst.py: [median, min, max] ms over the timed passes, the batch's resident slices "
                            "added; GB/s = algorithmic traffic / median time, per order\n")
                    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
