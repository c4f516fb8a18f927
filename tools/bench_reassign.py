#!/usr/bin/env python
"""Kernel times of the reassigned spectrogram (`ssq_reassign_stft_exec`: the operator kernel and the two-way scatter, HIP
events around the launches, everything resident on the device), next to the first-order time-reassigned transform
(`ssq_tssq_stft_exec`, order 1) at the same shapes.

    python tools/bench_reassign.py [--batch 64] [--n 262144] [--n-fft 1024] [--hops 1,64] [--reps 5] [--out FILE]

Every (dtype, hop) runs in a child process of its own under a time limit (`--step-timeout` seconds); the first one that
fails or runs out of time ends the run.  At hop 1 the maps of 64 signals of 2^18 samples do not fit the device, so the
batch runs in resident slices of `--slice-gib` and the slices' times are added: a signal's result and cost do not depend
on the slice it is in.  Per kernel: median and min..max over `--reps` passes after one warm-up pass, and the achieved
bytes/s against the ALGORITHMIC traffic (operator: the signal in, Sx and one 4-byte target a bin out; scatter: the
target and Sx in and Rx out once a bin -- the halo re-read of the targets, (T + 2 H) / T of them, is not counted but
reported as `target_reread`)."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ssqueeze_rs_amd import _lib  # noqa: E402

CELLS, MAX_TILE = 16384, 1024          # csrc/stft_reassign.hip: kReassignCells, kReassignMaxTile


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _stats(ts):
    return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]


def run(x, win, n_fft, hop, reps, slice_bytes):
    """-> dict of [median, min, max] ms: reassign operator and scatter, tssq order 1 operator and scatter."""
    lib = _lib.load()
    B, N = x.shape
    code = _lib.SSQ_F32 if x.dtype == np.float32 else _lib.SSQ_F64
    F, nfr = n_fft // 2 + 1, (N - 1) // hop + 1
    rsize = x.dtype.itemsize
    csize = 2 * rsize
    per = F * nfr * (2 * csize + 4) + 8 * N + 16           # Tx / Rx, Sx and the targets: the larger of the two transforms
    S = int(max(1, min(B, slice_bytes // per)))
    map_bytes = S * F * nfr * csize
    ws = max(int(lib.ssq_reassign_stft_workspace_bytes(code, S, N, n_fft, hop)),
             int(lib.ssq_tssq_stft_workspace_bytes(code, S, N, n_fft, hop)))
    bufs = [C.c_void_p() for _ in range(4)]
    d_x, d_Tx, d_Sx, d_ws = bufs
    acc = {k: [0.0] * (1 + reps) for k in ("operator", "scatter", "tssq1_operator", "tssq1_scatter")}
    try:
        for d, n in zip(bufs, (S * N * rsize, map_bytes, map_bytes, ws)):
            _lib.check(lib.ssq_dev_malloc(C.byref(d), n))
        ms = (C.c_float * 2)()
        for b0 in range(0, B, S):
            xs = np.ascontiguousarray(x[b0:b0 + S])
            nb = xs.shape[0]
            _lib.check(lib.ssq_memcpy_h2d(d_x, _vp(xs), xs.nbytes, None))
            for i in range(1 + reps):
                _lib.check(lib.ssq_reassign_stft_exec(code, d_x, nb, N, _vp(win), n_fft, hop, 1.0, 0, -1.0, 3, d_Tx, d_Sx,
                                                      None, None, d_ws, ws, ms))
                acc["operator"][i] += ms[0]
                acc["scatter"][i] += ms[1]
                _lib.check(lib.ssq_tssq_stft_exec(code, d_x, nb, N, _vp(win), n_fft, hop, 1.0, 0, 1, -1.0, 3, d_Tx, d_Sx,
                                                  None, d_ws, ws, ms))
                acc["tssq1_operator"][i] += ms[0]
                acc["tssq1_scatter"][i] += ms[1]
    finally:
        for d in bufs:
            if d:
                lib.ssq_dev_free(d)
    out = {k: _stats(v[1:]) for k, v in acc.items()}
    cells = B * F * nfr
    H, T = -(-n_fft // (2 * hop)), min(MAX_TILE, CELLS // F, nfr)
    op_bytes = B * N * (8 if code == _lib.SSQ_F64 else 4 + 8 + 8) + cells * (csize + 4)
    sc_bytes = cells * (4 + csize + rsize)
    out["slice_signals"] = S
    out["tile_frames"], out["reach"] = T, H
    out["target_reread"] = round((T + 2 * H) / T, 2)
    out["operator_GBps"] = round(op_bytes / out["operator"][0] / 1e6, 1)
    out["scatter_GBps"] = round(sc_bytes / out["scatter"][0] / 1e6, 1)
    out["ratio_to_tssq1"] = round((out["operator"][0] + out["scatter"][0]) /
                                  (out["tssq1_operator"][0] + out["tssq1_scatter"][0]), 2)
    return out


def child(a):
    _lib.require_gpu()
    dt = np.dtype(a.dtype).type
    u = np.arange(a.n_fft) - a.n_fft // 2
    win = np.exp(-0.5 * (u / (a.n_fft / 10.0)) ** 2)
    x = np.random.default_rng(0).standard_normal((a.batch, a.n)).astype(dt)
    rec = dict(dtype=np.dtype(dt).name, batch=a.batch, n=a.n, n_fft=a.n_fft, hop=a.hop, reps=a.reps)
    rec.update(run(x, win, a.n_fft, a.hop, a.reps, int(a.slice_gib * 2 ** 30)))
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--n-fft", type=int, default=1024)
    ap.add_argument("--hops", default="1,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slice-gib", type=float, default=24.0)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dtype", default=None, help=argparse.SUPPRESS)       # the child's configuration
    ap.add_argument("--hop", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.dtype is not None:
        return child(a)
    lines = []
    for dt in ("float32", "float64"):
        for hop in (int(h) for h in a.hops.split(",")):
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--batch", str(a.batch),
                   "--n", str(a.n), "--n-fft", str(a.n_fft), "--reps", str(a.reps), "--slice-gib", str(a.slice_gib),
                   "--dtype", dt, "--hop", str(hop)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            res = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not res:                 # nothing more is started on the GPU after a failure
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit("bench_reassign: %s hop %d ended with status %d" % (dt, hop, r.returncode))
            lines.append(res[0])
            print(lines[-1], flush=True)
            if a.out:                                        # (rewritten after every shape: a long run leaves what it has)
                with open(a.out, "w") as f:
                    f.write("# tools/bench_reassign.py: [median, min, max] ms over the timed passes, the batch's resident "
                            "slices added; GB/s = algorithmic traffic / median time; tssq1_*: tssq_stft order 1\n")
                    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
