#!/usr/bin/env python
"""Kernel times of the synchroextracting / transient-extracting STFT (`ssq_extract_stft_exec`: ONE kernel, HIP events
around the launch, everything resident on the device), both axes, orders 1 and 2, with Sx stored and not stored, next to
the transforms whose maps it reads, at the same shapes and from the same build: `ssq_ssq_stft2_exec` (operator + scatter,
one figure) and `ssq_tssq_stft_exec` (operator and time scatter apart), orders 1 and 2.

    python tools/bench_extract.py [--batch 64] [--n 262144] [--n-fft 1024] [--hops 256,64] [--reps 9] [--out FILE]

All variants run interleaved in the same process, pass after pass: one warm-up pass, then per variant the median and the
min..max over `--reps` timed passes.  A float32 call's time includes the widening of its signals, in every transform.  GB/s
is the ALGORITHMIC traffic of an extract call (the signal in, Te and, where stored, Sx out) over the median time."""
import argparse
import ctypes as C
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from ssqueeze_rs_amd import _lib  # noqa: E402

AXES = {"set": 0, "tet": 1}


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _stats(ts):
    return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]


def run(x, win, n_fft, hop, reps):
    """-> dict of [median, min, max] ms per variant."""
    lib = _lib.load()
    B, N = x.shape
    code = _lib.SSQ_F32 if x.dtype == np.float32 else _lib.SSQ_F64
    F, nfr = n_fft // 2 + 1, (N - 1) // hop + 1
    csize = 2 * x.dtype.itemsize
    map_bytes = B * F * nfr * csize
    ws = max(int(lib.ssq_extract_stft_workspace_bytes(code, B, N, n_fft, hop)),
             int(lib.ssq_tssq_stft_workspace_bytes(code, B, N, n_fft, hop)),
             int(lib.ssq_ssq_stft2_workspace_bytes(code, B, N, n_fft, hop)))
    bufs = [C.c_void_p() for _ in range(4)]
    d_x, d_Tx, d_Sx, d_ws = bufs
    variants = [("%s_o%d_%s" % (a, o, "Sx" if sx else "noSx"), a, o, sx) for a in AXES for o in (2, 1) for sx in (False, True)]
    acc = {v[0]: [] for v in variants}
    for k in ("ssq_stft2", "tssq_o1_operator", "tssq_o1_scatter", "tssq_o2_operator", "tssq_o2_scatter"):
        acc[k] = []
    try:
        for d, n in zip(bufs, (x.nbytes, map_bytes, map_bytes, ws)):
            _lib.check(lib.ssq_dev_malloc(C.byref(d), n))
        _lib.check(lib.ssq_memcpy_h2d(d_x, _vp(x), x.nbytes, None))
        ms2, ms1 = (C.c_float * 2)(), C.c_float(0)
        for i in range(1 + reps):
            for name, a, o, sx in variants:
                _lib.check(lib.ssq_extract_stft_exec(code, d_x, B, N, _vp(win), n_fft, hop, 1.0, 0, AXES[a], o, -1.0, 3, d_Tx,
                                                     d_Sx if sx else None, None, d_ws, ws, C.byref(ms1)))
                acc[name].append(ms1.value)
            _lib.check(lib.ssq_ssq_stft2_exec(code, d_x, B, N, _vp(win), n_fft, hop, 1.0, 0, 0, -1.0, 3, d_Tx, d_Sx, None,
                                              d_ws, ws, C.byref(ms1)))
            acc["ssq_stft2"].append(ms1.value)
            for o in (1, 2):
                _lib.check(lib.ssq_tssq_stft_exec(code, d_x, B, N, _vp(win), n_fft, hop, 1.0, 0, o, -1.0, 3, d_Tx, d_Sx, None,
                                                  d_ws, ws, ms2))
                acc["tssq_o%d_operator" % o].append(ms2[0])
                acc["tssq_o%d_scatter" % o].append(ms2[1])
    finally:
        for d in bufs:
            if d:
                lib.ssq_dev_free(d)
    out = {k: _stats(v[1:]) for k, v in acc.items()}
    cells = B * F * nfr
    sig = B * N * (8 if code == _lib.SSQ_F64 else 4 + 8 + 8)
    out["GBps"] = {name: round((sig + cells * csize * (2 if sx else 1)) / out[name][0] / 1e6, 1) for name, a, o, sx in variants}
    return out


def table(recs):
    rows = ["# tools/bench_extract.py: kernel_ms, median [min .. max] over the timed passes after one warm-up pass, all variants",
            "# interleaved in one process.  set / tet: ssq_extract_stft_exec (ONE kernel; float32: with the widening), order 2 and 1,",
            "# Sx not stored / stored.  ssq_stft2: operator + scatter.  tssq: operator | time scatter."]
    for r in recs:
        rows.append("%s  batch %d x %d  n_fft %d  hop %d  reps %d" % (r["dtype"], r["batch"], r["n"], r["n_fft"], r["hop"], r["reps"]))
        for k, v in r.items():
            if isinstance(v, list):
                gb = r["GBps"].get(k)
                rows.append("  %-18s %9.3f  [%9.3f .. %9.3f] ms%s" % (k, v[0], v[1], v[2], "   %7.1f GB/s" % gb if gb else ""))
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--n-fft", type=int, default=1024)
    ap.add_argument("--hops", default="256,64")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    u = np.arange(a.n_fft) - a.n_fft // 2
    win = np.exp(-0.5 * (u / (a.n_fft / 10.0)) ** 2)
    recs = []
    for dt in (np.float32, np.float64):
        x = rng.standard_normal((a.batch, a.n)).astype(dt)
        for hop in (int(h) for h in a.hops.split(",")):
            rec = dict(dtype=np.dtype(dt).name, batch=a.batch, n=a.n, n_fft=a.n_fft, hop=hop, reps=a.reps)
            rec.update(run(x, win, a.n_fft, hop, a.reps))
            recs.append(rec)
            print(json.dumps(rec), flush=True)
            if a.out:                                        # (rewritten after every shape: a long run leaves what it has)
                with open(a.out, "w") as f:
                    f.write(table(recs))


if __name__ == "__main__":
    main()
