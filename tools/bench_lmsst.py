#!/usr/bin/env python
"""Kernel times of the local maximum synchrosqueezed transforms (`ssq_lmssq_stft_exec`: ONE kernel; `ssq_lmssq_cwt_exec`:
the transforms with the Wx kernel, the plane kernel, the squeeze), HIP events around the launches, everything resident on
the device, at delta 1, the default and 256 (the largest the shape admits), next to the transforms they are measured
against at the same shapes and from the same build: `ssq_ssq_stft2_exec` and `ssq_extract_stft_exec` (axis 0, order 1) on
the STFT, `ssq_ssq_cwt2_exec` on the CWT.

    python tools/bench_lmsst.py [--batch 64] [--n 262144] [--n-fft 1024] [--hop 256] [--cwt-batch 4] [--cwt-n 65536]
                                [--scales 128] [--reps 9] [--out FILE]

All variants of a shape run interleaved in the same process, pass after pass: one warm-up pass, then per variant the median
and the min..max over `--reps` timed passes.  A float32 STFT call's time includes the widening of its signals, in every
transform."""
import argparse
import ctypes as C
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from ssqueeze_rs_amd import _lib  # noqa: E402
from ssqueeze_rs_amd import upstream as up  # noqa: E402
from tools.bench_reassign_cwt import BETA, GAMMA, _grids  # noqa: E402

GMW = ("gmw", {"gamma": GAMMA, "beta": BETA})


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _stats(ts):
    return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]


def _alloc(lib, sizes):
    bufs = [C.c_void_p() for _ in sizes]
    for d, n in zip(bufs, sizes):
        _lib.check(lib.ssq_dev_malloc(C.byref(d), max(int(n), 16)))
    return bufs


def run_stft(x, win, n_fft, hop, reps):
    """-> (deltas, dict of [median, min, max] ms per variant)."""
    lib = _lib.load()
    B, N = x.shape
    code = _lib.SSQ_F32 if x.dtype == np.float32 else _lib.SSQ_F64
    F, nfr = n_fft // 2 + 1, (N - 1) // hop + 1
    map_bytes = B * F * nfr * 2 * x.dtype.itemsize
    ws = max(int(lib.ssq_lmssq_stft_workspace_bytes(code, B, N, n_fft, hop)),
             int(lib.ssq_extract_stft_workspace_bytes(code, B, N, n_fft, hop)),
             int(lib.ssq_ssq_stft2_workspace_bytes(code, B, N, n_fft, hop)))
    deltas = {"1": 1, "default": up.lmsst_default_delta(win, n_fft), "256": min(256, F - 1)}
    acc = {"lmssq_stft_delta_%s" % k: [] for k in deltas}
    acc.update(ssq_stft2=[], set_stft_o1=[])
    bufs = _alloc(lib, (x.nbytes, map_bytes, map_bytes, ws))
    d_x, d_Tx, d_Sx, d_ws = bufs
    try:
        _lib.check(lib.ssq_memcpy_h2d(d_x, _vp(x), x.nbytes, None))
        ms = C.c_float(0)
        for _ in range(1 + reps):
            for k, delta in deltas.items():
                _lib.check(lib.ssq_lmssq_stft_exec(code, d_x, B, N, _vp(win), n_fft, hop, 1.0, 0, 0, -1.0, 3, delta, d_Tx, d_Sx,
                                                   None, d_ws, ws, C.byref(ms)))
                acc["lmssq_stft_delta_%s" % k].append(ms.value)
            _lib.check(lib.ssq_ssq_stft2_exec(code, d_x, B, N, _vp(win), n_fft, hop, 1.0, 0, 0, -1.0, 3, d_Tx, d_Sx, None, d_ws,
                                              ws, C.byref(ms)))
            acc["ssq_stft2"].append(ms.value)
            _lib.check(lib.ssq_extract_stft_exec(code, d_x, B, N, _vp(win), n_fft, hop, 1.0, 0, 0, 1, -1.0, 3, d_Tx, d_Sx, None,
                                                 d_ws, ws, C.byref(ms)))
            acc["set_stft_o1"].append(ms.value)
    finally:
        for d in bufs:
            if d:
                lib.ssq_dev_free(d)
    return deltas, {k: _stats(v[1:]) for k, v in acc.items()}


def run_cwt(x, na, reps):
    """-> (deltas, dict of [median, min, max] ms per variant and part)."""
    lib = _lib.load()
    B, N = x.shape
    code = _lib.SSQ_F32 if x.dtype == np.float32 else _lib.SSQ_F64
    wcode, p0, p1 = up._wavelet(GMW)
    s, rowc, f = _grids(N, na)                               # (the grid of tools/bench_extract_cwt.py: 'log' frequencies)
    kind, f_idx = "log", None
    nu_hz = np.ascontiguousarray(up.tssq_cwt_row_freqs(GMW, s))
    cells = B * na * N
    cb, rb = cells * 2 * x.dtype.itemsize, cells * x.dtype.itemsize
    ws = max(int(lib.ssq_lmssq_cwt_workspace_bytes(code, B, N, na, None)), int(lib.ssq_ssq_cwt2_workspace_bytes(code, B, N, na, None)))
    deltas = {"1": 1, "default": up.lmssq_cwt_default_delta(GMW, s), "256": min(256, na - 1)}
    parts = ("transforms", "plane", "squeeze")
    acc = {"lmssq_cwt_delta_%s_%s" % (k, p): [] for k in deltas for p in parts}
    acc["ssq_cwt2"] = []
    bufs = _alloc(lib, (x.nbytes, cb, cb, rb, ws))
    d_x, d_Tx, d_Wx, d_w, d_ws = bufs
    try:
        _lib.check(lib.ssq_memcpy_h2d(d_x, _vp(x), x.nbytes, None))
        ms3, ms = (C.c_float * 3)(), C.c_float(0)
        for _ in range(1 + reps):
            for k, delta in deltas.items():
                _lib.check(lib.ssq_lmssq_cwt_exec(code, d_x, B, N, wcode, p0, p1, _vp(s), na, 1.0, _vp(rowc), _vp(f),
                                                  up.FREQS[kind], f_idx or 0, 0, 0, -1.0, up.VARIANT_FLIPUD, delta, _vp(nu_hz),
                                                  d_Tx, d_Wx, d_w, None, d_ws, ws, None, ms3))
                for j, p in enumerate(parts):
                    acc["lmssq_cwt_delta_%s_%s" % (k, p)].append(ms3[j])
            _lib.check(lib.ssq_ssq_cwt2_exec(code, d_x, B, N, wcode, p0, p1, _vp(s), na, 1.0, _vp(rowc), _vp(f), up.FREQS[kind],
                                             f_idx or 0, 0, 0, -1.0, up.VARIANT_FLIPUD, d_Tx, d_Wx, d_w, d_ws, ws, None,
                                             C.byref(ms)))
            acc["ssq_cwt2"].append(ms.value)
    finally:
        for d in bufs:
            if d:
                lib.ssq_dev_free(d)
    out = {k: _stats(v[1:]) for k, v in acc.items()}
    for k in deltas:
        tot = [sum(t) for t in zip(*(acc["lmssq_cwt_delta_%s_%s" % (k, p)][1:] for p in parts))]
        out["lmssq_cwt_delta_%s_total" % k] = _stats(tot)
    return deltas, out


def table(recs):
    rows = ["# tools/bench_lmsst.py: kernel_ms, median [min .. max] over the timed passes after one warm-up pass, the variants of a",
            "# shape interleaved in one process.  lmssq_stft: ssq_lmssq_stft_exec (ONE kernel; float32: with the widening).",
            "# ssq_stft2: operator + scatter.  set_stft_o1: ssq_extract_stft_exec, axis 0, order 1.  lmssq_cwt: the transforms with",
            "# the Wx kernel | the plane kernel (the window maximum) | the squeeze, and their sum.  ssq_cwt2: one figure."]
    for r in recs:
        rows.append(r["head"])
        for k, v in r["ms"].items():
            rows.append("  %-32s %9.3f  [%9.3f .. %9.3f] ms" % (k, v[0], v[1], v[2]))
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--n-fft", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--cwt-batch", type=int, default=4)
    ap.add_argument("--cwt-n", type=int, default=1 << 16)
    ap.add_argument("--scales", type=int, default=128)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    u = np.arange(a.n_fft) - a.n_fft // 2
    win = np.exp(-0.5 * (u / (a.n_fft / 10.0)) ** 2)
    recs = []

    def keep(rec):
        recs.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:                                            # (rewritten after every shape: a long run leaves what it has)
            with open(a.out, "w") as f:
                f.write(table(recs))
    for dt in (np.float32, np.float64):
        x = rng.standard_normal((a.batch, a.n)).astype(dt)
        deltas, ms = run_stft(x, win, a.n_fft, a.hop, a.reps)
        keep(dict(head="STFT %s  batch %d x %d  n_fft %d  hop %d  reps %d  deltas %s" % (
            np.dtype(dt).name, a.batch, a.n, a.n_fft, a.hop, a.reps, deltas), ms=ms))
    for dt in (np.float32, np.float64):
        x = rng.standard_normal((a.cwt_batch, a.cwt_n)).astype(dt)
        deltas, ms = run_cwt(x, a.scales, a.reps)
        keep(dict(head="CWT %s  batch %d x %d  %d log scales  reps %d  deltas %s" % (
            np.dtype(dt).name, a.cwt_batch, a.cwt_n, a.scales, a.reps, deltas), ms=ms))


if __name__ == "__main__":
    main()
