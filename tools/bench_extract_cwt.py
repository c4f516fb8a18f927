#!/usr/bin/env python
"""Kernel times of the synchroextracting / transient-extracting CWT (`ssq_extract_cwt_exec`: padding, the forward
transform, two (order 1) or five (order 2) product spectra and inverse transforms a row and ONE operator kernel; HIP events
around the launches, everything resident on the device), both axes, orders 1 and 2, with Wx stored and not stored, next to
the transforms whose maps it reads, at the same shape and from the same build: `ssq_ssq_cwt2_exec` (operator + scatter, one
figure) and `ssq_tssq_cwt_exec` (everything before the scatter -- its operator part -- and the scatter kernel apart),
orders 1 and 2.

    python tools/bench_extract_cwt.py [--batch 4] [--n 65536] [--na 128] [--reps 9] [--out FILE]

GMW(3, 60), log scales from the Nyquist peak down to N/4 samples per cycle (tools/bench_reassign_cwt.py's grid), white
noise.  All variants run interleaved in the same process, pass after pass: one warm-up pass, then per variant the median
and the min..max over `--reps` timed passes."""
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

AXES = {"set": 0, "tet": 1}
WAVELET = ("gmw", {"gamma": GAMMA, "beta": BETA})


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _stats(ts):
    return [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)]


def run(x, na, reps):
    """-> dict of [median, min, max] ms per variant, and the workspaces in MB."""
    lib = _lib.load()
    B, N = x.shape
    code = _lib.SSQ_F32 if x.dtype == np.float32 else _lib.SSQ_F64
    scales, rc, f = _grids(N, na)
    nu = up.tssq_cwt_row_freqs(WAVELET, scales)
    edges = up.set_cwt_row_edges(WAVELET, scales)
    cells = B * na * N
    cbytes = cells * 2 * x.dtype.itemsize
    ws_e = {o: int(lib.ssq_extract_cwt_workspace_bytes(code, B, N, na, o, None)) for o in (1, 2)}
    ws_t = {o: int(lib.ssq_tssq_cwt_workspace_bytes(code, B, N, na, o, None)) for o in (1, 2)}
    ws_2 = int(lib.ssq_ssq_cwt2_workspace_bytes(code, B, N, na, None))
    ws = max(ws_2, *ws_e.values(), *ws_t.values())
    bufs = [C.c_void_p() for _ in range(5)]
    d_x, d_Tx, d_Wx, d_w, d_ws = bufs
    variants = [("%s_o%d_%s" % (a, o, "Wx" if wx else "noWx"), a, o, wx) for a in AXES for o in (2, 1) for wx in (False, True)]
    acc = {v[0]: [] for v in variants}
    for k in ("ssq_cwt2", "tssq_o1_operator_part", "tssq_o1_scatter", "tssq_o1_all", "tssq_o2_operator_part", "tssq_o2_scatter",
              "tssq_o2_all"):
        acc[k] = []
    try:
        for d, n in zip(bufs, (x.nbytes, cbytes, cbytes, cbytes // 2, ws)):
            _lib.check(lib.ssq_dev_malloc(C.byref(d), n))
        _lib.check(lib.ssq_memcpy_h2d(d_x, _vp(x), x.nbytes, None))
        ms3, ms1 = (C.c_float * 3)(), C.c_float(0)
        for i in range(1 + reps):
            for name, a, o, wx in variants:
                _lib.check(lib.ssq_extract_cwt_exec(code, d_x, B, N, 0, GAMMA, BETA, _vp(scales), _vp(nu), _vp(edges), na, 1.0, 0,
                                                    AXES[a], o, -1.0, d_Tx, d_Wx if wx else None, None, d_ws, ws_e[o], None,
                                                    C.byref(ms1)))
                acc[name].append(ms1.value)
            _lib.check(lib.ssq_ssq_cwt2_exec(code, d_x, B, N, 0, GAMMA, BETA, _vp(scales), na, 1.0, _vp(rc), _vp(f), 0, 0, 0, 0,
                                             -1.0, 4, d_Tx, d_Wx, d_w, d_ws, ws_2, None, C.byref(ms1)))
            acc["ssq_cwt2"].append(ms1.value)
            for o in (1, 2):
                _lib.check(lib.ssq_tssq_cwt_exec(code, d_x, B, N, 0, GAMMA, BETA, _vp(scales), _vp(nu), na, 1.0, 0, o, -1.0, d_Tx,
                                                 d_Wx, None, None, d_ws, ws_t[o], None, ms3))
                acc["tssq_o%d_all" % o].append(ms3[0])
                acc["tssq_o%d_scatter" % o].append(ms3[1])
                acc["tssq_o%d_operator_part" % o].append(ms3[2])
    finally:
        for d in bufs:
            if d:
                lib.ssq_dev_free(d)
    out = {k: _stats(v[1:]) for k, v in acc.items()}
    out["workspace_MB"] = dict(extract_o1=round(ws_e[1] / 2 ** 20, 1), extract_o2=round(ws_e[2] / 2 ** 20, 1),
                               tssq_o1=round(ws_t[1] / 2 ** 20, 1), tssq_o2=round(ws_t[2] / 2 ** 20, 1),
                               ssq_cwt2=round(ws_2 / 2 ** 20, 1))
    return out


def table(recs):
    rows = ["# tools/bench_extract_cwt.py: kernel_ms, median [min .. max] over the timed passes after one warm-up pass, all",
            "# variants interleaved in one process.  set / tet: ssq_extract_cwt_exec (all its kernels), order 2 and 1, Wx not",
            "# stored / stored.  ssq_cwt2: all its kernels (operator + scatter).  tssq: everything before the scatter (its",
            "# operator part), the scatter kernel alone, all its kernels (with the read-out)."]
    for r in recs:
        rows.append("%s  batch %d x %d  na %d  reps %d  workspace MB %s" % (r["dtype"], r["batch"], r["n"], r["na"], r["reps"],
                                                                          json.dumps(r["workspace_MB"])))
        for k, v in r.items():
            if isinstance(v, list):
                rows.append("  %-24s %9.3f  [%9.3f .. %9.3f] ms" % (k, v[0], v[1], v[2]))
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--n", type=int, default=1 << 16)
    ap.add_argument("--na", type=int, default=128)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    recs = []
    for dt in (np.float32, np.float64):
        x = rng.standard_normal((a.batch, a.n)).astype(dt)
        rec = dict(dtype=np.dtype(dt).name, batch=a.batch, n=a.n, na=a.na, reps=a.reps)
        rec.update(run(x, a.na, a.reps))
        recs.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:                                            # (rewritten after every dtype: a long run leaves what it has)
            with open(a.out, "w") as f:
                f.write(table(recs))


if __name__ == "__main__":
    main()
