"""Time the device paths of `upstream.ssqueeze` / `phase_cwt` (ssqueeze.hip) with HIP events on warm device buffers
at the C4 shape, F = 256 rows by N = 2**20 columns, fp32 and fp64: ssq_phase_exec, ssq_ssqueeze_w_exec (squeezing
'sum', log frequencies) and ssq_ssqueeze_dwx_exec (the fused ssq_cwt's reassignment kernel).  Prints one JSON line per
case with the bytes the path must move (Wx and w or dWx read, Tx once: the clear streams it, the column walk adds
only the rows a column's bins hit) and the fraction of the 8 TB/s HBM peak.

    python tools/bench_ssqueeze.py [--reps 10] [--n 1048576] [--f 256]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssqueeze_rs_amd import _lib  # noqa: E402

PEAK_TBS = 8.0


def _ok(rc):
    _lib.check(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--f", type=int, default=256)
    a = ap.parse_args()
    lib = _lib.load()
    _lib.require_gpu()
    F, N = a.f, a.n
    freqs = np.ascontiguousarray(0.001 * 2.0 ** (np.arange(F) / 32))          # ascending, log-spaced
    fp = freqs.ctypes.data_as(C.c_void_p)
    for code, rdt in ((_lib.SSQ_F32, np.float32), (_lib.SSQ_F64, np.float64)):
        esz = np.dtype(rdt).itemsize
        n = F * N
        # a chirp per row: w finite everywhere, the rows of a column land in a few bins (runs merge in registers)
        t = np.arange(N)
        f0 = (0.002 + 0.1 * t / N)[None, :] * (1 + 0.05 * np.arange(F)[:, None] / F)
        Wh = (np.exp(2j * np.pi * f0 * t) * (1 + np.arange(F)[:, None] / F)).astype(np.complex128 if esz == 8 else
                                                                                    np.complex64)
        dWh = (2j * np.pi * f0 * Wh).astype(Wh.dtype)
        ptr = {}
        for name, nbytes in (("W", 2 * n * esz), ("dW", 2 * n * esz), ("w", n * esz), ("T", 2 * n * esz),
                             ("c", F * esz)):
            p = C.c_void_p()
            _ok(lib.ssq_dev_malloc(C.byref(p), nbytes))
            ptr[name] = p
        _ok(lib.ssq_memcpy_h2d(ptr["W"], Wh.ctypes.data_as(C.c_void_p), 2 * n * esz, None))
        _ok(lib.ssq_memcpy_h2d(ptr["dW"], dWh.ctypes.data_as(C.c_void_p), 2 * n * esz, None))
        c = np.full(F, np.log(2) / 32, dtype=rdt)
        _ok(lib.ssq_memcpy_h2d(ptr["c"], c.ctypes.data_as(C.c_void_p), F * esz, None))
        del Wh, dWh
        _ok(lib.ssq_device_sync())
        gamma = 10 * float(np.finfo(rdt).eps)
        cases = {
            "phase_cwt": (lambda: lib.ssq_phase_exec(code, ptr["W"], ptr["dW"], None, 1, F, N, gamma, ptr["w"], None),
                          (2 * 2 * esz + esz) * n),
            "ssqueeze_w": (lambda: lib.ssq_ssqueeze_w_exec(code, ptr["W"], ptr["w"], 1, F, N, ptr["c"], fp, 0, 0, 0,
                                                           1, ptr["T"], None),
                           (2 * esz + esz + 2 * esz) * n),
            "ssqueeze_dwx": (lambda: lib.ssq_ssqueeze_dwx_exec(code, ptr["W"], ptr["dW"], None, 1, F, N, ptr["c"], fp,
                                                               0, 0, 0, 1, gamma, ptr["T"], None),
                             (2 * esz + 2 * esz + 2 * esz) * n),
        }
        ev0, ev1 = C.c_void_p(), C.c_void_p()
        _ok(lib.ssq_event_create(C.byref(ev0)))
        _ok(lib.ssq_event_create(C.byref(ev1)))
        for name, (fn, nbytes) in cases.items():
            _ok(fn())                                                          # warm-up
            _ok(lib.ssq_device_sync())
            ms = []
            for _ in range(a.reps):
                _ok(lib.ssq_event_record(ev0, None))
                _ok(fn())
                _ok(lib.ssq_event_record(ev1, None))
                _ok(lib.ssq_event_sync(ev1))
                m = C.c_float()
                _ok(lib.ssq_event_elapsed_ms(ev0, ev1, C.byref(m)))
                ms.append(m.value)
            med = float(np.median(ms))
            print(json.dumps({"case": name, "dtype": "fp32" if esz == 4 else "fp64", "F": F, "N": N,
                              "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "gbytes": round(nbytes / 1e9, 3),
                              "tb_s": round(nbytes / med / 1e9, 3),
                              "frac_of_8tbs": round(nbytes / med / 1e9 / PEAK_TBS, 4)}), flush=True)
        _ok(lib.ssq_event_destroy(ev0))
        _ok(lib.ssq_event_destroy(ev1))
        for p in ptr.values():
            _ok(lib.ssq_dev_free(p))


if __name__ == "__main__":
    main()
