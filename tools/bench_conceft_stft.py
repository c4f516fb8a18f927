#!/usr/bin/env python
"""Kernel times of `conceft_stft` (`ssq_conceft_stft_exec`, its kernel_ms: the stage-2 squeeze kernel alone and the
stage-1 plane kernel alone, HIP events around their launches, everything resident on the device) beside what the same
work cost before it existed:

    (a) squeeze_ms      the stage-2 kernel: the 2 J planes read once per chunk of 8 draws, every draw combined, binned
                        and summed in registers, one Tx written
    (b) m_squeezes_ms   M x batch x the time of `ssq_ssqueeze_dwx_exec` (its clear of Tx and its kernel, HIP events) on ONE
                        device-resident [F, n_frames] plane pair: the M squeezes alone, the combinations free
    planes_ms           the stage-1 kernel (J packed transforms per frame), beside
    stft2_ms            `ssq_ssq_stft2_exec`'s kernel_ms on the same frames with taper 0: its clear of Tx, its operator
                        kernel (three transforms per frame and the second-order operator) and its scatter

    python tools/bench_conceft_stft.py [--batch 4] [--n 65536] [--n-fft 1024] [--tapers 3] [--reps 7] [--out FILE]

Hermite tapers, hop 1 and hop 16, M in {8, 20, 64}, float32 and float64, and the workspace at 128 MiB, 1 GiB (the
preferred size) and 4 GiB.  The signals are a chirp (long runs of rows in one bin: the best case for combining runs) and
white noise (the worst).  Median and min..max over `--reps` repeats after two warm-up runs, (a) and (b) alternating inside
every repeat."""
import argparse
import ctypes as C
import json
import statistics
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from ssqueeze_rs_amd import _lib  # noqa: E402
from ssqueeze_rs_amd import upstream as up  # noqa: E402

DRAWS = (8, 20, 64)
HOPS = (1, 16)
WORKSPACES = (128 << 20, 1 << 30, 4 << 30)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _stats(ts):
    return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]


def signals(batch, n, dtype):
    t = np.arange(n, dtype=np.float64)
    chirp = np.cos(2 * np.pi * (0.02 * t + 0.5 * (0.4 / n) * t * t))
    rng = np.random.default_rng(0)
    return {"chirp": np.ascontiguousarray(np.tile(chirp, (batch, 1)).astype(dtype)),
            "noise": np.ascontiguousarray(rng.standard_normal((batch, n)).astype(dtype))}


class DevBufs:
    def __init__(self, lib, sizes):
        self.lib, self.bufs = lib, [C.c_void_p() for _ in sizes]
        for d, n in zip(self.bufs, sizes):
            _lib.check(lib.ssq_dev_malloc(C.byref(d), int(n)))

    def free(self):
        for d in self.bufs:
            if d:
                self.lib.ssq_dev_free(d)


def run(x, n_fft, hop, J, reps):
    """-> records (dicts) of one dtype, signal and hop."""
    lib = _lib.load()
    B, N = x.shape
    f32 = x.dtype == np.float32
    code = _lib.SSQ_F32 if f32 else _lib.SSQ_F64
    csz = 8 if f32 else 16
    F, nfr = n_fft // 2 + 1, (N - 1) // hop + 1
    h = np.ascontiguousarray(up.hermite_windows(n_fft, J))
    adm = h[:, n_fft // 2]
    Sfs = np.linspace(0, 0.5, F)
    SfsT = np.ascontiguousarray(Sfs.astype(x.dtype))
    mn = C.c_int64(0)
    _lib.check(0 if lib.ssq_conceft_stft_workspace_bytes(code, B, N, n_fft, hop, J, C.byref(mn)) > 0 else 1)
    need = B * ((8 * N if f32 else 0) + 2 * J * F * nfr * csz)             # the whole batch in one slice
    sizes = [max(mn.value, min(w, need)) for w in WORKSPACES]
    ws2 = int(lib.ssq_ssq_stft2_workspace_bytes(code, B, N, n_fft, hop))
    plane = F * nfr * csz
    # x, Tx, workspace, one plane pair and its Tx, Sfs, ssq_stft2's Sx and workspace
    d = DevBufs(lib, (x.nbytes, B * plane, max(sizes), plane, plane, plane, SfsT.nbytes, B * plane, ws2))
    out = []
    try:
        dx, dTx, dwork, dS1, ddS1, dT1, dSfs, dSx2, dwork2 = d.bufs
        _lib.check(lib.ssq_memcpy_h2d(dx, _vp(x), x.nbytes, None))
        _lib.check(lib.ssq_memcpy_h2d(dSfs, _vp(SfsT), SfsT.nbytes, None))
        e0 = np.array([[1.0 + 0j]])
        var = up._variant(True)
        # the resident plane pair of (b): V_0, V1_0 of the first signal
        _lib.check(lib.ssq_conceft_stft_exec(code, dx, 1, N, _vp(h), 1, n_fft, hop, 1.0, 0, _vp(e0), 1, 1.0, -1.0, var, dT1, dS1,
                                             ddS1, None, dwork, sizes[0], None, None))
        ev = [C.c_void_p() for _ in range(2)]
        for e in ev:
            _lib.check(lib.ssq_event_create(C.byref(e)))
        gamma = 10 * float(np.finfo(x.dtype).eps)
        for M in DRAWS:
            r, c = up._conceft_gauge(up._conceft_draws(M, J, 0), adm)
            scale = float(adm[0] / c.sum())
            ms = (C.c_float * 2)(0, 0)
            ta = {w: [] for w in sizes}
            tp = {w: [] for w in sizes}
            tb, t2 = [], []
            for i in range(2 + reps):
                for w in dict.fromkeys(sizes):
                    _lib.check(lib.ssq_conceft_stft_exec(code, dx, B, N, _vp(h), J, n_fft, hop, 1.0, 0, _vp(r), M, scale, -1.0,
                                                         var, dTx, None, None, None, dwork, w, None, ms))
                    if i >= 2:
                        ta[w].append(ms[0])
                        tp[w].append(ms[1])
                _lib.check(lib.ssq_event_record(ev[0], None))
                _lib.check(lib.ssq_ssqueeze_dwx_exec(code, dS1, ddS1, dSfs, 1, F, nfr, None, _vp(Sfs), 1, 0, 0, 0, gamma, dT1,
                                                     None))
                _lib.check(lib.ssq_event_record(ev[1], None))
                _lib.check(lib.ssq_event_sync(ev[1]))
                one = C.c_float(0)
                _lib.check(lib.ssq_event_elapsed_ms(ev[0], ev[1], C.byref(one)))
                k2 = C.c_float(0)
                _lib.check(lib.ssq_ssq_stft2_exec(code, dx, B, N, _vp(h[0]), n_fft, hop, 1.0, 0, 0, -1.0, var, dTx, dSx2, None,
                                                  dwork2, ws2, C.byref(k2)))
                if i >= 2:
                    tb.append(one.value * B * M)               # one signal's plane pair x the batch x the draws
                    t2.append(k2.value)
            for w in dict.fromkeys(sizes):
                a, b = _stats(ta[w]), _stats(tb)
                out.append(dict(dtype=x.dtype.name, batch=B, n=N, n_fft=n_fft, hop=hop, tapers=J, draws=M, reps=reps,
                                workspace_mib=round(w / 2 ** 20, 1), squeeze_ms=a, m_squeezes_ms=b,
                                ratio_b_over_a=round(b[0] / a[0], 2) if a[0] > 0 else None, planes_ms=_stats(tp[w]),
                                stft2_ms=_stats(t2)))
        for e in ev:
            lib.ssq_event_destroy(e)
    finally:
        d.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--n", type=int, default=1 << 16)
    ap.add_argument("--n-fft", type=int, default=1024)
    ap.add_argument("--tapers", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    lines = []
    for dt in (np.float32, np.float64):
        for name, x in signals(a.batch, a.n, dt).items():
            for hop in HOPS:
                for rec in run(x, a.n_fft, hop, a.tapers, a.reps):
                    lines.append(json.dumps(dict(signal=name, **rec)))
                    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/bench_conceft_stft.py: [median, min, max] in ms over the timed repeats.  squeeze_ms (a): the "
                    "stage-2 kernel of ssq_conceft_stft_exec alone, summed over the slices of a workspace of workspace_mib.  "
                    "m_squeezes_ms (b): batch x draws x the time of ssq_ssqueeze_dwx_exec (clear + kernel) on one resident "
                    "[F, n_frames] plane pair, measured in the same repeat.  ratio_b_over_a: the medians.  planes_ms: the "
                    "stage-1 kernel alone (J packed transforms a frame).  stft2_ms: ssq_ssq_stft2_exec's kernel_ms on the "
                    "same frames (clear, the three-transform operator kernel, scatter).\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
