#!/usr/bin/env python3
"""bench.py -- headline benchmark: TF-bins/s of ssq_stft (n_fft=1024, hop=256, fp32) on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B | --total-batch B] [--gather] [--dump-outputs DIR]
                    [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ...

One "step" = one pass of the fused ssq_stft hot path over one batch of synthetic signals of 2^20 samples resident
in HBM.  Default: B = 256 signals per GPU (BASELINE.json's target workload "batch=256 x 2^20-sample signals on
1xMI355X"); with N GPUs every rank processes its own B signals -> weak scaling, no data-path collective.
`--total-batch B` instead splits ONE batch of B signals over the ranks by contiguous blocks (BASELINE config 3:
256 signals -> 32 per GPU at N = 8) -> strong scaling.  Rank 0 prints ONE JSON line.

The number of GPUs is the WORLD SIZE, never the flag: under torch.distributed.run `--gpus` must equal WORLD_SIZE
(exit 2 otherwise); started as plain `python bench.py --gpus N` with N > 1 the script launches the N rank
processes itself (fresh children through torch.distributed.run, before this process touches any GPU) and
relays their JSON line and exit code.

A plain run does only what the headline figure needs: it sets up, runs in, warms up, times the K steps, writes its
outputs if asked and prints the line.  `--full` adds everything else the bench measures or checks: the validation
below, the secondary legs (one C2 signal, fp64, the C4 / C5 ssq_cwt legs) and the CPU baselines, each of them still
skipped by its own `--no-*` option.

With `--full` the bench checks what it times, outside the timed region: three signals of the batch are copied back and
compared bitwise with the single-signal path of the same library, and signal 0 with the committed BASELINE-config-2
checksums (tests/golden/c2_summary.npz) -> "validated".

`--dump-outputs DIR` writes what the last timed step left in Tx (rank 0's signals) as .npy files, float32 with a
trailing (real, imag) axis: whole signals 0, B/2 and B-1 as far as they fit, and a fixed seeded sample of single bins
over the whole batch, under 64 MiB in all (see dump_plan).  The inputs are seeded, so two builds run with the same
arguments can be compared file by file.

torch is plumbing only (process group, barrier, torch.cuda.synchronize, the buffer handed to RCCL); the
stream, the HIP events and the kernels all come from libssq_hip.so through its C-ABI.
"""
import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_MEASURED_COPY_GBS = 6290.0   # MI355X_MICROARCH.md: HBM3E 6.29 TB/s measured (float4 copy)
HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec peak (MI355X_MICROARCH.md, chip-level parameters)
TRAFFIC_FILE = os.path.join("profiles", "r03_traffic.json")
TRAFFIC_FILE_F64 = os.path.join("profiles", "r03_traffic_f64.json")      # the fp64 leg's own PMC passes (tools/pmc_f64.sh)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256, help="signals per GPU (weak scaling)")
    ap.add_argument("--total-batch", type=int, default=0,
                    help="signals in the whole job, split over the ranks (strong scaling; BASELINE config 3 = 256)")
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--n-fft", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=0,
                    help="distinct synthetic signals per rank (0 = all of them distinct); fewer are tiled to the batch")
    ap.add_argument("--full", action="store_true",
                    help="also validate what is timed and run the secondary legs and the CPU baselines")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the secondary legs")
    ap.add_argument("--no-validate", action="store_true", help="with --full: skip the validation")
    ap.add_argument("--settle-ms", type=float, default=80.0,
                    help="untimed run-in of the same step before the W warm-up steps (reported as settle_ms): the first "
                         "~30 ms of this kernel after any gap run 5-8 %% slower than its steady state (clock ramp)")
    ap.add_argument("--no-c5", action="store_true",
                    help="with --full: skip the fp64 BASELINE-config-5 secondary legs (17 - 170 GB)")
    ap.add_argument("--gather", action="store_true", help="also time the optional RCCL all_gather of the Tx shards")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write rank 0's Tx of the last step (whole signals + a seeded sample) "
                         "as DIR/<name>.npy")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    return args


# ----------------------------------------------------------------------------------------------- launcher ----
def world_from_env(env=None):
    """(world, rank, local_rank) of this process; (1, 0, 0) when not started by torch.distributed.run."""
    env = os.environ if env is None else env
    if "RANK" in env and "WORLD_SIZE" in env:
        return int(env["WORLD_SIZE"]), int(env["RANK"]), int(env.get("LOCAL_RANK", env["RANK"]))
    return 1, 0, 0


def launch_plan(gpus, env=None):
    """What this process has to do, decided before anything touches a GPU:
    ("run", world, rank, local_rank)  -- be a rank (world == gpus), or
    ("spawn", gpus)                   -- plain `python bench.py --gpus N`, N > 1: start N rank processes, or
    ("error", message)                -- --gpus disagrees with the world size the launcher gave us."""
    env = os.environ if env is None else env
    world, rank, local_rank = world_from_env(env)
    in_dist = "RANK" in env and "WORLD_SIZE" in env
    if in_dist:
        if gpus != world:
            return ("error", f"--gpus {gpus} disagrees with WORLD_SIZE {world}: the number of GPUs is the world size")
        return ("run", world, rank, local_rank)
    if gpus > 1:
        return ("spawn", gpus)
    if gpus < 1:
        return ("error", "--gpus must be >= 1")
    return ("run", 1, 0, 0)


def free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(n, argv, script=None, extra_env=None):
    """Start n fresh rank processes through torch.distributed.run (this process has made no GPU call) and wait.
    Their stdout (rank 0's JSON line) passes straight through; returns the launcher's exit code."""
    script = script or os.path.abspath(__file__)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), script] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if extra_env:
        env.update(extra_env)
    return subprocess.call(cmd, env=env)


def job_shape(world, rank, batch, total_batch):
    """(signals of this rank, first global signal index, signals of the whole job, scaling)."""
    from ssqueeze_rs_amd.batch import shard_bounds
    if total_batch > 0:
        lo, hi = shard_bounds(total_batch, world, rank)
        return hi - lo, lo, total_batch, "strong"
    return batch, rank * batch, batch * world, "weak"


# ------------------------------------------------------------------------------------------------- pieces ----
def measured_traffic(B, log2n, n_fft, hop, file=None):
    """HBM bytes per launch from the committed PMC run of this kernel (separate rocprofv3 --pmc FETCH_SIZE /
    WRITE_SIZE passes, gfx950 correction applied; see profiles/README.md).  Counters cannot be read from inside
    the timed process, so this is a per-signal figure scaled to the batch; other shapes -> None."""
    try:
        with open(os.path.join(ROOT, file or TRAFFIC_FILE)) as f:
            t = json.load(f)
        w = t["workload"]
        if (w["log2n"], w["n_fft"], w["hop"]) != (log2n, n_fft, hop):
            return None
        return int(t["bytes_per_signal"] * B)
    except (OSError, KeyError, ValueError):
        return None


SYNTH_THREADS = 16                 # host threads that generate the inputs (NumPy releases the GIL in its loops)


def synth_rows(first, count, N, dtype):
    """Signals first .. first + count - 1 as [count, N] rows, generated on up to SYNTH_THREADS host threads: each row
    is synth_signal's own result, so the rows do not depend on the number of threads."""
    from concurrent.futures import ThreadPoolExecutor
    from ssqueeze_rs_amd.synth import synth_signal   # synthetic workload generator
    out = np.empty((count, N), dtype=dtype)

    def fill(b):
        out[b] = synth_signal(N, first + b, dtype)

    with ThreadPoolExecutor(max_workers=max(1, min(count, SYNTH_THREADS, len(os.sched_getaffinity(0))))) as ex:
        list(ex.map(fill, range(count)))
    return out


def cpu_baseline(N, n_fft, hop, budget_s=20.0):
    """The oracle's C restatement of the reference CPU path (oracle/ssq_ref.c, kind "port"), timed on
    this box's host cores on a bounded sample of the same workload."""
    from oracle import ref_c                         # the only use of oracle/ here: the timed CPU baseline
    from ssqueeze_rs_amd.synth import synth_signal
    win = np.hanning(n_fft)
    cores = ref_c.num_threads()
    bins = (n_fft // 2 + 1) * ((N - 1) // hop + 1)
    out = {}
    for mode, name in ((0, "faithful"), (1, "optimized")):
        done, t_total = 0, 0.0
        while done < 64 and t_total < budget_s / 2:
            x = synth_signal(N, done, np.float64)
            t0 = time.perf_counter()
            ref_c.ssq_stft(x, win, n_fft, hop, fs=1.0, mode=mode)
            t_total += time.perf_counter() - t0
            done += 1
        out[name] = (bins * done / t_total, done, t_total)
    v, done, tt = out["faithful"]
    return {
        "value": v, "unit": "TF-bins/s", "cores": cores, "kind": "port",
        "sample": f"{done} signal(s) x 2^{int(np.log2(N))} samples, fp64, reference-faithful structure "
                  f"(2 scalar radix-2 FFTs/frame, C built -march=x86-64-v2, over {cores} OpenMP threads; serial phase, "
                  f"serial linear-scan reassignment), "
                  f"{tt:.1f} s",
        "optimized_value": out["optimized"][0],
        "optimized_sample": f"{out['optimized'][1]} signal(s), arithmetic binning + column-parallel reassignment, "
                            f"{out['optimized'][2]:.1f} s",
    }


class Leg:
    """One device-resident ssq_stft workload: plan + buffers + HIP-event timing on the launch stream."""

    def __init__(self, lib, _lib, dtype, N, n_fft, hop, B, stream, d_out_ptr=None):
        self.lib, self._lib = lib, _lib
        self.f32 = dtype == np.float32
        self.esz = 4 if self.f32 else 8
        self.N, self.n_fft, self.hop, self.B, self.stream = N, n_fft, hop, B, stream
        self.n_freqs, self.n_frames = n_fft // 2 + 1, (N - 1) // hop + 1
        self.bins = self.n_freqs * self.n_frames
        self.alg_bytes_per_signal = self.esz * N + 2 * self.esz * self.bins     # x in once, Tx out once
        win = np.hanning(n_fft)
        self.plan = C.c_void_p()
        _lib.check(lib.ssq_stft_plan_create(C.byref(self.plan), _lib.SSQ_F32 if self.f32 else _lib.SSQ_F64, N,
                                            win.ctypes.data_as(C.c_void_p), n_fft, hop, 1.0, 0, 0, -1.0, 0))
        assert lib.ssq_stft_plan_is_fused(self.plan) == 1
        self.d_x = C.c_void_p()
        _lib.check(lib.ssq_dev_malloc(C.byref(self.d_x), B * N * self.esz))
        self.own_out = d_out_ptr is None
        self.d_out = C.c_void_p()
        if self.own_out:
            _lib.check(lib.ssq_dev_malloc(C.byref(self.d_out), B * self.bins * 2 * self.esz))
        else:
            self.d_out = C.c_void_p(d_out_ptr)
        self.d_one = C.c_void_p()
        _lib.check(lib.ssq_dev_malloc(C.byref(self.d_one), self.bins * 2 * self.esz))

    def upload(self, host):
        """host: [nd, N] rows, tiled to the batch."""
        nd = host.shape[0]
        for b in range(self.B):
            row = host[b % nd]
            self._lib.check(self.lib.ssq_memcpy_h2d(C.c_void_p(self.d_x.value + b * self.N * self.esz),
                                                    row.ctypes.data_as(C.c_void_p), self.N * self.esz, self.stream))
        self._lib.check(self.lib.ssq_stream_sync(self.stream))

    n_step_calls = 0          # launches of the batch pass so far (= dispatches of the interior-tile kernel)
    timed_first = None        # index of the first TIMED one: tools/trace_timed.py cuts a rocprofv3 kernel trace there

    def step(self):
        self.n_step_calls += 1
        self._lib.check(self.lib.ssq_stft_plan_exec(self.plan, self._lib.OUT_TX, self.d_x, self.B, self.d_out,
                                                    None, 0, self.stream))

    def timed(self, steps, warmup, before=None, after=None, settle_ms=0.0):
        """`steps` timed steps bracketed by `before()` / `after()` (barrier + synchronize); returns
        (wall seconds, per-step kernel ms from HIP events recorded on the launch stream)."""
        lib, _lib = self.lib, self._lib
        t_end = time.perf_counter() + settle_ms * 1e-3
        while time.perf_counter() < t_end:               # untimed run-in (see --settle-ms)
            for _ in range(4):
                self.step()
            _lib.check(lib.ssq_stream_sync(self.stream))
        for _ in range(warmup):
            self.step()
        _lib.check(lib.ssq_stream_sync(self.stream))
        evs = []
        for _ in range(steps):
            a, b_ = C.c_void_p(), C.c_void_p()
            _lib.check(lib.ssq_event_create(C.byref(a)))
            _lib.check(lib.ssq_event_create(C.byref(b_)))
            evs.append((a, b_))
        if before:
            before()
        self.timed_first = self.n_step_calls
        t0 = time.perf_counter()
        for a, b_ in evs:
            _lib.check(lib.ssq_event_record(a, self.stream))
            self.step()
            _lib.check(lib.ssq_event_record(b_, self.stream))
        _lib.check(lib.ssq_stream_sync(self.stream))
        if after:
            after()
        wall = time.perf_counter() - t0
        kern = []
        for a, b_ in evs:
            ms = C.c_float(0)
            _lib.check(lib.ssq_event_elapsed_ms(a, b_, C.byref(ms)))
            kern.append(ms.value)
            lib.ssq_event_destroy(a)
            lib.ssq_event_destroy(b_)
        return wall, kern

    def fetch(self, b):
        """Tx of signal b of the batch as it stands in HBM."""
        cd = np.complex64 if self.f32 else np.complex128
        out = np.empty((self.n_freqs, self.n_frames), dtype=cd)
        self._lib.check(self.lib.ssq_memcpy_d2h(out.ctypes.data_as(C.c_void_p),
                                                C.c_void_p(self.d_out.value + b * self.bins * 2 * self.esz),
                                                out.nbytes, self.stream))
        self._lib.check(self.lib.ssq_stream_sync(self.stream))
        return out

    def single(self, b, kind=None):
        """Signal b through the single-signal path (batch = 1: one launch of the edge-capable kernel)."""
        cd = np.complex64 if self.f32 else np.complex128
        self._lib.check(self.lib.ssq_stft_plan_exec(self.plan, self._lib.OUT_TX if kind is None else kind,
                                                    C.c_void_p(self.d_x.value + b * self.N * self.esz), 1,
                                                    self.d_one, None, 0, self.stream))
        out = np.empty((self.n_freqs, self.n_frames), dtype=cd)
        self._lib.check(self.lib.ssq_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.d_one, out.nbytes, self.stream))
        self._lib.check(self.lib.ssq_stream_sync(self.stream))
        return out

    def validate(self, first_seed):
        """Outside the timed region: the batch result against the single-signal path (bitwise: the fixed-point tile
        is order-exact) and, when signal 0 is seed 0 of the C2 shape, against the committed C2 checksums."""
        self.step()
        self._lib.check(self.lib.ssq_stream_sync(self.stream))
        idx = sorted({0, self.B // 2, self.B - 1})
        rep = {"signals_checked": idx, "bitwise_equal_single_signal_path": True}
        t0 = None
        for b in idx:
            got = self.fetch(b)
            if b == 0:
                t0 = got
            if not np.array_equal(got, self.single(b)):
                rep["bitwise_equal_single_signal_path"] = False
        ok = rep["bitwise_equal_single_signal_path"] and bool(np.isfinite(t0.view(t0.real.dtype)).all())
        gpath = os.path.join(ROOT, "tests", "golden", "c2_summary.npz")
        rep["golden_checked"] = False            # true only when signal 0 IS the C2 signal and the fixtures are present
        if first_seed == 0 and (self.N, self.n_fft, self.hop) == (1 << 20, 1024, 256) and os.path.exists(gpath):
            g = np.load(gpath)
            dw = 0.5 / (self.n_freqs - 1)
            scale = float(g["sx_absmax"]) * dw
            e_col = float(np.abs(t0.astype(np.complex128).sum(0) - g["col_sums"]).max() / scale)
            e_row = float(np.abs(np.abs(t0).sum(1) - g["row_energy"]).max() / g["row_energy"].max())
            rep["c2_colsum_relerr"] = e_col       # column sums are invariant under bin flips (measured 8.6e-7 fp32)
            rep["c2_row_energy_relerr"] = e_row   # measured 4.1e-5 fp32: the bound is ~10x that, not a loose 2e-2
            tol_col = 1e-5 if self.f32 else 1e-9
            tol_row = 5e-4 if self.f32 else 1e-8
            ok = ok and e_col <= tol_col and e_row <= tol_row
            rep["golden_checked"] = True
            kpath = os.path.join(ROOT, "tests", "golden", "c2_k_cols.npz")
            if os.path.exists(kpath):
                # end-to-end bin parity: the Tx kernel's OWN bins (SSQ_OUT_WK hook of the timed kernel) against the
                # fp64 oracle's on 256 frames -- the measured mismatch rate SURVEY 8(c) asks to report
                gk = np.load(kpath)
                wk = self.single(0, kind=self._lib.OUT_WK)
                k_own = np.rint(wk.imag[:, gk["col_index"]]).astype(np.int64)
                k_or = gk["k"].astype(np.int64)
                shp = tuple(int(v) for v in gk["shape"])
                strong = np.unpackbits(gk["strong"])[: shp[0] * shp[1]].reshape(shp).astype(bool)
                both = strong & (k_own >= 0) & (k_or >= 0)
                rate = float((k_own[both] != k_or[both]).mean())
                rep["bin_mismatch_rate_vs_fp64_oracle"] = rate          # measured 1.3e-5 (profiles/r03_bin_parity.json)
                rep["bin_mismatch_max_abs_dk"] = int(np.abs(k_own[both] - k_or[both]).max())
                rep["bins_compared"] = int(both.sum())
                ok = ok and rate <= (5e-5 if self.f32 else 1e-6) and rep["bin_mismatch_max_abs_dk"] <= 1
        rep["ok"] = bool(ok)
        return rep

    def close(self):
        self.lib.ssq_dev_free(self.d_x)
        if self.own_out:
            self.lib.ssq_dev_free(self.d_out)
        self.lib.ssq_dev_free(self.d_one)
        self.lib.ssq_stft_plan_destroy(self.plan)


def roofline_of(leg, kern_ms, traffic, kernel_name):
    k_avg = float(np.mean(kern_ms))
    alg = leg.B * leg.alg_bytes_per_signal
    achieved = alg / (k_avg * 1e-3) / 1e9
    return {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            # context only: the guide's MEASURED float4-copy rate (6.29 TB/s = 79 % of the 8 TB/s spec `frac` is priced against)
            "frac_of_measured_copy_rate": achieved / HBM_MEASURED_COPY_GBS,
            "traffic": traffic,
            "traffic_source": TRAFFIC_FILE if traffic is not None else None,
            "kernel": kernel_name, "kernel_ms_avg": k_avg, "kernel_ms_min": float(np.min(kern_ms)),
            # which dispatches of the interior-tile kernel were the timed ones (0-based, in launch order): a kernel trace
            # of this command restricted to them is what `kernel_ms_avg` must agree with (tools/trace_timed.py)
            "timed_dispatches": None if leg.timed_first is None else [leg.timed_first, leg.timed_first + len(kern_ms)],
            "kernel_ms_all": [round(float(v), 4) for v in kern_ms],
            "alg_bytes_per_launch": alg}


DUMP_LIMIT_BYTES = 64 << 20       # --dump-outputs: everything written, headers included
DUMP_SAMPLE_BINS = 1 << 19         # single bins sampled over the whole batch (value + index: 16 bytes each)


def dump_plan(B, n_freqs, n_frames, seed=0):
    """What --dump-outputs takes of a [B, n_freqs, n_frames] Tx: (whole signals, sorted flat bin indices).
    Signals 0, B/2, B-1 as many as fit beside the sample; the sample depends on the shape and the seed only."""
    total = B * n_freqs * n_frames
    flat = np.sort(np.random.default_rng(seed).choice(total, size=min(total, DUMP_SAMPLE_BINS), replace=False))
    room = DUMP_LIMIT_BYTES - 16 * flat.size - 4 * 4096            # 4 KiB per .npy header, generously
    whole = sorted({0, B // 2, B - 1})[: max(0, room // (n_freqs * n_frames * 2 * 4))]
    return whole, flat


def dump_outputs(out_dir, out_t, leg):
    """Write the Tx of the last step (fp32 `out_t`, [B, n_freqs, n_frames] complex) as float32 (..., 2) arrays, and
    the positions they were taken from as float64."""
    import torch
    whole, flat = dump_plan(leg.B, leg.n_freqs, leg.n_frames)
    tx = out_t.view(leg.B, leg.n_freqs, leg.n_frames, 2)
    arrays = {"Tx_sample": out_t.view(-1, 2)[torch.from_numpy(flat).to(out_t.device)].cpu().numpy(),
              "Tx_sample_index": flat.astype(np.float64)}
    if whole:
        arrays["Tx_signals"] = tx[whole].cpu().numpy()
        arrays["Tx_signals_index"] = np.asarray(whole, dtype=np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {name: list(a.shape) for name, a in arrays.items()}


FP_PEAK_TFLOPS = {"f32": 157.3, "f64": 78.6}            # MI355X_MICROARCH.md: vector fp32 / fp64


def cwt_leg(lib, _lib, f32, log2n, batch, steps, golden, cpu, traffic_files=(), label=""):
    """ssq_cwt (Morlet, 256 log scales 2**linspace(1, log2n - 1, 256)) through the plan API on `batch` signals of 2^log2n
    samples: ms per call, bins/s, BOTH rooflines (algorithmic bytes against HBM, the transforms' flops against the vector
    roof), the measured traffic of the committed PMC passes if present, and a check of signal 0 of what was timed against
    the committed oracle summary (block sums of the column sums -- invariant under bin flips --, row energies, the norm:
    the quantities tests/test_gpu_cwt_full.py checks)."""
    import ctypes as C
    from ssqueeze_rs_amd.synth import synth_signal
    N, na = 1 << log2n, 256
    es = 4 if f32 else 8
    rdt, cdt = (np.float32, np.complex64) if f32 else (np.float64, np.complex128)
    scales = 2.0 ** np.linspace(1, log2n - 1, na)
    plan, dx, dT, ws = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    _lib.check(lib.ssq_cwt_plan_create(C.byref(plan), _lib.SSQ_F32 if f32 else _lib.SSQ_F64, N, _lib.WAVELET["morlet"],
                                       scales.ctypes.data_as(C.c_void_p), na, 1.0, 0))
    wsb = lib.ssq_cwt_plan_workspace_bytes(plan, batch)
    plane = na * N * 2 * es
    try:
        _lib.check(lib.ssq_dev_malloc(C.byref(dx), batch * N * es))
        _lib.check(lib.ssq_dev_malloc(C.byref(dT), batch * plane))
        _lib.check(lib.ssq_dev_malloc(C.byref(ws), wsb))
        x = np.concatenate([synth_signal(N, b, rdt) for b in range(batch)])
        _lib.check(lib.ssq_memcpy_h2d(dx, x.ctypes.data_as(C.c_void_p), x.nbytes, None))

        def run():
            _lib.check(lib.ssq_cwt_plan_exec_ssq(plan, dx, batch, 0, 0, 0, 1, -1.0, dT, None, None, None, ws, wsb, None))
            _lib.check(lib.ssq_device_sync())

        run()
        check = {"validated": None}
        gpath = os.path.join(ROOT, "tests", "golden", golden) if golden else None
        if gpath and os.path.exists(gpath):
            g = np.load(gpath)
            nb = g["block_col_sums"].shape[0]
            col = np.zeros(N, dtype=np.complex128)
            row = np.zeros(na, dtype=np.float64)
            sq = 0.0
            rows_per = max(1, (1 << 30) // (N * 2 * es))           # <= 1 GiB of host memory per piece (C5: 17 GB per signal)
            for r0 in range(0, na, rows_per):
                r1 = min(na, r0 + rows_per)
                part = np.empty((r1 - r0, N), dtype=cdt)
                _lib.check(lib.ssq_memcpy_d2h(part.ctypes.data_as(C.c_void_p), C.c_void_p(dT.value + r0 * N * 2 * es),
                                              part.nbytes, None))
                _lib.check(lib.ssq_device_sync())
                col += part.sum(0, dtype=np.complex128)
                row[r0:r1] = np.abs(part).sum(1, dtype=np.float64)
                sq += float((part.real.astype(np.float64) ** 2).sum() + (part.imag.astype(np.float64) ** 2).sum())
                del part
            blk = col.reshape(nb, N // nb).sum(1)
            e_blk = float(np.abs(blk - g["block_col_sums"]).max() / np.abs(g["block_col_sums"]).max())
            e_row = float(np.abs(row - g["row_energy"]).max() / g["row_energy"].max())
            e_nrm = abs(float(np.sqrt(sq)) - float(g["norm2"])) / float(g["norm2"])
            tol = (2e-4, 1e-3, 1e-4) if f32 else (1e-9, 1e-6, 1e-7)
            check = {"validated": bool(e_blk <= tol[0] and e_row <= tol[1] and e_nrm <= tol[2]),
                     "validation": {"signal": 0, "block_colsum_relerr": e_blk, "row_energy_relerr": e_row,
                                    "norm_relerr": e_nrm, "golden": "tests/golden/" + golden}}
        t0 = time.perf_counter()
        for _ in range(steps):
            run()
        dt = (time.perf_counter() - t0) / steps
    finally:
        for ptr in (dx, dT, ws):
            if ptr:
                lib.ssq_dev_free(ptr)
        lib.ssq_cwt_plan_destroy(plan)
    alg = batch * (es * N + 2 * es * na * N)                       # x in once, Tx out once
    P = 1 << int(np.ceil(np.log2(N + N // 2)))
    flops = batch * (1 + 2 * na) * 5.0 * P * np.log2(P)            # (1 + 2 na) transforms of length P
    out = {"workload": f"ssq_cwt morlet, 256 log scales, {batch} x 2^{log2n}, {'fp32' if f32 else 'fp64'}" + label,
           "ms_per_call": dt * 1e3, **check,
           "value": batch * na * N / dt, "unit": "TF-bins/s", "roofline_frac": alg / dt / 1e9 / HBM_PEAK_GBS,
           "roofline_vector": {"bound": "valu", "achieved": flops / dt / 1e12, "unit": "TFLOP/s",
                               "peak": FP_PEAK_TFLOPS["f32" if f32 else "f64"],
                               "frac": flops / dt / 1e12 / FP_PEAK_TFLOPS["f32" if f32 else "f64"]},
           "device_footprint_GB": (batch * plane + wsb + batch * N * es) / 1e9, "workspace_GB": wsb / 1e9}
    for name in traffic_files:
        tf = os.path.join(ROOT, "profiles", name)
        if os.path.exists(tf):
            with open(tf) as fh:
                out["traffic_over_algorithmic"] = json.load(fh)["total_GB_per_call"] * 1e9 / (alg / batch)
            out["traffic_source"] = "profiles/" + name
            break
    if cpu:
        out["cpu_baseline"] = cwt_cpu_baseline(N, scales)
    return out


def cwt_cpu_baseline(N, scales):
    """The oracle's C restatement of ssq_cwt.rs (oracle/ssq_ref.c::ssq_ref_ssq_cwt: forward FFT, per scale two inverse
    FFTs over OpenMP threads, phase transform, column-parallel reassignment), timed on this box's host cores on C4."""
    from oracle import ref_c                         # the timed CPU baseline (kind "port")
    from ssqueeze_rs_amd.synth import synth_signal
    x = synth_signal(N, 0, np.float64)
    t0 = time.perf_counter()
    ref_c.ssq_cwt(x, scales, wavelet="morlet")
    t = time.perf_counter() - t0
    return {"value": len(scales) * N / t, "unit": "TF-bins/s", "cores": ref_c.num_threads(), "kind": "port",
            "sample": f"the whole C4 call once (1 x 2^20, 256 scales, fp64; radix-2 C FFTs built -march=x86-64-v2, "
                      f"OpenMP over scales / columns), {t:.1f} s"}


def main():
    args = parse_args()
    plan = launch_plan(args.gpus)
    if plan[0] == "error":
        print("bench.py: " + plan[1], file=sys.stderr)
        sys.exit(2)
    if plan[0] == "spawn":
        sys.exit(spawn_ranks(plan[1], sys.argv[1:]))
    _, world, rank, local_rank = plan

    # Native libraries (RCCL prints a version banner on its first collective) write to file descriptor 1: park the
    # real stdout and point fd 1 at stderr, so that the ONE JSON line is the only thing this process puts on stdout.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    # torch first: libssq_hip.so then binds to the HIP runtime torch already loaded
    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    torch.cuda.set_device(local_rank)
    use_dist = world > 1 or "RANK" in os.environ
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))   # "nccl" is RCCL on ROCm
        assert dist.get_world_size() == world

    from ssqueeze_rs_amd import _lib
    lib = _lib.load()
    _lib.check(lib.ssq_set_device(local_rank))

    N = 1 << args.log2n
    n_fft, hop = args.n_fft, args.hop
    B, first, total, scaling = job_shape(world, rank, args.batch, args.total_batch)
    if B <= 0:
        raise SystemExit("bench.py: a rank got no signal (total batch smaller than the world size)")

    stream = C.c_void_p()
    _lib.check(lib.ssq_stream_create(C.byref(stream)))
    bins = (n_fft // 2 + 1) * ((N - 1) // hop + 1)
    # Tx lives in a torch allocation so that the optional gather hands RCCL the real result buffer
    out_t = torch.empty(B * bins * 2, dtype=torch.float32, device="cuda")
    leg = Leg(lib, _lib, np.float32, N, n_fft, hop, B, stream, d_out_ptr=out_t.data_ptr())
    nd = B if args.distinct <= 0 else min(args.distinct, B)
    leg.upload(synth_rows(first, nd, N, np.float32))          # global signal index = seed offset

    def fence():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    # --full: check what is about to be timed (outside the timed region, and before it: the check's own launches and
    # copies also bring the device out of its idle clocks before the W warm-up steps).
    validation = None
    if args.full and not args.no_validate:
        validation = leg.validate(first)
        if use_dist:
            okt = torch.tensor([1 if validation["ok"] else 0], device="cuda", dtype=torch.int32)
            dist.all_reduce(okt, op=dist.ReduceOp.MIN)
            validation["ok_all_ranks"] = bool(okt.item())

    wall, kern_ms = leg.timed(args.steps, args.warmup, before=fence, after=torch.cuda.synchronize,
                              settle_ms=args.settle_ms)
    if use_dist:
        dist.barrier()
        tt = torch.tensor([wall], device="cuda", dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        wall = float(tt.item())
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, out_t, leg)

    # Secondary legs (--full, N = 1 only) run AFTER the headline's timed region (round 2 ran them before it, which
    # lengthened the undisclosed warm-up): the only load in front of the K timed steps is the disclosed run-in
    # (settle_ms) + W steps.
    sec = None
    if args.full and rank == 0 and world == 1 and not args.no_secondary:
        sec = {}
        # (1) BASELINE config 2: ONE signal (latency-bound: one launch of the edge-capable kernel)
        one = Leg(lib, _lib, np.float32, N, n_fft, hop, 1, stream)
        one.upload(synth_rows(0, 1, N, np.float32))
        _, k1 = one.timed(50, 5)
        sec["c2_one_signal_f32"] = {"ms_per_step": float(np.mean(k1)), "value": one.bins / (float(np.mean(k1)) * 1e-3),
                                    "unit": "TF-bins/s",
                                    "roofline_frac": one.alg_bytes_per_signal / (float(np.mean(k1)) * 1e-3) / 1e9 / HBM_PEAK_GBS}
        # the same call captured 20x into one HIP graph (ssq_graph_*): what a launch-bound caller replays per signal
        try:
            g, a, b_ = C.c_void_p(), C.c_void_p(), C.c_void_p()
            _lib.check(lib.ssq_graph_capture_begin(stream))
            for _ in range(20):
                one.step()
            _lib.check(lib.ssq_graph_capture_end(stream, C.byref(g)))
            _lib.check(lib.ssq_event_create(C.byref(a)))
            _lib.check(lib.ssq_event_create(C.byref(b_)))
            _lib.check(lib.ssq_graph_launch(g, stream))
            _lib.check(lib.ssq_event_record(a, stream))
            for _ in range(5):
                _lib.check(lib.ssq_graph_launch(g, stream))
            _lib.check(lib.ssq_event_record(b_, stream))
            _lib.check(lib.ssq_stream_sync(stream))
            ms = C.c_float(0)
            _lib.check(lib.ssq_event_elapsed_ms(a, b_, C.byref(ms)))
            sec["c2_one_signal_f32"]["ms_per_step_graph_replay"] = ms.value / 100.0
            for h in (a, b_):
                lib.ssq_event_destroy(h)
            lib.ssq_graph_destroy(g)
        except Exception as e:
            sec["c2_one_signal_f32"]["graph_replay_error"] = str(e)
        one.close()
        # (2) the reference's own arithmetic: fp64 in, complex128 out, same workload
        l64 = Leg(lib, _lib, np.float64, N, n_fft, hop, B, stream)
        nd64 = min(nd, 16)
        l64.upload(synth_rows(first, nd64, N, np.float64))
        v64 = l64.validate(first) if not args.no_validate else None
        _, k64 = l64.timed(max(3, args.steps // 2), 2)
        r64 = roofline_of(l64, k64, measured_traffic(B, int(np.log2(N)), n_fft, hop, TRAFFIC_FILE_F64),
                          "stft_fused_kernel<double,10,true,false,false> (8 waves; + edge-tile launch)")
        if r64.get("traffic") is not None:
            r64["traffic_source"] = TRAFFIC_FILE_F64
        sec["f64"] = {"dtype": "f64", "batch": B, "data": f"seeds {first}..{first + nd64 - 1} tiled to the batch",
                      "ms_per_step": float(np.mean(k64)),
                      "value": B * l64.bins / (float(np.mean(k64)) * 1e-3), "unit": "TF-bins/s",
                      "roofline": r64, "validated": None if v64 is None else v64["ok"]}
        l64.close()
        # (3) BASELINE config 4: ssq_cwt, 1 x 2^20, 256 log scales, Morlet, fp32 (wall clock around synchronised calls)
        try:
            sec["c4_ssq_cwt_f32"] = cwt_leg(lib, _lib, True, 20, 1, 5, "c4_summary.npz", not args.no_cpu_baseline,
                                             ("r03_cwt_traffic.json", "r02_cwt_traffic.json"))
        except Exception as e:                                    # a secondary leg must not take the headline down
            sec["c4_ssq_cwt_f32"] = {"error": str(e)}
        # (4) BASELINE config 5 in the reference's own arithmetic: ONE fp64 signal of 2^22 samples (its 17.2 GB of Tx
        #     checked against the committed oracle summary), then C5's per-GPU share -- 8 signals, 137 GB of Tx plus the
        #     plan's scratch resident at once -- run once to prove the footprint DESIGN.md section 3 claims
        if not args.no_c5:
            for key, nb, st, gold, lab in (("c5_one_signal_f64", 1, 2, "c5_summary.npz", ""),
                                           ("c5_share_8_signals_f64", 8, 1, "c5_summary.npz",
                                            " (BASELINE config 5's share of one of 8 GPUs)")):
                try:
                    sec[key] = cwt_leg(lib, _lib, False, 22, nb, st, gold, False, ("r03_cwt_traffic_f64.json",), lab)
                except Exception as e:
                    sec[key] = {"error": str(e)}

    gather = None
    if args.gather and use_dist:
        # optional final gather of the Tx shards over xGMI (RCCL all_gather of the REAL result buffer; equal shard
        # sizes are required by all_gather_into_tensor, so the strong mode gathers the common minimum per rank)
        cnt = torch.tensor([B], device="cuda", dtype=torch.int64)
        dist.all_reduce(cnt, op=dist.ReduceOp.MIN)
        nshare = int(cnt.item())
        shard = out_t[: nshare * bins * 2]
        outl = torch.empty(world * shard.numel(), device="cuda", dtype=torch.float32)
        # the gather itself goes through the C-ABI (ssq_gather_shards: RCCL dlopen'd by the library, no torch on the data
        # path); torch.distributed only carries the 128-byte RCCL id from rank 0 to the others
        idb = C.create_string_buffer(128)
        if rank == 0:
            _lib.check(lib.ssq_rccl_unique_id(idb))
        box = [bytes(idb.raw)]
        dist.broadcast_object_list(box, src=0)
        idb = C.create_string_buffer(box[0], 128)
        comm = C.c_void_p()
        _lib.check(lib.ssq_rccl_comm_init(C.byref(comm), world, idb, rank))
        nbytes = int(shard.numel() * 4)

        def do_gather():
            _lib.check(lib.ssq_gather_shards(comm, C.c_void_p(shard.data_ptr()), C.c_void_p(outl.data_ptr()), nbytes, stream))
            _lib.check(lib.ssq_stream_sync(stream))

        do_gather()
        dist.barrier()
        g0 = time.perf_counter()
        do_gather()
        g_ms = (time.perf_counter() - g0) * 1e3
        mine = outl[rank * shard.numel(): (rank + 1) * shard.numel()]
        n_seen, me = C.c_int(0), C.c_int(0)
        _lib.check(lib.ssq_rccl_comm_info(comm, C.byref(n_seen), C.byref(me)))
        heads = outl.view(world, -1)[:, :2].clone()         # every rank's first value arrived where its rank says
        gather = {"ms": g_ms, "bytes_per_rank": nbytes, "signals_per_rank": nshare, "via": "ssq_gather_shards (C-ABI, RCCL)",
                  "own_shard_round_trip_equal": bool(torch.equal(mine, shard)),
                  "ranks_seen_by_rccl": int(n_seen.value), "my_rccl_rank": int(me.value),
                  "shards_nonzero": bool((heads.abs().sum(1) > 0).all().item())}
        lib.ssq_rccl_comm_destroy(comm)
        del outl

    if rank == 0:
        ms_per_step = wall / args.steps * 1e3
        value = total * bins * args.steps / wall
        cu = C.c_int(0)
        name = C.create_string_buffer(128)
        lib.ssq_device_info(C.byref(cu), None, name, 128)
        line = {
            "metric": "TF-bins/sec (ssq_stft, n_fft=1024)",
            "value": value, "unit": "TF-bins/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "settle_ms": args.settle_ms, "higher_is_better": True, "scaling": scaling,
            "vs_baseline": None,
            "dtype": "f32",
            "data": f"synthetic multi-sine+chirp+noise, seeds {first}..{first + nd - 1}"
                    + ("" if nd == B else f" tiled to the batch of {B}"),
            "config": {"workload": f"ssq_stft batch={B}/GPU ({total} in the job) x 2^{args.log2n} samples, n_fft={n_fft} "
                                   f"hop={hop} Hann, fs=1, reflect, sum; inputs and Tx resident in HBM",
                       "batch_per_gpu": B, "total_batch": total, "n_signal": N, "n_fft": n_fft, "hop": hop,
                       "n_freqs": leg.n_freqs, "n_frames": leg.n_frames, "parallelism": f"batch-sharded x{world}"},
            "roofline": roofline_of(leg, kern_ms, measured_traffic(B, args.log2n, n_fft, hop),
                                    "stft_tx1024_kernel<false,false,16> (interior tiles; the edge-tile launch of the "
                                    "same pass is inside the timed events)"),
            "device": name.value.decode(), "cu_count": cu.value,
        }
        if validation is not None:
            line["validated"] = bool(validation.get("ok_all_ranks", validation["ok"]))
            line["validation"] = validation
        if gather is not None:
            line["gather"] = gather
        if dumped is not None:
            line["dumped_outputs"] = {"dir": args.dump_outputs, "shapes": dumped}
        if sec is not None:
            line["secondary"] = sec
    ok = validation is None or validation.get("ok_all_ranks", validation["ok"])

    if rank == 0:
        if args.full and not args.no_cpu_baseline and world == 1:
            line["cpu_baseline"] = cpu_baseline(N, n_fft, hop)
        sys.stdout.flush()
        os.write(real_stdout, (json.dumps(line) + "\n").encode())

    if leg is not None:
        leg.close()
    lib.ssq_stream_destroy(stream)
    if use_dist:
        dist.destroy_process_group()
    if not ok:
        sys.exit(3)


if __name__ == "__main__":
    main()
