"""bench.py --dump-outputs: what the timed path computed in its last step, written as .npy files (float32 Tx as
(..., 2) = (real, imag), float64 positions), under 64 MiB, the same positions from run to run; and --steps is the
number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_plan_is_fixed_and_fits_the_limit():
    B, nf, nt = 256, 513, 4096                       # the headline workload: 4.3 GB of Tx
    whole, flat = bench.dump_plan(B, nf, nt)
    whole2, flat2 = bench.dump_plan(B, nf, nt)
    assert whole == whole2 == [0, 128, 255] and np.array_equal(flat, flat2)
    assert flat.size == bench.DUMP_SAMPLE_BINS and np.all(np.diff(flat) > 0) and flat[-1] < B * nf * nt
    assert len(whole) * nf * nt * 2 * 4 + flat.size * 16 + 4 * 4096 <= bench.DUMP_LIMIT_BYTES
    # a signal larger than the room left: the sample alone
    whole, flat = bench.dump_plan(2, 2049, 8192)
    assert whole == [] and flat.size == bench.DUMP_SAMPLE_BINS
    # a batch smaller than the sample: every bin, once
    whole, flat = bench.dump_plan(1, 9, 7)
    assert whole == [0] and np.array_equal(flat, np.arange(63))


def test_dump_outputs_writes_the_buffer_it_is_given(tmp_path):
    """In a child process: torch loaded into this one would make libssq_hip.so bind torch's own HIP runtime and RCCL
    in every later test (tests/test_gather.py's communicator then fails to initialise)."""
    B, nf, nt = 5, 9, 7
    full = np.random.default_rng(0).standard_normal((B, nf, nt, 2)).astype(np.float32)
    np.save(tmp_path / "full.npy", full)
    code = ("import json, sys, types; sys.path.insert(0, %r); import numpy as np, torch, bench; "
            "out_t = torch.from_numpy(np.load(%r).reshape(-1)); "
            "print(json.dumps(bench.dump_outputs(%r, out_t, types.SimpleNamespace(B=%d, n_freqs=%d, n_frames=%d))))"
            % (ROOT, str(tmp_path / "full.npy"), str(tmp_path / "dump"), B, nf, nt))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    shapes = json.loads(r.stdout.strip().splitlines()[-1])
    got = {n: np.load(tmp_path / "dump" / (n + ".npy")) for n in shapes}
    assert sorted(os.listdir(tmp_path / "dump")) == sorted(n + ".npy" for n in shapes)
    assert {n: list(a.shape) for n, a in got.items()} == shapes
    assert got["Tx_signals"].dtype == got["Tx_sample"].dtype == np.float32
    assert got["Tx_signals_index"].dtype == got["Tx_sample_index"].dtype == np.float64
    assert np.array_equal(got["Tx_signals"], full[got["Tx_signals_index"].astype(np.int64)])
    assert np.array_equal(got["Tx_sample"], full.reshape(-1, 2)[got["Tx_sample_index"].astype(np.int64)])


@pytest.mark.gpu
def test_bench_dump_matches_the_batch_front_end(tmp_path):
    """A small bench run: --steps K timed steps, and the dumped Tx bitwise equal to the same signals through
    ssqueeze_rs_amd.batch (same kernel, same plan parameters)."""
    B, log2n, steps = 4, 16, 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--batch", str(B), "--log2n", str(log2n), "--settle-ms", "0",
                        "--full", "--no-secondary", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == steps and len(d["roofline"]["kernel_ms_all"]) == steps and d["ms_per_step"] > 0
    assert d["validated"] is True
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in d["dumped_outputs"]["shapes"])

    from ssqueeze_rs_amd.batch import SsqStftBatch
    from ssqueeze_rs_amd.synth import synth_signal
    N = 1 << log2n
    x = np.stack([synth_signal(N, b, np.float32) for b in range(B)])
    eng = SsqStftBatch(N, np.hanning(1024), 1024, 256, dtype=np.float32, max_batch=B)
    try:
        Tx = eng.run(x)
    finally:
        eng.close()
    ref = np.stack([Tx.real, Tx.imag], axis=-1)
    idx = np.load(tmp_path / "Tx_signals_index.npy").astype(np.int64)
    assert idx.tolist() == [0, 2, 3]
    assert np.array_equal(np.load(tmp_path / "Tx_signals.npy"), ref[idx])
    flat = np.load(tmp_path / "Tx_sample_index.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "Tx_sample.npy"), ref.reshape(-1, 2)[flat])
