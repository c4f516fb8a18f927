"""bench.py without --full: the headline only (no validation, no secondary legs, no CPU baseline), on the same inputs
as before: the rows synth_rows generates on several threads are bitwise the single-threaded ones."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_full_is_off_by_default():
    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--full"]).full is True


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_synth_rows_equal_the_serial_rows(dtype):
    from ssqueeze_rs_amd.synth import synth_signal
    first, count, N = 3, 21, 1 << 12
    got = bench.synth_rows(first, count, N, dtype)
    want = np.stack([synth_signal(N, first + b, dtype) for b in range(count)])
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(tmp_path):
    B, log2n, steps, warmup = 4, 16, 3, 2
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--batch", str(B), "--log2n", str(log2n), "--settle-ms", "0"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == "TF-bins/sec (ssq_stft, n_fft=1024)" and d["unit"] == "TF-bins/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == steps and d["warmup"] == warmup and len(d["roofline"]["kernel_ms_all"]) == steps
    assert d["ms_per_step"] > 0 and d["value"] > 0
    # with no validation step in front, the timed dispatches follow the W warm-up steps directly
    assert d["roofline"]["timed_dispatches"] == [warmup, warmup + steps]
    for key in ("validated", "validation", "secondary", "cpu_baseline", "dumped_outputs"):
        assert key not in d
