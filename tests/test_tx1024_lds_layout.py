"""The LDS image of the fp32 n_fft = 1024 Tx kernel (csrc/tx1024_lds_layout.h), checked on the host by the stand-alone
program tests/helpers/tx1024_lds_layout_check.cpp, which indexes with the very functions the kernel uses: one slot per
table entry, aligned 16-byte reads that return the consumed pair in order, the exchange-1 permutation, bank-conflict
degrees under the LDS lane-group rules, and the 160 KiB total.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helpers", "tx1024_lds_layout_check.cpp")
# the conflict degrees DESIGN.md section 4.1 records for the layout: 1 = no two addresses of a lane group share a bank
DEGREES = {"window": 1, "tw1": 1, "tw2": 1, "exch_store": 1, "exch_load": 1}


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tx1024_lds") / "layout_check")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-fno-omit-frame-pointer"]
    r = subprocess.run(base + san + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    if r.returncode != 0 and "cannot find" in (r.stderr or "") and ("asan" in r.stderr or "ubsan" in r.stderr):
        # no static sanitizer runtimes here: the program's own checks (bounds included) still run
        r = subprocess.run(base + [SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return r.stdout.split("\n")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_tables_and_exchange_hold(report):
    """Slots, alignment, consumed pairs and the exchange permutation: the program's CHECKs, all of them."""
    assert report[-2:] == ["ok", ""], report


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_bank_conflict_degrees(report):
    got = {ln.split()[1]: int(ln.split()[2]) for ln in report if ln.startswith("degree ")}
    assert got == DEGREES


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_lds_total_within_160_kib(report):
    total = [int(ln.split()[1]) for ln in report if ln.startswith("lds_bytes ")]
    assert len(total) == 1 and 0 < total[0] <= 160 * 1024
    # and it is the size the kernel's own struct asserts against (Hi1024::LDS_BYTES == tx1024::LDS_BYTES)
    src = open(os.path.join(ROOT, "ssqueeze_rs_amd", "csrc", "stft_fused.hip")).read()
    assert "LDS_BYTES == tx1024::LDS_BYTES" in src
