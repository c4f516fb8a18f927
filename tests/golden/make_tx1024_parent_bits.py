"""Record tests/golden/tx1024_parent_bits.npz for tests/test_gpu_tx1024_readout.py (needs the GPU).

    python tests/golden/make_tx1024_parent_bits.py COMMIT [OUT.npz]

Run it on a checkout of the commit whose bits are to be kept -- the parent of the read-out rework of
`stft_tx1024_kernel` -- with that commit's library built; COMMIT is stored in the file as `parent_commit`.
The cases, shapes and inputs are the test module's own (`CASES`, `run_case`), so generator and test cannot drift.
Per case: the batch size, a CRC32 of every input signal and of every signal's output bytes, and in full row 512 and
the first and last frame column of the signals in FULL_SIGNALS (row 512 only for the (w, k) hook).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import test_gpu_tx1024_readout as t  # noqa: E402


def main():
    commit = sys.argv[1]
    dst = sys.argv[2] if len(sys.argv) > 2 else t.GOLDEN
    z = {"parent_commit": np.array(commit)}
    for case in t.CASES:
        x, out, again = t.run_case(case)
        assert np.array_equal(out.view(np.uint32), again.view(np.uint32)), case
        full = [b for b in t.FULL_SIGNALS if b < x.shape[0]]
        z[f"{case}_B"] = np.array(x.shape[0])
        z[f"{case}_xcrc"] = t.crc_per_signal(x)
        z[f"{case}_crc"] = t.crc_per_signal(out)
        z[f"{case}_row512"] = np.stack([out[b, 512] for b in full])
        if case != "wk":
            z[f"{case}_col_first"] = np.stack([out[b, :, 0] for b in full])
            z[f"{case}_col_last"] = np.stack([out[b, :, -1] for b in full])
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    np.savez_compressed(dst, **z)
    print(f"wrote {dst}: {os.path.getsize(dst)} bytes, parent_commit {commit}")


if __name__ == "__main__":
    main()
