"""GPU test of `stft_tx1024_kernel`'s interior instantiations with their Tx stores left in flight across the tile loop
(csrc/stft_fused.hip): fp32, n_fft 1024, hop 256, Hann, OUT_TX.

Since each interior instantiation has one read-out path and waits for the next tile's samples behind the read-out
(tests/test_tx1024_isa_waits.py), a block starts the next tile's FFT while the stores of the tile before are still
outstanding.  Nothing of theirs is needed again -- the LDS cells were read and re-zeroed before the store was issued --
so the bits must not move.  Checked here on both instantiations:

  paired   : N = 32 768 -> 128 frames, 8 tiles a signal;
  per-frame: N = 33 024 -> 129 frames, 9 tiles a signal, the last ragged.
Tiles 1..6 of a signal are interior at both lengths (tile 7 reads into the reflected right pad).

Batch 80 with SSQ_SINGLE_LAUNCH=0 is the interior launch (480 tiles) followed by the edge launch; on a 256-CU device
224 of the 256 blocks of the interior launch walk a second tile with the first one's stores behind it (its window
multiply and pass 0 come from the loop's end), and every block takes those of its first tile ahead of the loop.  Signals 0, 39 and 79 are compared BITWISE with
the batch-1 call of the same signal, which is one launch of the edge-capable kernel over all tiles -- another
instantiation, whose code this change does not touch.  The batch runs twice into the same device buffer and is compared
again: the second pass overwrites the first one's Tx while nothing is pending.
"""
import numpy as np
import pytest

from oracle import ssq_oracle as o
from ssqueeze_rs_amd.batch import SsqStftBatch

pytestmark = pytest.mark.gpu

N_FFT, HOP, B = 1024, 256, 80
CHECKED = (0, 39, 79)
# case -> (N, frames, tiles per signal, interior tiles per signal)
CASES = {"paired": (32768, 128, 8, 6), "per_frame": (33024, 129, 9, 6)}


def _engine(N, max_batch):
    return SsqStftBatch(N, np.hanning(N_FFT), N_FFT, HOP, fs=1.0, dtype=np.float32, max_batch=max_batch)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("case", list(CASES))
def test_batch_bits_equal_the_single_signal_launch(case, monkeypatch):
    N, frames, tiles, interior = CASES[case]
    x = np.stack([o.synth_signal(N, 900 + b, np.float64) for b in range(B)]).astype(np.float32)

    monkeypatch.delenv("SSQ_SINGLE_LAUNCH", raising=False)
    one = _engine(N, 1)
    try:
        assert one.n_frames == frames
        launches = one.launch_list(1)
        assert [(l[0], l[1]) for l in launches] == [(1, tiles)], launches        # ONE edge-capable launch, all tiles
        ref = {b: one.run(x[b:b + 1])[0] for b in CHECKED}
    finally:
        one.close()

    monkeypatch.setenv("SSQ_SINGLE_LAUNCH", "0")
    eng = _engine(N, B)
    try:
        launches = eng.launch_list(B)
        print(f"TX1024 inflight {case}: launches(edge, tiles, blocks)={launches}")
        assert [l[0] for l in launches] == [0, 1], launches
        assert launches[0][1] == interior * B and launches[1][1] == (tiles - interior) * B, launches
        assert launches[0][1] > launches[0][2], "no block of the interior launch walks a second tile"
        out = eng.run(x)
        again = eng.run(x)
    finally:
        eng.close()

    for b in CHECKED:
        assert np.abs(ref[b]).max() > 0
        assert np.array_equal(_bits(out[b]), _bits(ref[b])), (case, b, "first pass")
        assert np.array_equal(_bits(again[b]), _bits(ref[b])), (case, b, "second pass into the same buffer")
    assert np.array_equal(_bits(out), _bits(again)), "two passes of the same batch differ"
