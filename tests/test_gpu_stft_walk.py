"""GPU tests of the fused STFT kernels' PERSISTENT TILE WALK: batches big enough that every block processes several
tiles, so `advance()` (with its step across signals), the sample prefetch ring (two deep; one deep for fp64 n_fft = 1024),
the read-out that re-zeroes the tile for the next one and the reuse of `col_scale[]` all run -- for
`stft_fused_kernel` in every family (power of two fp32 / fp64, SPLIT, mixed radix, Bluestein; Tx sum and Lebesgue, Sx,
dSx, (w, k)) and for the Lebesgue instantiation of `stft_tx1024_kernel`.

Every case asserts its own regime from `ssq_stft_plan_launch_info` (total_tiles >= 2 max_blocks + 1, not a multiple of
the grid) and sizes the batch from that query, so a change of F, W or blocks per CU cannot quietly turn it back into a
one-tile-per-block test.  Two regimes:
  short: many signals of 4 tiles (ragged last tile, N no multiple of the tile span): tiles_per_signal < grid, one
         `advance()` skips many signals;
  long : two signals of max_blocks + 3 tiles: tiles_per_signal > grid.
Both are small enough that a pass is ONE launch of the edge-capable instantiation (EDGE = true: the loader with index
mirroring).  A third regime covers what bench.py runs, the SPLIT pass of the power-of-two kernels:
  split: about 260 signals of 6 tiles, more than 4 grids of tiles, so the pass is the interior launch (EDGE = false
         instantiations, direct loads in the prefetch ring) followed by the edge launch (the ta0 / ta_n / tb0 tile map);
         asserted per launch from `ssq_stft_plan_launch_list`: two launches, each with >= 2 blocks + 1 tiles.
The any-length modes (mixed radix, Bluestein) only have the edge-capable instantiation, one launch always.
Reference = the same kernels in the one-tile-per-block regime (total_tiles <= max_blocks, asserted from the query), which
tests/test_gpu_stft.py checks against the oracle at these n_fft; the large run must equal it BITWISE (fixed-point tile:
order-exact).  Short regime: the same signals in sub-batches.  Long regime: one signal alone already has more tiles than
blocks, so the reference runs overlapping SEGMENTS of the signal (start a multiple of hop) as a batch of short signals;
a column whose frame lies inside the segment (or touches only the end of the signal the segment shares) reads the very
same samples, hence the same bits.  Two signals of each large batch also go through `_check_ssq_f32/_f64` against the
float64 oracle (the drop-in call, bitwise equal to the batch's), and each large batch runs twice.
"""
import numpy as np
import pytest

from oracle import ssq_oracle as o
from ssqueeze_rs_amd import _lib, _rs
from ssqueeze_rs_amd.batch import SsqStftBatch
from tests.helpers.scatter_model import bound as scatter_bound, frames_covering
from tests.test_gpu_stft import _check_ssq_f32, _check_ssq_f64

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
# (id, dtype, n_fft, hop, squeezing)
FAMILIES = [
    ("f32-64", F32, 64, 16, "sum"),
    ("f32-256", F32, 256, 64, "sum"),
    ("f32-4096", F32, 4096, 1024, "sum"),
    ("f32-1024-lebesgue", F32, 1024, 256, "lebesgue"),        # stft_tx1024_kernel<.., LEB = true>
    ("f64-64", F64, 64, 16, "sum"),
    ("f64-512", F64, 512, 128, "sum"),
    ("f64-1024", F64, 1024, 256, "sum"),                      # SPLIT: one-deep prefetch
    ("f64-2048", F64, 2048, 512, "sum"),
    ("f32-1000", F32, 1000, 250, "sum"),                      # mixed radix
    ("f64-1000", F64, 1000, 250, "sum"),
    ("f64-333", F64, 333, 83, "sum"),                         # Bluestein
]
BY_ID = {f[0]: f for f in FAMILIES}
KINDS = {"tx": _lib.OUT_TX, "sx": _lib.OUT_SX, "dsx": _lib.OUT_DSX, "wk": _lib.OUT_WK}


@pytest.fixture(autouse=True)
def _default_launch_split(monkeypatch):
    monkeypatch.delenv("SSQ_SINGLE_LAUNCH", raising=False)


def _engine(N, n_fft, hop, dtype, squeezing, B):
    return SsqStftBatch(N, np.hanning(n_fft), n_fft, hop, fs=1.0, squeezing=squeezing, dtype=dtype, max_batch=B)


def _grid(n_fft, hop, dtype, squeezing, kind):
    """(F, grid of a launch that has more tiles than blocks) of the kernel that serves `kind`, from the query.
    Only used to SIZE a case: at this batch the pass is split, and the figure is the larger of the two grids.  Each
    case then asserts its regime with the query at its own plan and batch (_assert_walk, _assert_split)."""
    eng = _engine(8 * n_fft, n_fft, hop, dtype, squeezing, 1)
    try:
        F, tiles, blocks = eng.launch_info(1 << 16, kind)
        assert F > 0 and tiles > blocks > 0
        return F, blocks
    finally:
        eng.close()


def _assert_walk(eng, B, kind, tag):
    F, tiles, blocks = eng.launch_info(B, kind)
    print(f"WALK {tag}: tile_frames={F} max_blocks={blocks} total_tiles={tiles} batch={B}")
    assert tiles >= 2 * blocks + 1, (tag, tiles, blocks)       # every block walks >= 2 tiles, some 3
    assert tiles % blocks != 0, (tag, tiles, blocks)
    return F, tiles, blocks


def _signals(N, B, dtype, first):
    return np.stack([o.synth_signal(N, first + b, dtype) for b in range(B)])


def _short_case(fam, kind):
    """(x, engine, B, sub) of the many-short-signals regime: 4 tiles per signal, the last one ragged."""
    _, dtype, n_fft, hop, squeezing = fam
    F, grid = _grid(n_fft, hop, dtype, squeezing, kind)
    n_frames = 3 * F + F // 2 + 1
    N = (n_frames - 1) * hop + 1 + hop // 3
    assert (N - 1) // hop + 1 == n_frames and N % (F * hop) != 0
    tps = -(-n_frames // F)
    assert 3 <= tps <= 5
    B = -(-(2 * grid + 1) // tps)
    while (B * tps) % grid == 0:
        B += 1
    eng = _engine(N, n_fft, hop, dtype, squeezing, B)
    sub = max(1, grid // tps)
    return _signals(N, B, dtype, 100), eng, B, sub


def _run_in_sub_batches(eng, x, sub, kind):
    """The one-tile-per-block reference: asserted from the query, not assumed."""
    out = []
    for b0 in range(0, x.shape[0], sub):
        nb = min(sub, x.shape[0] - b0)
        F, tiles, blocks = eng.launch_info(nb, kind)
        assert tiles <= blocks, (tiles, blocks)
        out.append(eng.run(x[b0:b0 + nb], kind))
    return np.concatenate(out)


def _oracle_check(fam, x1, Tx_batch):
    """One signal of the large batch: the drop-in call gives the batch's bits, and passes the oracle checks."""
    _, dtype, n_fft, hop, squeezing = fam
    win = np.hanning(n_fft)
    one, _ = _rs.ssq_stft(x1, win, n_fft=n_fft, hop_len=hop, fs=1.0, squeezing=squeezing)
    assert np.array_equal(one, Tx_batch)
    if dtype == F32:
        _check_ssq_f32(x1, win, n_fft, hop, 1.0, "reflect", squeezing)
    else:
        _check_ssq_f64(x1, win, n_fft, hop, 1.0, "reflect", squeezing)


@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_many_short_signals_tx(fam):
    x, eng, B, sub = _short_case(fam, _lib.OUT_TX)
    try:
        _assert_walk(eng, B, _lib.OUT_TX, f"{fam[0]} short tx")
        Tx = eng.run(x, _lib.OUT_TX)
        assert np.array_equal(Tx, eng.run(x, _lib.OUT_TX))                      # run to run
        ref = _run_in_sub_batches(eng, x, sub, _lib.OUT_TX)
        bad = [b for b in range(B) if not np.array_equal(Tx[b], ref[b])]
        assert not bad, f"signals {bad[:8]} differ from the one-tile-per-block run"
    finally:
        eng.close()
    for b in (1, B - 1):
        _oracle_check(fam, x[b], Tx[b])


@pytest.mark.parametrize("fid", ["f32-256", "f64-512"])
@pytest.mark.parametrize("kind", ["lebesgue", "sx", "dsx", "wk"])
def test_many_short_signals_other_outputs(fid, kind):
    """One family per dtype through the other instantiations: Lebesgue Tx, Sx, dSx and the Tx epilogue's own (w, k)."""
    fam = BY_ID[fid]
    if kind == "lebesgue":
        fam = fam[:4] + ("lebesgue",)
    out_kind = KINDS.get(kind, _lib.OUT_TX)
    x, eng, B, sub = _short_case(fam, out_kind)
    try:
        _assert_walk(eng, B, out_kind, f"{fid} short {kind}")
        out = eng.run(x, out_kind)
        assert np.array_equal(out, eng.run(x, out_kind), equal_nan=True)
        ref = _run_in_sub_batches(eng, x, sub, out_kind)
        bad = [b for b in range(B) if not np.array_equal(out[b], ref[b], equal_nan=True)]
        assert not bad, f"signals {bad[:8]} differ from the one-tile-per-block run"
    finally:
        eng.close()
    if kind == "lebesgue":
        for b in (1, B - 1):
            _oracle_check(fam, x[b], out[b])


@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_few_long_signals_tx(fam):
    """tiles_per_signal > grid: a block's next tile lies further along the SAME signal (or in the next one)."""
    fid, dtype, n_fft, hop, squeezing = fam
    F, grid = _grid(n_fft, hop, dtype, squeezing, _lib.OUT_TX)
    B = 2
    n_frames = (grid + 2) * F + F // 2 + 1
    N = n_frames * hop                                        # hop | N: segments can be aligned to the end
    assert N % (F * hop) != 0
    x = _signals(N, B, dtype, 200)
    eng = _engine(N, n_fft, hop, dtype, squeezing, B)
    try:
        _, tiles, blocks = _assert_walk(eng, B, _lib.OUT_TX, f"{fid} long tx")
        assert tiles // B > blocks
        Tx = eng.run(x, _lib.OUT_TX)
        assert Tx.shape[2] == n_frames
        assert np.array_equal(Tx, eng.run(x, _lib.OUT_TX))
    finally:
        eng.close()
    # ---- reference: overlapping segments of 4 tiles (at least 2 n_fft samples) as a batch of short signals ----
    Lf = max(4 * F, -(-2 * n_fft // hop) + 4)
    M = Lf * hop
    pad_left = (n_fft - 1) // 2
    lo = -(-pad_left // hop)                                  # first column whose frame starts inside the segment
    hi = (M - (n_fft - pad_left)) // hop                      # last column whose frame ends inside it
    assert hi - lo >= F
    starts = list(range(0, n_frames - Lf, hi - lo + 1)) + [n_frames - Lf]
    segs = np.stack([x[b, j0 * hop:j0 * hop + M] for b in range(B) for j0 in starts])
    seg_eng = _engine(M, n_fft, hop, dtype, squeezing, segs.shape[0])
    try:
        sub = max(1, grid // (-(-Lf // F)))
        ref = _run_in_sub_batches(seg_eng, segs, sub, _lib.OUT_TX)
    finally:
        seg_eng.close()
    covered = np.zeros((B, n_frames), dtype=bool)
    for i, (b, j0) in enumerate((b, j0) for b in range(B) for j0 in starts):
        a = 0 if j0 == 0 else lo                              # the first segment shares the signal's left padding
        z = Lf - 1 if j0 == n_frames - Lf else hi             # the last one its right padding
        assert np.array_equal(Tx[b][:, j0 + a:j0 + z + 1], ref[i][:, a:z + 1]), (fid, b, j0)
        covered[b, j0 + a:j0 + z + 1] = True
    assert covered.all()
    for b in range(B):
        _oracle_check(fam, x[b], Tx[b])


POW2 = [f for f in FAMILIES if f[2] & (f[2] - 1) == 0]


def _assert_split(eng, B, kind, tag):
    """The pass is the interior launch + the edge launch, and in EACH every block walks two tiles or more."""
    launches = eng.launch_list(B, kind)
    F, tiles, blocks = eng.launch_info(B, kind)
    print(f"WALK {tag}: tile_frames={F} launches(edge, tiles, blocks)={launches} batch={B}")
    assert [l[0] for l in launches] == [0, 1], (tag, launches)
    for edge, t, g in launches:
        assert t >= 2 * g + 1 and t % g != 0, (tag, launches)
    assert tiles == sum(l[1] for l in launches) and blocks == max(l[2] for l in launches)    # the summary query
    return launches


@pytest.mark.parametrize("fam", POW2, ids=[f[0] for f in POW2])
def test_split_pass_walks_interior_and_edge_kernels(fam, monkeypatch):
    """The default launch split of a batch of more than 4 grids of tiles -- the path bench.py times."""
    fid, dtype, n_fft, hop, squeezing = fam
    F, grid = _grid(n_fft, hop, dtype, squeezing, _lib.OUT_TX)
    n_frames = 5 * F + F // 2 + 1                             # 6 tiles, the last one ragged
    N = (n_frames - 1) * hop + 1 + hop // 3
    tps = -(-n_frames // F)
    probe = _engine(N, n_fft, hop, dtype, squeezing, 1)
    try:
        B = -(-(4 * grid + 1) // tps)
        while True:                                           # size the batch from the per-launch query
            ls = probe.launch_list(B, _lib.OUT_TX)
            if len(ls) == 2 and all(t >= 2 * g + 1 and t % g != 0 for _, t, g in ls):
                break
            B += 1
            assert B <= 4 * grid, "no batch puts two tiles per block on both launches"
    finally:
        probe.close()
    x = _signals(N, B, dtype, 300)
    eng = _engine(N, n_fft, hop, dtype, squeezing, B)
    try:
        _assert_split(eng, B, _lib.OUT_TX, f"{fid} split tx")
        Tx = eng.run(x, _lib.OUT_TX)
        assert np.array_equal(Tx, eng.run(x, _lib.OUT_TX))
        ref = _run_in_sub_batches(eng, x, max(1, grid // tps), _lib.OUT_TX)
        bad = [b for b in range(B) if not np.array_equal(Tx[b], ref[b])]
        assert not bad, f"signals {bad[:8]} differ from the one-tile-per-block run"
        monkeypatch.setenv("SSQ_SINGLE_LAUNCH", "1")          # the same batch as one edge-capable launch: same bits
        assert len(eng.launch_list(B, _lib.OUT_TX)) == 1
        assert np.array_equal(Tx, eng.run(x, _lib.OUT_TX))
    finally:
        eng.close()
    monkeypatch.delenv("SSQ_SINGLE_LAUNCH")
    for b in (0, B - 1):
        _oracle_check(fam, x[b], Tx[b])


NAN_CASES = [("f32-256", "sum"), ("f64-512", "sum"), ("f64-1024", "sum"), ("f32-1024-lebesgue", "lebesgue"),
             ("f32-256", "lebesgue"), ("f64-512", "lebesgue")]


@pytest.mark.parametrize("fid,squeezing", NAN_CASES, ids=[f"{a}-{b}" for a, b in NAN_CASES])
def test_nan_in_a_middle_tile_stays_in_its_columns(fid, squeezing):
    """One NaN sample in the second tile of one signal of the first grid wave: its block goes on to tiles of other
    signals, the signal's other tiles sit on other blocks.  Stale col_scale[] or tile cells carried into a block's next
    tile would show in another signal, or in a column of this one whose frame does not read the sample.
    The columns that do read it follow the reference (ssq_stft.rs:278-298: a NaN bin is kept, its scan leaves k = 0):
    sum mode adds NaN to row 0; Lebesgue adds 1/n_freqs * dw per bin to row 0 -- n_freqs NaN bins: dw -- and nothing
    elsewhere (the fp32 Lebesgue kernels used to drop these bins: this is the input that showed it)."""
    fam = BY_ID[fid][:4] + (squeezing,)
    _, dtype, n_fft, hop, _ = fam
    x, eng, B, sub = _short_case(fam, _lib.OUT_TX)
    try:
        F, tiles, blocks = _assert_walk(eng, B, _lib.OUT_TX, f"{fid} {squeezing} short nan")
        clean = eng.run(x, _lib.OUT_TX)
        assert np.isfinite(clean.view(dtype)).all()
        victim = 5
        assert (victim + 1) * (tiles // B) <= blocks          # first wave: the blocks that see the NaN have later tiles
        sample = (F + F // 2) * hop                            # inside tile 1
        xp = x.copy()
        xp[victim, sample] = np.nan
        out = eng.run(xp, _lib.OUT_TX)
    finally:
        eng.close()
    others = [b for b in range(B) if b != victim]
    assert np.array_equal(out[others], clean[others])
    hit = frames_covering(sample, out.shape[2], n_fft, hop)
    assert F <= np.flatnonzero(hit).min() and np.flatnonzero(hit).max() < 2 * F
    assert np.array_equal(out[victim][:, ~hit], clean[victim][:, ~hit])
    if squeezing == "sum":
        assert np.isnan(out[victim][0, hit].real).all()
    else:
        dw = 0.5 / (n_fft // 2)
        col = out[victim][:, hit].astype(np.complex128)
        assert not col[1:].any()
        assert (np.abs(col[0] - dw) <= scatter_bound(n_fft // 2 + 1, dtype) * dw).all(), col[0]
