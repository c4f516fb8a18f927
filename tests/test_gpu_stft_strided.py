"""`ssq_stft_plan_exec_strided` on every kernel route.  `sig_base()` (csrc/stft_kernels.h) places signal s of a strided
batch at x + (s / group) group_stride + (s % group) sig_stride; every STFT kernel reads its samples through it
(`make_frame` of stft_fused_kernel in its three modes, `load_frame` of stft_tx1024_kernel, dft_frames_kernel,
frames_pack_kernel), and this module runs each of them on a layout a friendly caller would not use: an odd channel
pitch, an odd window stride smaller than the window (the windows overlap), a window length that is no multiple of the hop,
a base pointer an odd number of elements into the allocation, 3 groups of 3 windows or more.

Reference: the same windows gathered on the host into a contiguous [n_groups group, n_signal] array and run through
`ssq_stft_plan_exec` ON THE SAME PLAN.  Same kernels, same samples, and the accumulation is fixed-point (fused Tx) or
ordered (everything else): the strided result must equal it BIT FOR BIT, every window, every cell.  Two windows of every
case tie that packed run to the float64 oracle with the bound tests/test_gpu_stft.py already has for the length
(`_check_ssq_f32` / `_check_ssq_f64` where that module or tests/test_gpu_stft_walk.py use them at the length, the
`_relerr` bound of the length's Sx otherwise); no tolerance is introduced here.

Every case prints and asserts its ROUTE from `ssq_stft_plan_route` and its REGIME from `ssq_stft_plan_launch_info` /
`ssq_stft_plan_launch_list`:
  one tile per block  total_tiles <= max_blocks; windows of 3 tiles, the last one ragged; every route.
  walk                total_tiles >= 2 max_blocks + 1, no multiple of the grid; windows of 4 tiles, so one `advance()`
                      of the persistent tile walk steps across windows of a group and across groups, and the sample
                      prefetch runs across that step; each case twice, the two runs bitwise equal.
  split               SSQ_SINGLE_LAUNCH=0: the interior launch (direct loads) and the edge launch, against the same batch
                      under SSQ_SINGLE_LAUNCH=1.
One case runs 7 x 9364 = 65548 windows through the direct-sum kernels, whose launchers slice a batch at 65535 signals.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import ssq_oracle as o
from ssqueeze_rs_amd import _lib, _rs
from ssqueeze_rs_amd.batch import SsqStftBatch
from tests.test_gpu_grid_limits import Door
from tests.test_gpu_stft import _check_ssq_f32, _check_ssq_f64, _relerr
from tests.test_gpu_stft_walk import _assert_walk, _grid

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TX, SX, DSX, WK = _lib.OUT_TX, _lib.OUT_SX, _lib.OUT_DSX, _lib.OUT_WK
KIND_NAMES = {TX: "tx", SX: "sx", DSX: "dsx", WK: "wk"}
UINT = {4: np.uint32, 8: np.uint64}


@pytest.fixture(autouse=True)
def _default_launch_split(monkeypatch):
    monkeypatch.delenv("SSQ_SINGLE_LAUNCH", raising=False)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.real.dtype.itemsize])


def route_of(eng, kind):
    r = C.c_int(-1)
    _lib.check(eng.lib.ssq_stft_plan_route(eng.plan, kind, C.byref(r)))
    return _lib.STFT_ROUTES[r.value]


def _engine(N, n_fft, hop, dtype, squeezing):
    """The plan (held by a one-signal SsqStftBatch: window np.hanning(n_fft), fs = 1, reflect), as `_rs.ssq_stft` builds
    it for the oracle checks."""
    return SsqStftBatch(N, np.hanning(n_fft), n_fft, hop, fs=1.0, squeezing=squeezing, dtype=dtype, max_batch=1)


class Layout:
    """n_groups x group overlapping windows of N samples inside one allocation of exactly the samples they span."""

    def __init__(self, N, hop, n_groups, group, sig_stride=None):
        self.N, self.n_groups, self.group = N, n_groups, group
        self.sig_stride = ((N // 3) | 1) if sig_stride is None else sig_stride
        self.group_stride = ((group - 1) * self.sig_stride + N + 4) | 1
        self.base = 3
        self.size = self.base + (n_groups - 1) * self.group_stride + (group - 1) * self.sig_stride + N
        assert self.sig_stride % 2 == 1 and self.group_stride % 2 == 1 and self.base % 2 == 1
        assert 0 < self.sig_stride < N and N % hop != 0 and n_groups >= 3 and group >= 3

    def starts(self):
        g, s = np.divmod(np.arange(self.n_groups * self.group), self.group)
        return self.base + g * self.group_stride + s * self.sig_stride

    def buffer(self, dtype, seed):
        """One synthetic channel per group (three sines, a chirp, noise), so that overlapping windows are a real signal."""
        buf = np.empty(self.size, dtype=dtype)
        buf[:self.base] = 7.0
        for g in range(self.n_groups):
            a = self.base + g * self.group_stride
            z = min(self.size, a + self.group_stride)
            buf[a:z] = o.synth_signal(z - a, seed + g, dtype)
        return buf

    def gather(self, buf):
        return np.ascontiguousarray(buf[self.starts()[:, None] + np.arange(self.N)[None, :]])


def run_plain(eng, kind, X):
    B = X.shape[0]
    ws = int(eng.lib.ssq_stft_plan_workspace_bytes(eng.plan, B, kind))
    with Door() as d:
        dx, dout, dws = d.buf(X.nbytes, X), d.buf(B * eng.n_freqs * eng.n_frames * np.dtype(eng.cdtype).itemsize), d.buf(ws)
        _lib.check(eng.lib.ssq_stft_plan_exec(eng.plan, kind, dx.p, B, dout.p, dws.p, ws, None))
        _lib.check(eng.lib.ssq_device_sync())
        return dout.get((B, eng.n_freqs, eng.n_frames), eng.cdtype)


def run_strided(eng, kind, buf, lay, repeat=1):
    """`repeat` runs on the same device buffers (a list of results): the guards of all three are checked on leaving."""
    B = lay.n_groups * lay.group
    ws = int(eng.lib.ssq_stft_plan_workspace_bytes(eng.plan, B, kind))
    outs = []
    with Door() as d:
        dx, dout, dws = d.buf(buf.nbytes, buf), d.buf(B * eng.n_freqs * eng.n_frames * np.dtype(eng.cdtype).itemsize), d.buf(ws)
        px = C.c_void_p(dx.p.value + lay.base * buf.dtype.itemsize)
        for _ in range(repeat):
            _lib.check(eng.lib.ssq_stft_plan_exec_strided(eng.plan, kind, px, lay.n_groups, lay.group, lay.group_stride,
                                                          lay.sig_stride, dout.p, dws.p, ws, None))
            _lib.check(eng.lib.ssq_device_sync())
            outs.append(dout.get((B, eng.n_freqs, eng.n_frames), eng.cdtype))
    return outs if repeat > 1 else outs[0]


def assert_windows_equal(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    ok = (_bits(got) == _bits(ref)).reshape(got.shape[0], -1).all(axis=1)
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, "%s: %d of %d windows differ from the packed run, the first %s" % (what, bad.size, ok.size, bad[:8])


# Sx bound each length already has in tests/test_gpu_stft.py: (fp64, fp32)
SX_BOUND = {
    "pow2": (2e-12, 4e-6),               # test_stft_fused_sizes
    "anylen": (1e-11, 6e-6),             # test_stft_bluestein_lengths
    "long": (1e-11, 2e-5),               # test_stft_long_lengths_through_the_batched_device_fft
    "dft": (1e-11, 2e-6),                # test_stft_generic_any_length; fp32: the Sx bound of _check_ssq_f32
}
# (dtype, n_fft) at which tests/test_gpu_stft.py or tests/test_gpu_stft_walk.py run _check_ssq_f32 / _check_ssq_f64
SSQ_CHECKED = {(F32, 64), (F32, 1024), (F32, 4096), (F32, 1000), (F32, 333), (F32, 48),
               (F64, 64), (F64, 1024), (F64, 2048), (F64, 1000), (F64, 333), (F64, 48)}


def oracle_tie(fam, X, outs, windows):
    """Windows `windows` of the packed run against the float64 oracle, by the bounds the length already has."""
    _, route, dtype, n_fft, hop, squeezing, bound = fam[:7]
    win = np.hanning(n_fft)
    for b in windows:
        x1 = X[b]
        if SX in outs:
            Sx_o, _ = o.stft(x1.astype(np.float64), n_fft, hop, win, "reflect")
            err = _relerr(outs[SX][b], Sx_o)
            print(f"STRIDED {fam[0]}: window {b} Sx relerr {err:.3e} (bound {SX_BOUND[bound][dtype == F32]:.0e})")
            assert err <= SX_BOUND[bound][dtype == F32]
        if TX in outs and (dtype, n_fft) in SSQ_CHECKED:
            one, _ = _rs.ssq_stft(x1, win, n_fft=n_fft, hop_len=hop, fs=1.0, squeezing=squeezing)
            assert np.array_equal(_bits(one), _bits(outs[TX][b]))              # the drop-in call gives the batch's bits
            (_check_ssq_f32 if dtype == F32 else _check_ssq_f64)(x1, win, n_fft, hop, 1.0, "reflect", squeezing)


# (id, route of TX, dtype, n_fft, hop, squeezing, Sx bound of the length, out kinds)
ROUTES = [
    ("dft-f32-17", "DFT", F32, 17, 5, "sum", "dft", (TX, SX, DSX, WK)),
    ("dft-f64-17", "DFT", F64, 17, 5, "sum", "dft", (TX, SX, DSX, WK)),
    ("fft-f32-8192", "FFT_BATCHED", F32, 8192, 2048, "sum", "long", (TX, SX)),
    ("fft-f64-8192", "FFT_BATCHED", F64, 8192, 2048, "sum", "long", (TX, SX)),
    ("fft-f64-4097", "FFT_BATCHED", F64, 4097, 1000, "sum", "long", (TX, SX)),
    ("pow2-f32-64", "FUSED_POW2", F32, 64, 16, "sum", "pow2", (TX, SX, DSX, WK)),
    ("pow2-f32-64-lebesgue", "FUSED_POW2", F32, 64, 16, "lebesgue", "pow2", (TX,)),
    ("pow2-f64-64", "FUSED_POW2", F64, 64, 16, "sum", "pow2", (TX, SX, DSX, WK)),
    ("pow2-f64-64-lebesgue", "FUSED_POW2", F64, 64, 16, "lebesgue", "pow2", (TX,)),
    ("pow2-f32-2048", "FUSED_POW2", F32, 2048, 512, "sum", "pow2", (TX, SX)),
    ("pow2-f64-2048", "FUSED_POW2", F64, 2048, 512, "sum", "pow2", (TX, SX)),
    ("pow2-f32-4096", "FUSED_POW2", F32, 4096, 1024, "sum", "pow2", (TX, SX)),
    ("split-f64-1024", "FUSED_SPLIT", F64, 1024, 256, "sum", "pow2", (TX, SX)),
    ("tx1024-f32", "TX1024", F32, 1024, 256, "sum", "pow2", (TX, WK)),
    ("tx1024-f32-lebesgue", "TX1024", F32, 1024, 256, "lebesgue", "pow2", (TX,)),
    ("mixed-f32-48", "MIXED_RADIX", F32, 48, 12, "sum", "anylen", (TX, SX, WK)),
    ("mixed-f64-48", "MIXED_RADIX", F64, 48, 12, "sum", "anylen", (TX, SX, WK)),
    ("mixed-f32-1000", "MIXED_RADIX", F32, 1000, 250, "sum", "anylen", (TX, SX, WK)),
    ("mixed-f64-1000", "MIXED_RADIX", F64, 1000, 250, "sum", "anylen", (TX, SX, WK)),
    ("blue-f32-333", "BLUESTEIN", F32, 333, 83, "sum", "anylen", (TX, SX, WK)),
    ("blue-f64-333", "BLUESTEIN", F64, 333, 83, "sum", "anylen", (TX, SX, WK)),
]
BY_ID = {f[0]: f for f in ROUTES}


def _window_len(n_frames, hop):
    N = (n_frames - 1) * hop + 1 + hop // 3
    assert (N - 1) // hop + 1 == n_frames and N % hop != 0
    return N


def _tile_frames(n_fft, hop, dtype, squeezing, kind):
    eng = _engine(4 * n_fft, n_fft, hop, dtype, squeezing)
    try:
        return eng.launch_info(1, kind)[0]
    finally:
        eng.close()


# ============================================================================================ one tile per block =======
@pytest.mark.parametrize("fam", ROUTES, ids=[f[0] for f in ROUTES])
def test_every_route_one_tile_per_block(fam):
    fid, route, dtype, n_fft, hop, squeezing, _, kinds = fam
    F = max(_tile_frames(n_fft, hop, dtype, squeezing, k) for k in kinds)      # 0 on the unfused routes
    n_frames = 2 * F + F // 2 + 1 if F else 7                                  # 3 tiles, the last one ragged
    N = _window_len(n_frames, hop)
    lay = Layout(N, hop, 3, 3)
    buf = lay.buffer(dtype, 400)
    X = lay.gather(buf)
    eng = _engine(N, n_fft, hop, dtype, squeezing)
    outs = {}
    try:
        fused = bool(eng.lib.ssq_stft_plan_is_fused(eng.plan))
        for kind in kinds:
            r = route_of(eng, kind)
            Fk, tiles, blocks = eng.launch_info(9, kind)
            print(f"STRIDED {fid} {KIND_NAMES[kind]}: route={r} tile_frames={Fk} total_tiles={tiles} max_blocks={blocks} "
                  f"N={N} sig_stride={lay.sig_stride} group_stride={lay.group_stride}")
            # fp32 n_fft = 1024: Tx and (w, k) have a kernel of their own, Sx / dSx run the general one
            assert r == (route if kind in (TX, WK) or route != "TX1024" else "FUSED_POW2"), (fid, kind, r)
            assert tiles <= blocks and (tiles == 9 * -(-n_frames // Fk) if fused else tiles == 0), (fid, tiles, blocks)
            if fused:
                assert -(-n_frames // Fk) >= 2 and n_frames % Fk != 0
            outs[kind] = run_plain(eng, kind, X)
            assert_windows_equal(run_strided(eng, kind, buf, lay), outs[kind], f"{fid} {KIND_NAMES[kind]}")
    finally:
        eng.close()
    oracle_tie(fam, X, outs, (1, 8))


# ========================================================================================================= walk ========
WALK = ["pow2-f32-64", "pow2-f64-64", "split-f64-1024", "mixed-f32-1000", "blue-f64-333", "tx1024-f32", "tx1024-f32-lebesgue"]


@pytest.mark.parametrize("fid", WALK)
def test_walk_crosses_windows_and_groups(fid):
    fam = BY_ID[fid]
    _, route, dtype, n_fft, hop, squeezing = fam[:6]
    F, grid = _grid(n_fft, hop, dtype, squeezing, TX)
    n_frames = 3 * F + F // 2 + 1                                              # 4 tiles, the last one ragged
    N = _window_len(n_frames, hop)
    tps = -(-n_frames // F)
    assert 3 <= tps <= 5
    group = -(-(2 * grid + 1) // (3 * tps))
    while (3 * group * tps) % grid == 0:
        group += 1
    lay = Layout(N, hop, 3, group)
    B = 3 * group
    buf = lay.buffer(dtype, 500)
    X = lay.gather(buf)
    eng = _engine(N, n_fft, hop, dtype, squeezing)
    try:
        r = route_of(eng, TX)
        print(f"STRIDED {fid} walk: route={r} windows={B} group={group} N={N}")
        assert r == route
        _, tiles, blocks = _assert_walk(eng, B, TX, f"{fid} strided walk")
        assert tps < blocks                                                    # one advance() skips whole windows
        ref = run_plain(eng, TX, X)
        a, b = run_strided(eng, TX, buf, lay, repeat=2)
        assert np.array_equal(_bits(a), _bits(b)), "two runs of the same strided batch differ"
        assert_windows_equal(a, ref, f"{fid} walk tx")
    finally:
        eng.close()
    oracle_tie(fam, X, {TX: ref}, (group - 1, B - 1))                          # the last window of a group, and of the batch


# ======================================================================================================== split ========
@pytest.mark.parametrize("fid,n_fft,hop", [("pow2-f32-256", 256, 64), ("split-f64-1024", 1024, 256), ("tx1024-f32", 1024, 256)])
def test_interior_and_edge_launches_on_a_strided_batch(fid, n_fft, hop, monkeypatch):
    dtype = F64 if "f64" in fid else F32
    route = {"pow2-f32-256": "FUSED_POW2", "split-f64-1024": "FUSED_SPLIT", "tx1024-f32": "TX1024"}[fid]
    F = _tile_frames(n_fft, hop, dtype, "sum", TX)
    n_frames = 5 * F + F // 2 + 1                                              # 6 tiles: interior ones in the middle
    N = _window_len(n_frames, hop)
    lay = Layout(N, hop, 3, 3)
    buf = lay.buffer(dtype, 600)
    X = lay.gather(buf)
    eng = _engine(N, n_fft, hop, dtype, "sum")
    try:
        assert route_of(eng, TX) == route
        monkeypatch.setenv("SSQ_SINGLE_LAUNCH", "0")
        launches = eng.launch_list(9, TX)
        print(f"STRIDED {fid} split: route={route} launches(edge, tiles, blocks)={launches} tile_frames={F} N={N}")
        assert [l[0] for l in launches] == [0, 1], launches                    # the interior launch, then the edge launch
        assert launches[0][1] > 0 and launches[0][1] % 9 == 0 and launches[0][1] + launches[1][1] == 9 * 6
        split = run_strided(eng, TX, buf, lay)
        ref_split = run_plain(eng, TX, X)
        monkeypatch.setenv("SSQ_SINGLE_LAUNCH", "1")
        assert [l[0] for l in eng.launch_list(9, TX)] == [1]
        single = run_strided(eng, TX, buf, lay)
        ref_single = run_plain(eng, TX, X)
    finally:
        eng.close()
    monkeypatch.delenv("SSQ_SINGLE_LAUNCH")
    assert_windows_equal(split, ref_split, f"{fid} split")
    assert_windows_equal(single, ref_single, f"{fid} single launch")
    assert_windows_equal(split, single, f"{fid} split against the single launch")
    win = np.hanning(n_fft)
    for b in (0, 8):
        one, _ = _rs.ssq_stft(X[b], win, n_fft=n_fft, hop_len=hop, fs=1.0)
        assert np.array_equal(_bits(one), _bits(split[b]))
        (_check_ssq_f32 if dtype == F32 else _check_ssq_f64)(X[b], win, n_fft, hop, 1.0, "reflect", "sum")


# ============================================================================================ past the grid limit ======
def test_direct_sums_slice_a_strided_batch_past_65535_windows():
    """stft_generic.hip slices a batch at 65535 signals (grid.z of dft_frames_kernel, grid.y of reassign_cols_kernel) and
    hands the kernels the slice's first signal `b0`; they index the signals through sig_base, so a strided batch must
    slice the same way.  7 groups of 9364 overlapping windows of 48 samples, fp32, n_fft = 16: Tx and Sx against the same
    windows as two plain batches of fewer than 65535."""
    n_fft, hop, N, n_groups, group = 16, 4, 48, 7, 9364
    B = n_groups * group
    assert B == 65548
    lay = Layout.__new__(Layout)
    lay.N, lay.n_groups, lay.group, lay.sig_stride, lay.base = N, n_groups, group, 17, 3
    lay.group_stride = ((group - 1) * 17 + N + 4) | 1
    lay.size = lay.base + (n_groups - 1) * lay.group_stride + (group - 1) * 17 + N
    buf = np.random.default_rng(65548).standard_normal(lay.size).astype(F32)
    X = lay.gather(buf)
    eng = _engine(N, n_fft, hop, F32, "sum")
    try:
        assert (eng.n_freqs, eng.n_frames) == (9, 12)
        half = B // 2
        for kind in (TX, SX):
            r = route_of(eng, kind)
            print(f"STRIDED grid limit {KIND_NAMES[kind]}: route={r} windows={B}")
            assert r == "DFT" and eng.launch_info(B, kind)[1] == 0
            ref = np.concatenate([run_plain(eng, kind, X[:half]), run_plain(eng, kind, X[half:])])
            assert_windows_equal(run_strided(eng, kind, buf, lay), ref, f"65548 windows {KIND_NAMES[kind]}")
    finally:
        eng.close()
    Sx_o, _ = o.stft(X[65540].astype(np.float64), n_fft, hop, np.hanning(n_fft), "reflect")
    assert _relerr(ref[65540], Sx_o) <= SX_BOUND["dft"][1]                     # (`ref` is the Sx run here)


# ===================================================================================================== refusals ========
def test_strided_refusals():
    lib = _lib.load()
    N, n_fft, hop = 60, 17, 5
    lay = Layout(N + 1, hop, 3, 3)                                             # 61 samples: no multiple of the hop
    buf = lay.buffer(F32, 700)
    eng = _engine(lay.N, n_fft, hop, F32, "sum")
    try:
        assert route_of(eng, TX) == "DFT"
        ws = int(lib.ssq_stft_plan_workspace_bytes(eng.plan, 9, TX))
        assert ws > 0
        nb = 9 * eng.n_freqs * eng.n_frames * 8
        with Door() as d:
            dx, dout, dws = d.buf(buf.nbytes, buf), d.buf(nb), d.buf(ws)

            def call(n_groups, group, gs, ss, ws_bytes=ws):
                return lib.ssq_stft_plan_exec_strided(eng.plan, TX, dx.p, n_groups, group, gs, ss, dout.p, dws.p, ws_bytes, None)

            def untouched():
                _lib.check(lib.ssq_device_sync())
                return bool((dout.get((nb,), np.uint8) == 0xA5).all()) and dout.guard_untouched()
            for gs, ss in ((0, lay.sig_stride), (-1, lay.sig_stride), (lay.group_stride, -1)):
                assert call(3, 3, gs, ss) != 0 and "bad strides" in lib.ssq_last_error().decode(), (gs, ss)
                assert untouched()
            assert call(0, 3, lay.group_stride, lay.sig_stride) == 0 and untouched()
            assert call(3, 0, lay.group_stride, lay.sig_stride) == 0 and untouched()
            assert call(3, 3, lay.group_stride, lay.sig_stride, ws - 1) != 0
            assert "workspace too small for the unfused STFT path" in lib.ssq_last_error().decode()
            assert untouched()
            assert call(3, 3, lay.group_stride, lay.sig_stride) == 0 and not untouched()    # and the call itself runs
    finally:
        eng.close()
