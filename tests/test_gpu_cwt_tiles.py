"""The time-tile kernel families of the fp32 `ssq_cwt` (csrc/cwt_os.hip, launched by `launch_time_tiles` in
csrc/api_cwt.hip), each at the smallest shape at which it exists, cell by cell: Tx against the re-accumulation of the
kernel's own (Wx, k), k against the kernel's own w, w against the kernel's own (Wx, dWx), and Wx / dWx of EVERY row
against the fp64 oracle (tests/helpers/cwt_scatter_check.py: the bounds and where they come from).

Which family ran is asserted from `ssq_cwt_plan_tile_segments`, which reads the plan fields the launcher launches from:

| case | N (padded P)          | scales 2^(j/4)                    | families that must hold at least one scale                  |
| A    | 2^18 (2^19 = 2 N)     | Morlet j = 4..47, GMW j = -1..43  | lead sweep, 4-row, 8-row, decimated, full-circle            |
| B    | 300 001 (2^19 < 2 N)  | the same                          | lead sweep, 4-row, 8-row, decimated; NO full-circle: the    |
|      |                       |                                   | coarse rows are read-modify-written behind the tiles         |
| C    | 350 003 (2^20, reg)   | Morlet j = 2..51, GMW j = -4..45  | analytic tiles + all of A; the untiled rows on the register |
|      |                       |                                   | core                                                        |
| D    | 2^18                  | 12 Morlet scales in [4, 341]      | every scale tiled: no frequency-domain transform at all     |

N is odd in B and C: the last 4096-, 2048- (full-circle) and 65536-sample (decimated) tiles are ragged and `col < N`
cuts inside a thread's four columns.  Inputs: the project's synthetic signal (short runs), a pure tone (one run carried
across all scales of a kernel and on into the next kernel), noise bursts between exact zeros (k = -1 gaps, empty columns,
the keep test) and unit impulses at a tile boundary (column 4096) and in the last column.
"""
import ctypes as C
import gc

import numpy as np
import pytest

from oracle import ssq_oracle as o
from ssqueeze_rs_amd import _lib, _rs
from tests.helpers import cwt_scatter_check as chk

pytestmark = pytest.mark.gpu

CASES = {"A": 1 << 18, "B": 300_001, "C": 350_003, "D": 1 << 18}
FAMILIES = ("lead", "analytic", "rows4", "rows8", "decimated", "full")
MUST = {
    "A": {"lead", "rows4", "rows8", "decimated", "full"},
    "B": {"lead", "rows4", "rows8", "decimated"},
    "C": {"lead", "analytic", "rows4", "rows8", "decimated", "full"},
    "D": {"rows4", "rows8"},
}


def _scales(case, wavelet):
    if case == "D":
        return np.geomspace(4.0, 341.0, 12)
    j = {("A", "morlet"): (4, 48), ("A", "gmw"): (-1, 44), ("B", "morlet"): (4, 48), ("B", "gmw"): (-1, 44),
         ("C", "morlet"): (2, 52), ("C", "gmw"): (-4, 46)}[case, wavelet]
    return 2.0 ** (np.arange(*j) / 4.0)


def _input(name, N):
    n = np.arange(N, dtype=np.float64)
    if name == "synth":
        return o.synth_signal(N, 91, np.float32)
    if name == "tone":
        return np.sin(2.0 * np.pi * 0.05 * n).astype(np.float32)
    if name == "bursts":                                   # a burst starts ON a tile boundary and ends inside a tile; the
        rng = np.random.default_rng(77)                    # gaps are longer than a 4096-sample tile with both halos
        x = np.zeros(N, dtype=np.float32)
        for start, length in ((8192, 3000), (70_001, 5000), (131_072 + 4095, 2), (200_000, 9000), (N - 1500, 1500)):
            x[start:start + length] = rng.standard_normal(length).astype(np.float32)
        return x
    assert name == "impulse"
    x = np.zeros(N, dtype=np.float32)
    x[4096] = 1.0
    x[N - 1] = 1.0
    return x


def _segments(N, wavelet, scales, fs=None, padtype="reflect"):
    """The plan's own account of which rows each family serves: ({family: (begin, end)}, reg, tiled rows)."""
    lib = _lib.load()
    vp = C.c_void_p
    plan = vp()
    sc = np.ascontiguousarray(scales, dtype=np.float64)
    _lib.check(lib.ssq_cwt_plan_create(C.byref(plan), _lib.SSQ_F32, N, _lib.WAVELET[wavelet], sc.ctypes.data_as(vp),
                                       len(sc), 1.0 if fs is None else 1.0 / fs, _lib.PAD[padtype]))
    out = (C.c_int32 * 8)(*([-7] * 8))
    _lib.check(lib.ssq_cwt_plan_tile_segments(plan, out))
    tiled = lib.ssq_cwt_plan_tiled_rows(plan)
    _lib.check(lib.ssq_cwt_plan_destroy(plan))
    a0, s0, mid, s1, d1, z0, z1, reg = list(out)
    first = a0 if s1 > s0 else (z0 if z1 > z0 else len(sc))
    seg = dict(lead=(0, first), analytic=(a0, s0), rows4=(s0, mid), rows8=(mid, s1), decimated=(s1, d1), full=(z0, z1))
    return seg, bool(reg), tiled


def _family_of_rows(seg, na):
    fam = np.full(na, "rmw", dtype=object)                # behind the tiles: read-modify-write column reassignment
    for name in FAMILIES:
        fam[seg[name][0]:seg[name][1]] = name
    return fam


_oracle = {}


def _oracle_for(case, wavelet, inp, x, scales, fs, padtype):
    """o.cwt of one (case, wavelet, input, fs, padtype), computed once and kept for the neighbouring test only (two
    fp64 planes of 45 x 3e5)."""
    key = (case, wavelet, inp, fs, padtype)
    if key not in _oracle:
        _oracle.clear()
        _oracle[key] = chk.oracle_cwt_rows(x, wavelet, scales, fs, padtype)
    return _oracle[key]


@pytest.fixture(autouse=True)
def _release_debug_planes():
    yield
    gc.collect()                                          # the four pinned planes of a debug call go back to the pool


@pytest.fixture(autouse=True, scope="module")
def _release_pool():
    yield
    _oracle.clear()
    gc.collect()
    _lib.load().ssq_host_cache_clear()                    # ... and the pool lets go of them behind the last case


RUNS = [
    ("A", "morlet", "synth", {}),
    ("A", "morlet", "synth", dict(squeezing="lebesgue")),
    ("A", "gmw", "synth", {}),
    ("A", "morlet", "tone", {}),
    ("A", "gmw", "bursts", {}),
    ("A", "morlet", "impulse", dict(flipud=False)),
    ("B", "morlet", "synth", dict(flipud=False)),
    ("B", "gmw", "tone", dict(padtype="zero")),
    ("B", "morlet", "bursts", {}),
    ("B", "gmw", "impulse", {}),
    ("C", "morlet", "synth", dict(ssq_freqs="linear")),
    ("C", "gmw", "tone", {}),
    ("C", "morlet", "bursts", dict(fs=50.0, gamma=1e-3)),
    ("C", "gmw", "impulse", dict(squeezing="lebesgue")),
    ("D", "morlet", "synth", {}),
    ("D", "morlet", "tone", dict(squeezing="lebesgue")),
    ("D", "morlet", "bursts", dict(padtype="zero")),
    ("D", "morlet", "impulse", dict(fs=50.0, gamma=1e-3)),
]


def _assert_case_segments(case, seg, reg, tiled, na, wavelet=None, scales=None):
    if wavelet is not None and seg["analytic"][1] > seg["analytic"][0]:
        # the continued wavelet of an analytic-input row peaks below the Nyquist frequency (the finding)
        peak = 6.0 if wavelet == "morlet" else 20.0 ** (1.0 / 3.0)
        assert peak / scales[seg["analytic"][0]] <= np.pi, (wavelet, scales[seg["analytic"][0]])
    # `lead`: rows in front of the first tiled one.  That they go through the plain-store sweep (and not the
    # read-modify-write loop behind the tiles) also takes `cwt_reassign_can_sweep(na)` (csrc/api_cwt.hip: `lead_sweep`;
    # csrc/cwt_kernels.hip: na <= 8192, the written-rows bitmap in LDS), which the query does not report: held here, and
    # if that rule changes these cases need a shape on either side of it
    assert na <= 8192
    for name in MUST[case]:
        assert seg[name][1] > seg[name][0], (case, name, seg)
    if case == "B":
        assert seg["full"][1] == seg["full"][0], seg       # os_z1 == os_z0: the coarse rows behind the tiles are
        assert seg["decimated"][1] < na                    # reassigned column by column, read-modify-write
    if case == "C":
        assert reg and seg["lead"][1] > 0                  # the rows in front of the analytic tiles: register core
    else:
        assert not reg
    if case == "D":
        assert tiled == na and seg["rows4"][0] == 0 and seg["rows8"][1] == na    # all_tiled
    else:
        assert tiled < na


@pytest.mark.parametrize("case,wavelet,inp,opts", RUNS,
                         ids=[f"{c}-{w}-{i}-{'-'.join(f'{k}={v}' for k, v in kw.items()) or 'default'}"
                              for c, w, i, kw in RUNS])
def test_ssq_cwt_tile_families_cell_by_cell(case, wavelet, inp, opts):
    N = CASES[case]
    scales = _scales(case, wavelet)
    na = len(scales)
    fs, padtype = opts.get("fs"), opts.get("padtype", "reflect")
    seg, reg, tiled = _segments(N, wavelet, scales, fs, padtype)
    _assert_case_segments(case, seg, reg, tiled, na, wavelet, scales)
    x = _input(inp, N)
    oracle = _oracle_for(case, wavelet, inp, x, scales, fs, padtype)
    r = chk.check_ssq_cwt_cells(x, oracle=oracle, wavelet=wavelet, scales=scales, **opts)
    fam = _family_of_rows(seg, na)
    print(f"\n[tiles] {case} {wavelet} {inp} {opts} segments {seg} reg {int(reg)} tiled {tiled}/{na} "
          f"gamma_exempt {r['gamma_exempt']:.2e} bin_mismatch {r['bin_mismatch']:.2e} "
          f"empty_columns {int((r['k'] < 0).all(axis=0).sum())}")
    for name in sorted(set(fam)):
        m = fam == name
        print(f"[tiles]   {name:9s} rows {int(m.sum()):2d}  scatter {r['scatter_rows'][m].max():.3f}  w {r['w_rows'][m].max():.3f}  "
              f"Wx {r['wx_rows'][m].max():.3f}  dWx {r['dwx_rows'][m].max():.3f}   (err / bound)")
    if inp == "bursts" and case == "D":
        assert (r["k"] < 0).all(axis=0).any()             # whole columns without a term: Tx must be exactly zero there


def test_tile_families_batch_of_two_equals_single_calls():
    """Case A, two signals through one plan and one workspace: each equals its own call bit for bit."""
    N = CASES["A"]
    scales = _scales("A", "morlet")
    seg, reg, tiled = _segments(N, "morlet", scales)
    _assert_case_segments("A", seg, reg, tiled, len(scales))
    xb = np.stack([_input("synth", N), _input("bursts", N)])
    Txb, fb = _rs.ssq_cwt(xb, wavelet="morlet", scales=scales)
    for i in range(2):
        Tx, f = _rs.ssq_cwt(xb[i], wavelet="morlet", scales=scales)
        assert np.array_equal(f, fb)
        assert np.array_equal(Tx.view(np.uint32), Txb[i].view(np.uint32)), i
    assert np.count_nonzero(Txb[1]) > 0


def test_tile_families_second_call_reproduces_the_first():
    """Case A twice in one process: Tx is cleared on a side stream while the transforms run, and every kernel that
    writes Tx waits for that clear; a missed wait shows as a difference between two calls."""
    N = CASES["A"]
    scales = _scales("A", "gmw")
    seg, reg, tiled = _segments(N, "gmw", scales)
    _assert_case_segments("A", seg, reg, tiled, len(scales))
    x = _input("synth", N)
    first = _rs.ssq_cwt(x, wavelet="gmw", scales=scales)[0].copy()
    for _ in range(2):
        again = _rs.ssq_cwt(x, wavelet="gmw", scales=scales)[0]
        assert np.array_equal(first.view(np.uint32), again.view(np.uint32))
