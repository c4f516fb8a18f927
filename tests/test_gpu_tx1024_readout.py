"""GPU tests of `stft_tx1024_kernel`'s Nyquist-bin path and tile read-out (csrc/stft_fused.hip): fp32, n_fft 1024,
hop 256, Hann, OUT_TX, in the regime bench.py times -- the interior launch followed by the edge launch, every block
walking two tiles or more, so the read-out's re-zero of tile i is what tile i + 1 accumulates into.

Shapes (sized from `ssq_stft_plan_launch_list`, asserted per case):
  even: N = 24 576 -> 96 frames, 6 tiles: the paired 16-byte read-out of the interior kernel;
  odd : N = 24 832 -> 97 frames, 7 tiles, the last one ragged: the unpaired fallback of the same kernel.
Signals 0..3 of every batch carry Nyquist content (`_signals`): +a (-1)^n and -a (-1)^n plus 1e-3 a noise (bin 512 holds
most of each column's L1 mass and sets its column scale; the sign of RE decides whether the 64-bit add borrows), a
signal that is exactly zero over whole frames (den = 0, d = NaN: every bin of those frames masked), and a synthetic
signal plus 0.01 (-1)^n, whose Nyquist bin the plan with gamma = 40 masks by the keep threshold (|Sx[512]| is about 5
there, 10 if counted on the kernel's unnormalised pair sum; the sines' ridges are above 100) and the default plan keeps.

Checked against, never against the kernel under test alone:
  * tests/golden/tx1024_parent_bits.npz, recorded on the GPU from the commit before the read-out rework (its
    `parent_commit` entry; generator: tests/golden/make_tx1024_parent_bits.py): a CRC32 of every signal's Tx bytes, and
    in full row 512 and the first and last frame column of the signals in FULL_SIGNALS (all of a batch would not fit
    the size limit of a committed file); for the (w, k) hook a CRC32 per signal and row 512 of the same signals.
    The fixed-point tile makes Tx order-exact, so the comparison is bitwise;
  * the fp64 oracle through `_check_ssq_f32` (tests/test_gpu_stft.py) on one interior-path signal and on every
    Nyquist-content signal, the drop-in call first shown to give the batch's bits;
  * the unfused generic kernels (`force_generic`), an independent fp32 implementation, on two signals: the comparison
    of tests/test_gpu_stft.py::test_ssq_stft_fused_vs_generic_kernels -- column sums (invariant under bin flips) and
    the fraction of differing elements <= 1e-3.  That test is fp64 and puts 1e-9 max|Tx| on both; fp32 cannot resolve
    1e-9 (eps = 6e-8), so here both take the fp32 Tx figure of the same file, 2e-5 max|Tx| (a column sums
    513 cells of 2^-30 column-scale resolution on top of fp32 Sx at 2e-6).
"""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

from oracle import ssq_oracle as o
from ssqueeze_rs_amd import _lib, _rs
from ssqueeze_rs_amd.batch import SsqStftBatch
from tests.test_gpu_stft import _check_ssq_f32

pytestmark = pytest.mark.gpu

N_FFT, HOP = 1024, 256
N_EVEN, N_ODD = 24576, 24832
GAMMA_MASK = 40.0
NYQ_SIGNALS = (0, 1, 2, 3)                       # see _signals
PLAIN = 7                                        # the interior-path signal that goes to the oracle
FULL_SIGNALS = (0, 1, 2, 3, 4, 7, 130, 259)      # rows / columns the fixture holds in full
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tx1024_parent_bits.npz")
# case -> (N, squeezing, gamma, out kind)
CASES = {
    "even": (N_EVEN, "sum", None, _lib.OUT_TX),
    "odd": (N_ODD, "sum", None, _lib.OUT_TX),
    "gamma": (N_EVEN, "sum", GAMMA_MASK, _lib.OUT_TX),
    "lebesgue": (N_EVEN, "lebesgue", None, _lib.OUT_TX),
    "wk": (N_EVEN, "sum", None, _lib.OUT_WK),
}


@pytest.fixture(autouse=True)
def _default_launch_split(monkeypatch):
    monkeypatch.delenv("SSQ_SINGLE_LAUNCH", raising=False)


def _signals(N, B):
    """[B, N] fp32.  0: +(-1)^n, 1: -(-1)^n (0.75 amplitude, 1e-3 relative noise), 2: synthetic with samples
    [6144, 14336) exactly zero (frames 26..52 read nothing else), 3: signal PLAIN + 0.01 (-1)^n, the rest synthetic.
    (Seeds checked with the fp64 oracle on the CPU: signals 3 and PLAIN have no strong bin within 4e-4 bins of a half-bin
    tie at either length, 0 and 1 none within 0.4 -- the fp32 w error is below 1e-4 bins -- so the reference itself
    stays clear of the bin-parity bounds of `_check_ssq_f32`.)"""
    n = np.arange(N)
    alt = np.where(n % 2 == 0, 1.0, -1.0)
    x = np.stack([o.synth_signal(N, 500 + b, np.float64) for b in range(B)])
    noise = np.random.default_rng(77).standard_normal((2, N))
    x[0] = 0.75 * (alt + 1e-3 * noise[0])
    x[1] = -0.75 * (alt + 1e-3 * noise[1])
    x[2, 6144:14336] = 0.0
    x[3] = x[PLAIN] + 0.01 * alt
    return x.astype(np.float32)


def _engine(N, squeezing, gamma, B):
    return SsqStftBatch(N, np.hanning(N_FFT), N_FFT, HOP, fs=1.0, squeezing=squeezing, gamma=gamma, dtype=np.float32,
                        max_batch=B)


def _split_ok(launches):
    return [l[0] for l in launches] == [0, 1] and all(t >= 2 * g + 1 and t % g != 0 for _, t, g in launches)


def _batch_size(N, kind):
    """About 260 signals: the smallest batch from 260 up at which both launches give every block two tiles or more."""
    probe = _engine(N, "sum", None, 1)
    try:
        B = 260
        while not _split_ok(probe.launch_list(B, kind)):
            B += 1
            assert B <= 1100, "no batch puts two tiles per block on both launches"
        return B
    finally:
        probe.close()


def run_case(case):
    """(x, out of the first run, out of the second run) of a case, its regime asserted.  Shared with the generator."""
    N, squeezing, gamma, kind = CASES[case]
    B = _batch_size(N, kind)
    x = _signals(N, B)
    eng = _engine(N, squeezing, gamma, B)
    try:
        launches = eng.launch_list(B, kind)
        print(f"TX1024 {case}: batch={B} launches(edge, tiles, blocks)={launches}")
        assert _split_ok(launches), (case, launches)       # interior launch + edge launch, >= 2 tiles per block
        assert eng.n_frames == (96 if N == N_EVEN else 97)
        return x, eng.run(x, kind), eng.run(x, kind)
    finally:
        eng.close()


def crc_per_signal(a):
    return np.array([zlib.crc32(np.ascontiguousarray(a[b]).tobytes()) for b in range(a.shape[0])], dtype=np.uint32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_RUNS = {}


def _case(case):
    """Each case runs once per session (twice on the device); the results are shared read-only."""
    if case not in _RUNS:
        x, out, again = run_case(case)
        for a in (x, out, again):
            a.setflags(write=False)
        _RUNS[case] = (x, out, again)
    return _RUNS[case]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", list(CASES))
def test_bits_of_the_parent_commit(case, golden):
    x, out, again = _case(case)
    assert np.array_equal(_bits(out), _bits(again)), "two runs of the same batch differ"
    assert x.shape[0] == int(golden[f"{case}_B"]), "the fixture was recorded at another batch size (CU count)"
    assert np.array_equal(crc_per_signal(x), golden[f"{case}_xcrc"]), "the inputs are not the fixture's"
    full = [b for b in FULL_SIGNALS if b < x.shape[0]]
    # the parts held in full first: they say where a difference is
    for i, b in enumerate(full):
        assert np.array_equal(_bits(out[b, 512]), _bits(golden[f"{case}_row512"][i])), (case, b, "row 512")
        if case != "wk":
            assert np.array_equal(_bits(out[b, :, 0]), _bits(golden[f"{case}_col_first"][i])), (case, b, "first column")
            assert np.array_equal(_bits(out[b, :, -1]), _bits(golden[f"{case}_col_last"][i])), (case, b, "last column")
    bad = np.flatnonzero(crc_per_signal(out) != golden[f"{case}_crc"])
    assert bad.size == 0, f"{case}: signals {bad[:8].tolist()} ({bad.size}) differ from the parent commit's bits"


def test_nyquist_content_is_what_the_cases_claim(golden):
    """The inputs do what the docstring says, read from the PARENT's recorded rows: bin 512 dominates the columns of
    signals 0 and 1 with opposite signs of RE, the zeroed frames of signal 2 are empty, and gamma = 40 masks the
    Nyquist bin of signal 3 that the default plan keeps."""
    r = golden["even_row512"]
    c0 = golden["even_col_first"]
    assert np.abs(c0[0][512]) > 0.5 * np.abs(c0[0]).sum() and np.abs(c0[1][512]) > 0.5 * np.abs(c0[1]).sum()
    assert (np.sign(r[0].real) == -np.sign(r[1].real)).all() and (r[0].real != 0).all()
    x, out, _ = _case("even")
    assert not out[2][:, 28:51].any()
    assert np.abs(golden["even_row512"][3]).min() > 0 and not golden["gamma_row512"][3].any()


@pytest.mark.parametrize("case,b", [("even", b) for b in NYQ_SIGNALS + (PLAIN,)] + [("odd", b) for b in NYQ_SIGNALS + (PLAIN,)]
                         + [("lebesgue", 0), ("lebesgue", PLAIN)])
def test_oracle(case, b):
    """Signal b of the batch: the drop-in call gives the batch's bits, and passes the fp64 oracle checks."""
    N, squeezing, _, _ = CASES[case]
    x, out, _ = _case(case)
    win = np.hanning(N_FFT)
    one, _ = _rs.ssq_stft(x[b], win, n_fft=N_FFT, hop_len=HOP, fs=1.0, squeezing=squeezing)
    assert np.array_equal(_bits(one), _bits(out[b]))
    with np.errstate(all="ignore"):                  # signal 2: 0 / 0 in the oracle's phase transform
        _check_ssq_f32(x[b], win, N_FFT, HOP, 1.0, "reflect", squeezing)


def test_gamma_plan_gives_the_drop_in_bits():
    x, out, _ = _case("gamma")
    for b in (3, PLAIN):
        one, _ = _rs.ssq_stft(x[b], np.hanning(N_FFT), n_fft=N_FFT, hop_len=HOP, fs=1.0, gamma=GAMMA_MASK)
        assert np.array_equal(_bits(one), _bits(out[b]))


def _generic_tx(x1):
    lib = _lib.load()
    N = x1.shape[0]
    win = np.hanning(N_FFT)
    plan = C.c_void_p()
    _lib.check(lib.ssq_stft_plan_create(C.byref(plan), _lib.SSQ_F32, N, win.ctypes.data_as(C.c_void_p), N_FFT, HOP, 1.0,
                                        0, 0, -1.0, 1))
    try:
        assert lib.ssq_stft_plan_is_fused(plan) == 0
        nf, nfr = N_FFT // 2 + 1, (N - 1) // HOP + 1
        d_x, d_out, d_ws = C.c_void_p(), C.c_void_p(), C.c_void_p()
        ws = lib.ssq_stft_plan_workspace_bytes(plan, 1, _lib.OUT_TX)
        _lib.check(lib.ssq_dev_malloc(C.byref(d_x), N * 4))
        _lib.check(lib.ssq_dev_malloc(C.byref(d_out), nf * nfr * 8))
        _lib.check(lib.ssq_dev_malloc(C.byref(d_ws), max(ws, 16)))
        try:
            _lib.check(lib.ssq_memcpy_h2d(d_x, x1.ctypes.data_as(C.c_void_p), N * 4, None))
            _lib.check(lib.ssq_stft_plan_exec(plan, _lib.OUT_TX, d_x, 1, d_out, d_ws, ws, None))
            Tx = np.empty((nf, nfr), dtype=np.complex64)
            _lib.check(lib.ssq_device_sync())
            _lib.check(lib.ssq_memcpy_d2h(Tx.ctypes.data_as(C.c_void_p), d_out, Tx.nbytes, None))
            _lib.check(lib.ssq_device_sync())
        finally:
            for p in (d_x, d_out, d_ws):
                lib.ssq_dev_free(p)
    finally:
        lib.ssq_stft_plan_destroy(plan)
    return Tx


@pytest.mark.parametrize("case,b", [("even", 3), ("odd", PLAIN)])
def test_against_the_generic_kernels(case, b):
    x, out, _ = _case(case)
    gen = _generic_tx(np.ascontiguousarray(x[b])).astype(np.complex128)
    fus = out[b].astype(np.complex128)
    tmax = np.abs(gen).max()
    colsum = np.abs(fus.sum(0) - gen.sum(0)).max() / tmax
    frac = (np.abs(fus - gen) > 2e-5 * tmax).mean()
    print(f"TX1024 generic {case} signal {b}: column sums {colsum:.3e} of max|Tx|, differing fraction {frac:.3e}")
    assert colsum <= 2e-5
    assert frac <= 1e-3
