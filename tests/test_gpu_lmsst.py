"""GPU tests of the local maximum synchrosqueezed STFT, `upstream.lmssq_stft` (csrc/stft_lmsst.hip), against
the numpy model tests/helpers/lmsst_ref.py.

The window maximum is integer work on the call's own `Sx`: it is compared with `np.array_equal`.  The scatter is held to
the bound of test_gpu_msst.py, 4 eps dw sum|Sx| per column.  The kernel runs ONE real-input transform with the window
alone, not `ssq_stft2`'s packed pair, so `Sx` may differ from `ssq_stft2`'s by the rounding of another FFT arrangement:
it is bounded by 10 x the difference between the model's FFT and DFT-matrix arithmetics on the strong bins."""
import ctypes as C
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.helpers import lmsst_ref as r
from tests.helpers import msst_ref as ms
from tests.helpers import sst2_ref as m2
from tests.test_gpu_sst2 import strong, two_chirps, window

pytestmark = pytest.mark.gpu

FS = 2.0
# (N, n_fft, hop, padtype, extra keywords): F = 9, where delta = 8 covers every column; the multi-wave frame route; the
# largest frame
CASES = [
    (600, 64, 1, "reflect", dict()),
    (500, 16, 3, "zero", dict()),
    (3000, 1024, 7, "wrap", dict(flipud=True)),
    (5000, 4096, 64, "symmetric", dict(squeezing="lebesgue")),
]
IDS = ["%d-%d-%d-%s" % c[:4] for c in CASES]
DTYPES = pytest.mark.parametrize("rdt", [np.float64, np.float32], ids=["f64", "f32"])
DELTAS = ("one", "default", "top")
EVERY = pytest.mark.parametrize("which", DELTAS)
CASE = pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)


def delta_of(i, which):
    n = CASES[i][1]
    F = n // 2 + 1
    return {"one": 1, "default": up.lmsst_default_delta(window(n), n), "top": min(F - 1, 256)}[which]


@functools.lru_cache(maxsize=None)
def gpu(i, rdt, which):
    N, n, hop, pad, kw = CASES[i]
    out = up.lmssq_stft(two_chirps(N, i).astype(rdt), window(n), n_fft=n, hop_len=hop, fs=FS, padtype=pad,
                        delta=delta_of(i, which), get_bins=True, **kw)
    for a in out:
        a.setflags(write=False)
    return out


@DTYPES
@EVERY
@CASE
def test_bins_are_the_model_on_the_calls_own_sx(i, rdt, which):
    N, n, hop, pad, kw = CASES[i]
    F = n // 2 + 1
    Tx, Sx, f, Sfs, bins = gpu(i, rdt, which)
    assert Tx.shape == Sx.shape == bins.shape == (F, (N - 1) // hop + 1)
    assert Tx.dtype == Sx.dtype == (np.complex64 if rdt == np.float32 else np.complex128)
    assert Sfs.dtype == f.dtype == rdt and bins.dtype == np.int32
    Sfs_ref = np.linspace(0, .5 * FS, F, dtype=rdt)
    assert np.array_equal(Sfs, Sfs_ref) and np.array_equal(f, Sfs_ref[::-1] if kw.get("flipud") else Sfs_ref)
    gamma = 10 * float(np.finfo(rdt).eps)
    ref = r.stft_bins(Sx, delta_of(i, which), gamma, kw.get("flipud", False))
    kept = bins >= 0
    assert np.array_equal(bins[kept], ref[kept])
    # the keep rule runs on the fp64 coefficient: it agrees with |Sx| <= gamma except within 1e-6 relative of gamma
    mag = np.abs(Sx.astype(np.complex128))
    clear = np.abs(mag - gamma) > 1e-6 * gamma
    assert np.array_equal(kept[clear], (mag > gamma)[clear])
    own = np.broadcast_to((F - 1 - np.arange(F) if kw.get("flipud") else np.arange(F))[:, None], bins.shape)
    print("delta %d: %d of %d cells kept, %d moved off their row" % (delta_of(i, which), kept.sum(), kept.size,
                                                                     (bins[kept] != own[kept]).sum()))


@DTYPES
@EVERY
@CASE
def test_tx_is_the_scatter_of_the_calls_own_bins(i, rdt, which):
    """Tx == the rows-ascending scatter of the call's own Sx under the call's own bins, within 4 eps dw sum|Sx| per
    column (the bound of test_gpu_msst.py::test_tx_is_the_scatter_of_the_calls_own_bins)."""
    N, n, hop, pad, kw = CASES[i]
    F = n // 2 + 1
    Tx, Sx, _, _, bins = gpu(i, rdt, which)
    dw = rdt(np.linspace(0, .5 * FS, F)[1])
    ref = ms.scatter(Sx, bins, dw, kw.get("squeezing", "sum"))
    tol = 4 * np.finfo(rdt).eps * float(dw) * np.abs(Sx).sum(0).astype(np.float64)
    err = np.abs(Tx.astype(np.complex128) - ref).max(0)
    print("worst column: %.3g of its tolerance" % (err / np.maximum(tol, 1e-300)).max())
    assert (err <= tol).all()


@CASE
def test_sx_against_the_model(i):
    """A real-input transform with the window alone: Sx (float64) against the model's FFT arithmetic, within 10 x the
    difference between the model's FFT and DFT-matrix arithmetics on the strong bins (as test_gpu_msst.py bounds w).
    Measured on an MI355X: 4.0e-15, 8.9e-16, 3.3e-14 and 4.3e-14 against bounds of 9.1e-14, 1.7e-14, 9.3e-13 and 1.2e-12;
    the distance to `ssq_stft2`'s Sx (a packed pair and a split) is of the same size, 9.0e-16 ... 4.3e-14."""
    N, n, hop, pad, kw = CASES[i]
    x, win = two_chirps(N, i), window(n)
    Vf = r.stft_V(x, win, n, hop, pad, True, "fft")
    Vd = r.stft_V(x, win, n, hop, pad, True, "dft")
    Sx = gpu(i, np.float64, "default")[1]
    big = strong(Vf)
    tol = 10 * np.abs(Vf - Vd)[big].max()
    err = np.abs(Sx - Vf)[big].max()
    S2 = up.ssq_stft2(x, win, n_fft=n, hop_len=hop, fs=FS, padtype=pad)[1]
    print("Sx err %.3g (tol %.3g, %d strong bins); against ssq_stft2's Sx %.3g" % (err, tol, big.sum(), np.abs(Sx - S2).max()))
    assert err <= tol


@DTYPES
@pytest.mark.parametrize("i", [0, 1], ids=IDS[:2])
def test_the_widest_window_sends_a_column_to_its_largest_row(i, rdt):
    """delta = F - 1 (the cases whose F - 1 is within the bound of 256): the window is the whole column."""
    N, n, hop, pad, kw = CASES[i]
    F = n // 2 + 1
    assert delta_of(i, "top") == F - 1
    Tx, Sx, _, _, bins = gpu(i, rdt, "top")
    top = r.energy(Sx).argmax(0)                                   # (argmax: the first of equal maxima, the lowest row)
    want = F - 1 - top if kw.get("flipud") else top
    kept = bins >= 0
    assert np.array_equal(bins[kept], np.broadcast_to(want, bins.shape)[kept])
    rows = np.arange(F)[:, None] == want[None, :]
    assert not Tx[~rows].any()                                     # everything else was written as zero


@DTYPES
@pytest.mark.parametrize("N,n,hop", [(600, 64, 1), (3000, 1024, 7)])
def test_batch_equals_single_calls_and_is_deterministic(rdt, N, n, hop):
    X = np.stack([two_chirps(N, s) for s in (11, 12, 13)]).astype(rdt)
    win = window(n)
    kw = dict(n_fft=n, hop_len=hop, fs=FS, get_bins=True)
    B = up.lmssq_stft(X, win, **kw)
    assert B[0].shape == B[4].shape == (3, n // 2 + 1, (N - 1) // hop + 1)
    for b in range(3):
        one = up.lmssq_stft(X[b], win, **kw)
        for k in (0, 1, 4):
            assert np.array_equal(B[k][b], one[k]), (b, k)
    again = up.lmssq_stft(X, win, **kw)
    for k in (0, 1, 4):
        assert np.array_equal(B[k], again[k]), k


def test_inverts_like_the_second_order_transform():
    N, n = 600, 64
    x = two_chirps(N, 5)
    win = window(n)
    Txl = up.lmssq_stft(x, win, n_fft=n)[0]
    Tx2 = up.ssq_stft2(x, win, n_fft=n)[0]
    xl, x2 = up.issq_stft(Txl, win), up.issq_stft(Tx2, win)
    print("inverse difference %.3g, reconstruction error %.3g" % (np.abs(xl - x2).max(), np.abs(xl - x).max()))
    assert not np.array_equal(Txl, Tx2)
    assert np.abs(xl - x2).max() <= 1e-9 * np.abs(x).max()


def test_concentrates_a_noisy_fm_signal():
    """The sinusoidal FM of DESIGN 4.17 (N = 1024, n_fft = 256, Gaussian sigma = 24, hop 1) plus 0.3 N(0, 1), seed 7: the
    share of each column's |Tx|^2 in the column's largest cell.  Model: 0.82 at the default delta (7), where the model of
    `ssq_stft2` has 0.42.  Measured on an MI355X: 0.8245 (model 0.8245) against `ssq_stft2`'s 0.4217."""
    N, n = 1024, 256
    x = ms.fm_signal(N)[0] + 0.3 * np.random.default_rng(7).standard_normal(N)
    win = m2.gauss_window(n, 24)
    delta = up.lmsst_default_delta(win, n)
    s_model = ms.top_cell_share(r.lmssq_stft_ref(x, win, n, delta=delta)[2], n)
    s_lm = ms.top_cell_share(up.lmssq_stft(x, win, n_fft=n)[0], n)
    s_2 = ms.top_cell_share(up.ssq_stft2(x, win, n_fft=n)[0], n)
    print("top-cell share at delta %d: lmssq_stft %.4f (model %.4f), ssq_stft2 %.4f" % (delta, s_lm, s_model, s_2))
    assert s_lm >= s_model - 0.01
    assert s_lm > s_2


@DTYPES
def test_degenerate_inputs(rdt):
    N, n = 500, 64
    F = n // 2 + 1
    win = window(n)
    kw = dict(n_fft=n, hop_len=3, get_bins=True)
    eps = np.finfo(rdt).eps
    Tx, Sx, _, _, bins = up.lmssq_stft(np.zeros(N, dtype=rdt), win, **kw)
    assert not Tx.any() and not Sx.any() and (bins == -1).all()
    Tx, Sx, _, _, bins = up.lmssq_stft(np.full(N, 3.0, dtype=rdt), win, **kw)
    assert np.isfinite(Tx.view(rdt)).all() and Tx.any()
    assert (bins[np.abs(Sx) < 5 * eps] == -1).all() and (bins[np.abs(Sx) > 20 * eps] >= 0).all() and bins.max() < F
    kept = bins >= 0
    assert np.array_equal(bins[kept], r.stft_bins(Sx, up.lmsst_default_delta(win, n))[kept])
    for delta in (1, F - 1):                                                   # a one-sample signal: one column
        Tx, Sx, _, _, bins = up.lmssq_stft(np.array([3.0], dtype=rdt), win, n_fft=n, delta=delta, get_bins=True)
        assert Tx.shape == bins.shape == (F, 1) and np.isfinite(Tx.view(rdt)).all() and Tx.any()
        assert bins.max() < F and np.array_equal(bins[bins >= 0], r.stft_bins(Sx, delta)[bins >= 0])
        dw = rdt(np.linspace(0, .5, F)[1])
        assert np.abs(Tx - ms.scatter(Sx, bins, dw)).max() <= 4 * eps * float(dw) * np.abs(Sx).sum()
    x = two_chirps(N, 2).astype(rdt)
    Tx, Sx, _, _, bins = up.lmssq_stft(x, win, gamma=1e6, **kw)
    assert np.abs(Sx).max() < 1e6 and not Tx.any() and (bins == -1).all()


@DTYPES
def test_device_door_equals_the_host_call(rdt):
    """`ssq_lmssq_stft_exec` on buffers from `ssq_dev_malloc`, a workspace of exactly `ssq_lmssq_stft_workspace_bytes`
    (none for float64), against the host door bit for bit; `kernel_ms` is one positive float."""
    from tests.test_gpu_grid_limits import Door
    lib = _lib.load()
    N, n, hop, pad, kw = CASES[2]
    F, nfr = n // 2 + 1, (N - 1) // hop + 1
    X = np.stack([two_chirps(N, s) for s in (21, 22)]).astype(rdt)
    win = window(n)
    delta = delta_of(2, "default")
    host = up.lmssq_stft(X, win, n_fft=n, hop_len=hop, fs=FS, padtype=pad, delta=delta, get_bins=True, **kw)
    code = _lib.SSQ_F32 if rdt == np.float32 else _lib.SSQ_F64
    cdt = np.complex64 if rdt == np.float32 else np.complex128
    cells = 2 * F * nfr
    ws = int(lib.ssq_lmssq_stft_workspace_bytes(code, 2, N, n, hop))
    assert ws == (8 * 2 * N if rdt == np.float32 else 0)
    ms_ = C.c_float(-1.0)
    with Door() as d:
        dx, dT, dS, db = d.buf(X.nbytes, X), d.buf(cells * np.dtype(cdt).itemsize), d.buf(cells * np.dtype(cdt).itemsize), \
            d.buf(cells * 4)
        dws = d.buf(ws) if ws else None
        _lib.check(lib.ssq_lmssq_stft_exec(code, dx.p, 2, N, win.ctypes.data_as(C.c_void_p), n, hop, FS, up.PAD_MODES[pad], 0,
                                           -1.0, up._variant(True, True), delta, dT.p, dS.p, db.p, dws.p if dws else None, ws,
                                           C.byref(ms_)))
        got = [dT.get((2, F, nfr), cdt), dS.get((2, F, nfr), cdt), db.get((2, F, nfr), np.int32)]
    for k, (a, b) in enumerate(zip(got, (host[0], host[1], host[4]))):
        assert np.array_equal(a, b), k
    assert 0.0 < ms_.value < 1e4
