"""GPU component inversion (`upstream.issq_cwt` / `issq_stft` with `cc`, `cw`; issq_components.hip) against the NumPy
restatement tests/helpers/components_ref.py, batched against the per-signal loop, the device-pointer chain from
`ssq_ridges_exec`, and the separation of a tone and a chirp end to end."""
import ctypes as C

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.helpers import components_ref as cr

pytestmark = pytest.mark.gpu


def _random_tx(rng, F, N, dt, B=None):
    shape = (F, N) if B is None else (B, F, N)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dt)


def _random_curves(rng, F, N, K):
    """Centres across and beyond the rows, with -1, -5 and F + 3 planted, half-widths 0 .. 9 and some negative:
    bands overlap, clip at both ends, vanish."""
    cc = rng.integers(-8, F + 8, size=(N, K))
    cc[rng.random((N, K)) < 0.15] = -1
    cc[rng.random((N, K)) < 0.05] = -5
    cc[rng.random((N, K)) < 0.05] = F + 3
    cw = rng.integers(-2, 10, size=(N, K))
    cw[rng.random((N, K)) < 0.1] = 0
    return cc, cw


def _check(got, want, Tx):
    """fp64 and fp32 components: 1e-12 of max|x| (fp64 sums in another order); the fp32 remainder 1e-5 (upstream sums
    it in fp32)."""
    assert got.shape == want.shape and got.dtype == np.float64
    tol = 1e-12 * np.abs(want).max()
    assert np.abs(got[:-1] - want[:-1]).max() <= tol
    rtol = 1e-5 if Tx.dtype == np.complex64 else 1e-12
    assert np.abs(got[-1] - want[-1]).max() <= rtol * np.abs(want).max()


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
@pytest.mark.parametrize("K", [1, 3, 8, 9, 40])
@pytest.mark.parametrize("N", [300, 257])
def test_mirror_matches_the_restatement(dt, K, N):
    rng = np.random.default_rng(K * 1000 + N)
    F = 65
    Tx = _random_tx(rng, F, N, dt)
    cc, cw = _random_curves(rng, F, N, K)
    got = up.issq_cwt(Tx, "gmw", cc=cc, cw=cw)
    _check(got, cr.issq_cwt(Tx, cc, cw, up.adm_ssq("gmw")), Tx)
    win = np.hanning(2 * (F - 1)) + 0.05
    got = up.issq_stft(Tx, win, cc=cc, cw=cw)
    _check(got, cr.issq_stft(Tx, cc, cw, win), Tx)


@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
def test_edge_curves_and_input_forms(dt):
    rng = np.random.default_rng(7)
    F, N = 300, 96                                        # F > 32 rows per wave: several waves split the rows
    Tx = _random_tx(rng, F, N, dt)
    adm = up.adm_ssq(("morlet", {"mu": 6.0}))
    cases = [
        (np.full(N, -1), np.full(N, 4)),                   # no curve anywhere: all remainder
        (np.full(N, -5), np.full(N, 2)),                   # row 0 only
        (np.full(N, F + 2), np.full(N, 1)),                # beyond the rows: empty
        (np.full(N, F), np.full(N, 1)),                    # the last row only
        (np.arange(N) % F, np.zeros(N, dtype=int)),        # cw = 0
        (rng.uniform(-3, F + 3, N), rng.uniform(-1, 12, N)),   # floats truncate; 1-D is one curve
        (rng.integers(0, F, (N, 3)), rng.integers(0, 40, (N, 5))),   # cw with extra columns
        (rng.integers(0, F, (N, 2)), rng.integers(0, 40, (1, 2))),   # cw broadcast over the columns
    ]
    for cc, cw in cases:
        got = up.issq_cwt(Tx, ("morlet", {"mu": 6.0}), cc=cc, cw=cw)
        _check(got, cr.issq_cwt(Tx, cc, cw, adm), Tx)


def test_fp32_wide_loads_equal_the_narrow_path():
    """fp32 with an even N and enough columns reads two columns per lane; an odd N reads one.  Same sums, same bits."""
    rng = np.random.default_rng(9)
    F, N = 40, 1 << 16
    Tx = _random_tx(rng, F, N + 1, np.complex64)
    cc, cw = _random_curves(rng, F, N + 1, 3)
    wide = up.issq_cwt(np.ascontiguousarray(Tx[:, :N]), "gmw", cc=cc[:N], cw=cw[:N])
    narrow = up.issq_cwt(Tx, "gmw", cc=cc, cw=cw)
    assert np.array_equal(wide, narrow[:, :N])
    _check(wide, cr.issq_cwt(Tx[:, :N], cc[:N], cw[:N], up.adm_ssq("gmw")), Tx)


def test_batch_equals_the_per_signal_loop():
    rng = np.random.default_rng(13)
    N = 512
    x = rng.standard_normal((3, N))
    scales = 2 ** (np.arange(64) / 16 + 1)
    Tx = up.ssq_cwt(x, "gmw", scales=scales)[0]
    assert Tx.shape == (3, 64, N)
    ridges = up.extract_ridges(Tx, scales, penalty=2, n_ridges=3, bw=4)
    assert ridges.shape == (3, N, 3)
    cw = np.full_like(ridges, 4)
    xb = up.issq_cwt(Tx, "gmw", cc=ridges, cw=cw)
    assert xb.shape == (3, 4, N) and xb.dtype == np.float64
    for b in range(3):
        assert np.array_equal(xb[b], up.issq_cwt(Tx[b], "gmw", cc=ridges[b], cw=cw[b]))
    xs = up.issq_stft(Tx, np.hanning(126) + 0.1, cc=ridges[:, :, 0], cw=np.full((3, N), 2))
    for b in range(3):
        assert np.array_equal(xs[b], up.issq_stft(Tx[b], np.hanning(126) + 0.1, cc=ridges[b, :, 0], cw=np.full(N, 2)))


def _ok(rc):
    _lib.check(rc)


def test_device_chain_from_ridges_equals_the_host_path():
    lib = _lib.load()
    rng = np.random.default_rng(17)
    N = 1024
    scales = 2 ** (np.arange(96) / 24 + 1)
    Tx = up.ssq_cwt(rng.standard_normal(N), "gmw", scales=scales)[0]
    F, K, bw, cw = Tx.shape[0], 2, 5.0, 6
    scale = 2.0 / up.adm_ssq("gmw")
    metric = np.ascontiguousarray(np.log(scales))
    ptrs = []

    def alloc(n):
        p = C.c_void_p()
        _ok(lib.ssq_dev_malloc(C.byref(p), int(n)))
        ptrs.append(p)
        return p
    st = C.c_void_p()
    _ok(lib.ssq_stream_create(C.byref(st)))
    try:
        dT, dm, di = alloc(Tx.nbytes), alloc(metric.nbytes), alloc(8 * N * K)
        dx = alloc(8 * (K + 1) * N)
        wsb = lib.ssq_ridges_workspace_bytes(_lib.SSQ_F64, 1, F, N)
        dw = alloc(wsb)
        _ok(lib.ssq_memcpy_h2d(dT, Tx.ctypes.data_as(C.c_void_p), Tx.nbytes, st))
        _ok(lib.ssq_memcpy_h2d(dm, metric.ctypes.data_as(C.c_void_p), metric.nbytes, st))
        _ok(lib.ssq_ridges_exec(_lib.SSQ_F64, _lib.SSQ_F64, 1, dT, 1, F, N, dm, None, 2.0, K, bw, di, None, None, None,
                                dw, wsb, st))
        _ok(lib.ssq_issq_components_exec(_lib.SSQ_F64, dT, 1, F, N, di, None, cw, K, scale, dx, st))
        x = np.empty((K + 1, N))
        ridges = np.empty((N, K), dtype=np.int64)
        _ok(lib.ssq_memcpy_d2h(x.ctypes.data_as(C.c_void_p), dx, x.nbytes, st))
        _ok(lib.ssq_memcpy_d2h(ridges.ctypes.data_as(C.c_void_p), di, ridges.nbytes, st))
        _ok(lib.ssq_stream_sync(st))
    finally:
        for p in ptrs:
            lib.ssq_dev_free(p)
        lib.ssq_stream_destroy(st)
    want_r = up.extract_ridges(Tx, scales, penalty=2.0, n_ridges=K, bw=bw)
    assert np.array_equal(ridges, want_r)
    assert np.array_equal(x, up.issq_cwt(Tx, "gmw", cc=want_r, cw=np.full_like(want_r, cw)))


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_separates_a_tone_and_a_chirp(dt):
    N = 2048
    t = np.arange(N) / N
    x1 = np.cos(2 * np.pi * 40 * t)
    x2 = 0.7 * np.cos(2 * np.pi * (150 * t + 60 * t ** 2))
    scales = 2 ** (np.arange(224) / 32)
    Tx = up.ssq_cwt((x1 + x2).astype(dt), "gmw", scales=scales)[0]
    ridges = up.extract_ridges(Tx, scales, penalty=2, n_ridges=2, bw=8)
    comps = up.issq_cwt(Tx, "gmw", cc=ridges, cw=np.full_like(ridges, 8))
    assert comps.shape == (3, N) and comps.dtype == np.float64
    sl = slice(100, N - 100)
    for truth in (x1, x2):
        err = min(np.sqrt(np.mean((c[sl] - truth[sl]) ** 2)) / np.sqrt(np.mean(truth[sl] ** 2)) for c in comps[:2])
        assert err < 0.01, err
    full = up.issq_cwt(Tx, "gmw")
    tol = (1e-12 if dt == np.float64 else 1e-6) * np.abs(full).max()   # fp32: the full inverse is rounded to fp32
    assert np.abs(comps.sum(axis=0) - full).max() <= tol
