"""The numpy model of the synchroextracting and transient-extracting CWT (tests/helpers/extract_cwt_ref.py) against the
facts it is built on: the share of a chirp's extracted energy on its own row (second order against first), a
tone coming back from the one row SET keeps, an impulse kept on its own column, a fast chirp kept where it crosses each
row, and the rules on their own.  CPU only.  The pinned figures are the model's own, to three digits.

The set-up: GMW(3, 60), 127 log scales at 32 to the octave whose rows run from 0.45 down to 0.029 cycles/sample, N = 1024,
float64, dt = 1."""
import numpy as np
import pytest

from tests.helpers import cwt_sst2_ref as c2
from tests.helpers import extract_cwt_ref as m
from tests.helpers import tssq_cwt_ref as tc

GMW = ("gmw", 3.0, 60.0)
N, NA, NV = 1024, 127, 32
NU = 0.45 * 2.0 ** (-np.arange(NA) / NV)                  # the rows' frequencies, cycles/sample
SCALES = c2.gmw_wc(3.0, 60.0) / (2 * np.pi * NU)
COLS = np.arange(128, 896)
TONE_ROW, TONE_PHASE = 40, 0.3
T0 = 400                                                   # the impulse's sample
NC, CROSS = 512, (64, 447)                                 # TET's chirp: 0.02 -> 0.45 over 512 samples; the rows it crosses here
# the model's values (printed by the tests below), by order
CHIRP_SHARE = {2: 1.000, 1: 0.882}                        # own-row share of |Te|^2 on COLS (order 2: 0.9999998)
CHIRP_KEPT = {2: 1.000, 1: 1.155}                         # kept cells with |W| >= 1e-2 max per column of COLS
TONE_ERR = {2: 6.11e-6, 1: 7.29e-4}                       # relative L2 error of Re sum_i Te[i, j] on COLS
TONE_ROWS = {2: [TONE_ROW], 1: [TONE_ROW] + list(range(115, 127))}    # rows kept above 1e-3 of the maximum on COLS
IMPULSE_SHARE = {1: 0.9988, 2: 0.9996}                    # kept energy on column T0, padtype='zero'
CROSS_SHARE = {2: 0.992, 1: 0.265}                        # kept energy within one column of the crossing


def chirp():
    return c2.chirp(N, 0.05, 0.40)


def strong(W, level=1e-2):
    return np.abs(W) >= level * np.abs(W).max()


def own_row_share(Te, cols=COLS):
    """Share of |Te|^2 of the columns `cols` on the row nearest in log frequency to the chirp's instantaneous frequency."""
    _, fi = chirp()
    own = np.abs(np.log(NU)[:, None] - np.log(fi[cols])[None, :]).argmin(0)
    P = np.abs(Te[:, cols]) ** 2
    return P[own, np.arange(len(cols))].sum() / P.sum()


def tone():
    return np.cos(2 * np.pi * NU[TONE_ROW] * np.arange(N) + TONE_PHASE)


def tone_error(Te, cols=COLS):
    x = tone()
    return np.linalg.norm(Te.sum(0).real[cols] - x[cols]) / np.linalg.norm(x[cols])


def impulse():
    x = np.zeros(N)
    x[T0] = 1.0
    return x


def column_share(Te, col=T0):
    E = np.abs(Te) ** 2
    return E[:, col].sum() / E.sum()


def crossing_chirp():
    return c2.chirp(NC, 0.02, 0.45)[0]


def crossing_share(Te):
    """Share of |Te|^2, over the rows the chirp crosses on columns CROSS, within one column of the crossing."""
    E = np.abs(Te) ** 2
    cross = (NU - 0.02) / ((0.45 - 0.02) / NC)
    near = total = 0.0
    for i in np.nonzero((cross >= CROSS[0]) & (cross <= CROSS[1]))[0]:
        c = int(np.rint(cross[i]))
        near += E[i, c - 1:c + 2].sum()
        total += E[i].sum()
    return near / total


def test_the_rows_are_the_stated_ones():
    assert np.allclose(tc.row_freqs(GMW, SCALES), NU, rtol=1e-15, atol=0)
    assert NU[0] == 0.45 and abs(NU[-1] - 0.029) < 5e-4


@pytest.mark.parametrize("order", [2, 1])
def test_chirp_concentration(order):
    x, _ = chirp()
    Te, W, w, keep = m.set_cwt_ref(x, GMW, SCALES, order=order)
    share = own_row_share(Te)
    ks = (keep & strong(W))[:, COLS].sum(0)
    print("order %d: own-row share %.7f, kept strong cells per column %.4f (%d .. %d)" % (order, share, ks.mean(), ks.min(), ks.max()))
    assert abs(share - CHIRP_SHARE[order]) <= 5e-4
    assert abs(ks.mean() / CHIRP_KEPT[order] - 1) <= 5e-4
    if order == 2:
        assert (ks == 1).all()                                  # exactly one strong cell a column


@pytest.mark.parametrize("order", [1, 2])
def test_a_tone_comes_back_from_the_row_that_is_kept(order):
    Te, W, w, keep = m.set_cwt_ref(tone(), GMW, SCALES, order=order)
    err = tone_error(Te)
    rows = np.unique(np.nonzero((keep & strong(W, 1e-3))[:, COLS])[0]).tolist()
    print("order %d: relative L2 error %.3e, rows kept above 1e-3 of the maximum: %s" % (order, err, rows))
    assert rows == TONE_ROWS[order]
    assert (keep & strong(W, 1e-3))[TONE_ROW][COLS].all()
    assert abs(err / TONE_ERR[order] - 1) <= 5e-3
    if order == 2:
        assert err <= 1e-5                                       # the identity itself


@pytest.mark.parametrize("order", [1, 2])
def test_an_impulse_is_kept_on_its_own_column(order):
    Te, W, tau, keep = m.tet_cwt_ref(impulse(), GMW, SCALES, padtype="zero", order=order)
    share = column_share(Te)
    print("order %d: %.6f of the kept energy on column %d, %d rows kept there" % (order, share, T0, keep[:, T0].sum()))
    assert keep[:, T0].all()
    assert abs(share - IMPULSE_SHARE[order]) <= 5e-5
    assert np.array_equal(Te[:, T0], W[:, T0])


@pytest.mark.parametrize("order", [2, 1])
def test_a_fast_chirp_is_kept_where_it_crosses_a_row(order):
    Te, W, tau, keep = m.tet_cwt_ref(crossing_chirp(), GMW, SCALES, order=order)
    share = crossing_share(Te)
    print("order %d: %.4f of the kept energy within one column of the crossing" % (order, share))
    assert abs(share - CROSS_SHARE[order]) <= 5e-4


def test_second_order_stays_on_the_ridge_where_first_order_does_not():
    x, _ = chirp()
    s1, s2 = (own_row_share(m.set_cwt_ref(x, GMW, SCALES, order=o)[0]) for o in (1, 2))
    c1, c2_ = (crossing_share(m.tet_cwt_ref(crossing_chirp(), GMW, SCALES, order=o)[0]) for o in (1, 2))
    assert s2 > 0.9999 and s1 < 0.9 and c2_ > 0.99 and c1 < 0.3


@pytest.mark.parametrize("order", [1, 2])
def test_set_is_built_on_the_parents_map(order):
    """w is `cwt_sst2_ref`'s w2 (order 2) or its w1 under the live rule (order 1); Te is W where kept and +0 elsewhere."""
    x = chirp()[0] + impulse() * 8.0
    f_asc = c2.log_freqs(N, NA)
    W2, w2, _, _, d = c2.cwt_sst2_ref(x, GMW, SCALES, f_asc, "log", details=True)
    Te, W, w, keep = m.set_cwt_ref(x, GMW, SCALES, order=order)
    assert np.array_equal(W, W2)
    assert np.array_equal(w, w2 if order == 2 else np.where(np.isinf(w2), np.inf, d["w1"]))
    assert keep.any() and not keep.all()
    assert np.array_equal(Te, np.where(keep, W, 0))
    assert not np.signbit(Te[~keep].real).any() and not np.signbit(Te[~keep].imag).any()


@pytest.mark.parametrize("order", [1, 2])
def test_tet_is_built_on_the_parents_map(order):
    x = chirp()[0] + impulse() * 8.0
    Wp, taup, mm, _ = tc.tssq_cwt_ref(x, GMW, SCALES, order=order, squeeze=False)
    Te, W, tau, keep = m.tet_cwt_ref(x, GMW, SCALES, order=order)
    assert np.array_equal(W, Wp) and np.array_equal(tau, taup)
    inside = np.ones((NA, N), dtype=bool)
    inside[:, [0, N - 1]] = False                               # (where the parent's clip cannot act)
    assert np.array_equal(keep[inside], (mm == np.arange(N)[None, :])[inside])
    assert np.array_equal(Te, np.where(keep, W, 0))


@pytest.mark.parametrize("order", [1, 2])
def test_the_restatement_in_one_dtype_is_the_parents_models_in_complex128(order):
    """`maps_in` exists for its complex64 run; in complex128 it must be the models the rest is built on, bit for bit."""
    x = chirp()[0] + impulse() * 8.0
    W, w, tau = m.maps_in(x, GMW, SCALES, np.complex128, dt=0.5, padtype="symmetric", order=order)
    _, Ws, ws, _ = m.set_cwt_ref(x, GMW, SCALES, dt=0.5, padtype="symmetric", order=order)
    _, Wt, taut, _ = m.tet_cwt_ref(x, GMW, SCALES, dt=0.5, padtype="symmetric", order=order)
    assert np.array_equal(W, Ws) and np.array_equal(w, ws, equal_nan=True)
    if order == 2:                                              # (order 1 of `tssq_cwt_ref` transforms W and Wt alone)
        assert np.array_equal(W, Wt)
    big = strong(W)
    assert np.allclose(tau[big], taut[big], rtol=1e-9, atol=1e-9) and np.array_equal(np.isposinf(tau), np.isposinf(taut))
    if order == 2:
        assert np.array_equal(tau, taut, equal_nan=True)
    W4, w4, tau4 = m.maps_in(x, GMW, SCALES, np.complex64, dt=0.5, padtype="symmetric", order=order)
    assert W4.dtype == np.complex64 and w4.dtype == tau4.dtype == np.float32
    assert 1e-8 < np.abs(W4 - W).max() / np.abs(W).max() < 1e-5


@pytest.mark.parametrize("order", [1, 2])
def test_tet_does_not_keep_an_edge_cell_that_the_clip_would_bring_back(order):
    """padtype='wrap' and an impulse on sample 0: the last column sees it one sample AHEAD, behind the signal's end.
    `tssq_cwt_ref` clips that target back onto the last column, the relative target before the clip is 1, not 0."""
    x = np.zeros(N)
    x[0] = 1.0
    Te, W, tau, keep = m.tet_cwt_ref(x, GMW, SCALES, padtype="wrap", order=order)
    mm = tc.tssq_cwt_ref(x, GMW, SCALES, padtype="wrap", order=order, squeeze=False)[2]
    seen = np.abs(W[:, N - 1]) > 1e-6
    assert seen.sum() > NA // 2 and (mm[seen, N - 1] == N - 1).all()       # tssq_cwt leaves them where they are
    assert np.allclose(tau[seen, N - 1], 1.0, atol=0.25)
    assert not keep[seen, N - 1].any()                                    # tet_cwt does not keep them


def test_row_edges():
    e = m.row_edges(GMW, SCALES, dt=0.5)
    assert e.dtype == np.float64 and e.shape == (NA + 1,) and e[0] == np.inf and e[-1] == 0
    nu = tc.row_freqs(GMW, SCALES)
    assert np.array_equal(e[1:-1], np.sqrt(nu[:-1] * nu[1:]) / 0.5) and (np.diff(e) < 0).all()
    assert ((e[1:-1] < 2 * nu[:-1]) & (e[1:-1] > 2 * nu[1:])).all()
    for bad in (SCALES[::-1], np.array([4.0, 4.0, 5.0])):
        with pytest.raises(ValueError):
            m.row_edges(GMW, bad)


def test_the_rules_alone():
    e = np.array([np.inf, 4.0, 2.0, 0.0])                                  # three rows
    row = lambda v: m.keep_freq(np.full((3, 1), v, dtype=np.float32), e)[:, 0].tolist()      # noqa: E731
    assert row(4.0) == [True, False, False]                    # a cell on an edge goes to the higher-frequency row
    assert row(2.0) == [False, True, False]
    assert row(np.nextafter(np.float32(4.0), np.float32(0))) == [False, True, False]
    assert row(1e30) == [True, False, False] and row(0.0) == [False, False, True]           # the outer rows are open-ended
    assert row(np.nan) == [False] * 3 and row(np.inf) == [False] * 3                        # NaN and a dead cell: nowhere
    # the edges are rounded to the map's dtype before the comparison: 4 (1 + 2^-30) is 4 in float32
    e2 = np.array([np.inf, 4.0 * (1 + 2.0 ** -30), 2.0, 0.0])
    assert m.keep_freq(np.full((3, 1), 4.0, dtype=np.float32), e2)[:, 0].tolist() == [True, False, False]
    assert m.keep_freq(np.full((3, 1), 4.0, dtype=np.float64), e2)[:, 0].tolist() == [False, True, False]
    w = np.array([[5.0, 3.0], [3.0, 1.0]])                                 # batched maps broadcast over the rows
    assert m.keep_freq(np.stack([w, w]), np.array([np.inf, 2.0, 0.0])).tolist() == [[[True, True], [False, True]]] * 2
    tau = np.array([[0.0, 0.24, -0.25, 0.26, np.inf, np.nan, -np.inf]])    # dt = 0.5: ties to even
    assert m.keep_time(tau, 0.5).tolist() == [[True, True, True, False, False, False, False]]
    W = np.array([[1 + 2j, -3j]], dtype=np.complex64)
    out = m.extract(W, np.array([[True, False]]))
    assert out.dtype == np.complex64 and out.tolist() == [[1 + 2j, 0j]] and not np.signbit(out[0, 1].imag)
