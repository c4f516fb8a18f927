"""The numpy model of the synchroextracting and transient-extracting STFT (tests/helpers/extract_ref.py) against the facts
it is built on: the share of a fast chirp's extracted energy on its own bin (second order against first), the identity of
a tone on a bin centre that stands in for an inverse, an isolated impulse kept on its own column only, and SET as the rows
of `sst2_ref`'s scatter that did not move.  CPU only.  The pinned figures are the model's own, to three digits."""
import numpy as np
import pytest

from tests.helpers import extract_ref as m
from tests.helpers import sst2_ref as s
from tests.helpers import tsst_ref as ts

N, NFFT, SIGMA = 1024, 256, 24
COLS = np.arange(128, 896)
TONE_BIN, TONE_PHASE = 37, 0.3
IMPULSES = (300, 800)
# the model's values (printed by the tests below): own-bin share and kept cells per column of the chirp, by order
CHIRP_SHARE = {2: 0.937, 1: 0.369}
CHIRP_KEPT = {2: 8.46, 1: 14.4}
# relative L2 error of the tone identity on COLS, by order
TONE_ERR = {1: 4.80e-9, 2: 9.70e-8}


def chirp():
    return s.chirp(N, 0.05, 0.45)


def own_bin_share(Te, n=NFFT, cols=COLS):
    """Share of |Te|^2 of the columns `cols` on the bin nearest the chirp's instantaneous frequency."""
    _, fi = chirp()
    own = np.rint(fi[cols] * n).astype(int)
    P = np.abs(Te[:, cols]) ** 2
    return P[own, np.arange(len(cols))].sum() / P.sum()


def tone():
    return np.cos(2 * np.pi * TONE_BIN * np.arange(N) / NFFT + TONE_PHASE)


def tone_error(Te, win, cols=COLS):
    x = tone()
    return np.linalg.norm(m.tone_identity(Te, win)[cols] - x[cols]) / np.linalg.norm(x[cols])


@pytest.mark.parametrize("order", [2, 1])
def test_chirp_concentration(order):
    x, _ = chirp()
    Te, V, w, keep = m.set_ref(x, s.gauss_window(NFFT, SIGMA), NFFT, order=order)
    share, kept = own_bin_share(Te), keep[:, COLS].sum(0).mean()
    print("order %d: own-bin share %.4f, kept cells per column %.3f of %d" % (order, share, kept, V.shape[0]))
    assert abs(share - CHIRP_SHARE[order]) <= 5e-4
    assert abs(kept / CHIRP_KEPT[order] - 1) <= 5e-3


def test_second_order_stays_on_the_ridge_where_first_order_does_not():
    x, _ = chirp()
    win = s.gauss_window(NFFT, SIGMA)
    s1, s2 = (own_bin_share(m.set_ref(x, win, NFFT, order=o)[0]) for o in (1, 2))
    assert s2 >= 0.9 and s1 <= 0.5


@pytest.mark.parametrize("order", [1, 2])
def test_tone_identity_on_a_bin_centre(order):
    win = s.gauss_window(NFFT, SIGMA)
    Te, V, w, keep = m.set_ref(tone(), win, NFFT, order=order)
    err = tone_error(Te, win)
    strong = np.abs(V) >= 1e-6 * np.abs(V).max()
    print("order %d: relative L2 error %.3e" % (order, err))
    ks = (keep & strong)[:, COLS]
    assert (np.nonzero(ks)[0] == TONE_BIN).all() and ks[TONE_BIN].all()
    assert err <= 1e-6                                          # the identity itself
    assert abs(err / TONE_ERR[order] - 1) <= 5e-2               # and the model's own figure


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("hop", [1, 4])
def test_an_isolated_impulse_is_kept_on_its_own_column_only(order, hop):
    win = s.gauss_window(NFFT, SIGMA)
    Te, V, tau, keep = m.tet_ref(ts.impulses(N, IMPULSES), win, NFFT, hop_len=hop, order=order)
    seen = np.abs(V) > 1e-6
    cols = np.unique(np.nonzero(keep & seen)[1])
    print("hop %d, order %d: kept on frames %s" % (hop, order, cols))
    assert cols.tolist() == [t0 // hop for t0 in IMPULSES]
    assert keep[:, cols].all()
    assert np.allclose(np.abs(Te[:, cols]), win[NFFT // 2], rtol=1e-12, atol=0)


@pytest.mark.parametrize("order", [1, 2])
def test_tet_does_not_keep_an_edge_cell_that_the_clip_would_bring_back(order):
    """An impulse behind the last frame's centre by more than half a hop: `tsst_ref` clips its target back onto the last
    frame, the relative target before the clip is 1, not 0."""
    hop = 16
    win = s.gauss_window(NFFT, SIGMA)
    xe = np.zeros(N)
    xe[N - 1] = 1.0                                            # the last frame is centred on (nfr - 1) hop = 1008: 15 samples on
    Te, V, tau, keep = m.tet_ref(xe, win, NFFT, hop_len=hop, padtype="zero", order=order)
    _, _, tgt, _ = ts.tsst_ref(xe, win, NFFT, hop_len=hop, padtype="zero", order=order, squeeze=False)
    last = V.shape[1] - 1
    seen = np.abs(V[:, last]) > 1e-6
    assert seen.any() and (tgt[seen, last] == last).all()       # tssq_stft leaves them where they are
    assert not keep[seen, last].any()                           # tet_stft does not keep them


@pytest.mark.parametrize("hop,pad,modulated", [(1, "reflect", True), (3, "zero", False)])
def test_set_is_the_rows_of_the_scatter_that_did_not_move(hop, pad, modulated):
    x, _ = chirp()
    x = x + ts.impulses(N, IMPULSES, 8.0)
    win = s.gauss_window(NFFT, SIGMA)
    V, w2, kk, _ = s.sst2_ref(x, win, NFFT, hop_len=hop, padtype=pad, modulated=modulated)
    Te, V2, w, keep = m.set_ref(x, win, NFFT, hop_len=hop, padtype=pad, modulated=modulated, order=2)
    rows = np.arange(V.shape[0])[:, None]
    assert np.array_equal(V, V2) and np.array_equal(w, w2)
    assert np.array_equal(keep, kk == rows) and keep.any() and not keep.all()
    assert np.array_equal(Te, np.where(kk == rows, V, 0))
    assert not np.signbit(Te[~keep].real).any() and not np.signbit(Te[~keep].imag).any()


def test_the_rules_alone():
    w = np.array([[0.0, 0.24, np.inf], [0.26, 0.5, 0.74], [1.0, 9.0, np.nan]], dtype=np.float32)     # F = 3, fs = 2: dw = 0.5
    assert m.bins_of(w, 2.0).tolist() == [[0, 0, 2], [1, 1, 1], [2, 2, 0]]
    assert m.keep_freq(w, 2.0).tolist() == [[True, True, False], [True, True, True], [True, True, False]]
    tau = np.array([[0.0, 0.24, -0.25, 0.26, np.inf, np.nan]])                                       # hop / fs = 0.5: ties to even
    assert m.keep_time(tau, 1, 2.0).tolist() == [[True, True, True, False, False, False]]
