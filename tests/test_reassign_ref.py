"""The numpy model of the reassigned spectrogram (tests/helpers/reassign_ref.py) against the facts it is built on: energy
is conserved, an impulse's bins all name the impulse's own column and a tone's its own row, no time target is further
than H = ceil(n / (2 hop)) frames away, and the concentration table of DESIGN 4.14.  CPU only."""
import numpy as np
import pytest

from tests.helpers import reassign_ref as m
from tests.helpers import sst2_ref as s
from tests.helpers import tsst_ref as ts

N, NFFT, SIGMA = 1024, 256, 16
F = NFFT // 2 + 1
IMPULSES = (300, 500, 800)
TONE_ROW = 64                                # 0.25 cycles/sample


def dilate(mask):
    """The cells within +-1 cell (row and column) of a cell of `mask`."""
    out = np.zeros_like(mask)
    R, Ccols = mask.shape
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            out[max(a, 0):R + min(a, 0), max(b, 0):Ccols + min(b, 0)] |= mask[max(-a, 0):R + min(-a, 0),
                                                                            max(-b, 0):Ccols + min(-b, 0)]
    return out


def chirp_mask():
    """The chirp's own bin of every frame: row rint(n f(m)) of column m."""
    _, fi = s.chirp(N, 0.05, 0.45)
    mask = np.zeros((F, N), dtype=bool)
    mask[np.rint(fi * NFFT).astype(int), np.arange(N)] = True
    return mask


def impulse_mask():
    mask = np.zeros((F, N), dtype=bool)
    mask[:, list(IMPULSES)] = True
    return mask


def tone_mask():
    mask = np.zeros((F, N), dtype=bool)
    mask[TONE_ROW] = True
    return mask


def share(P, mask, interior=False):
    """Share of the energy map P on `mask`; interior: on the frames whose window lies inside the signal (away from the
    padding, which is not a chirp or a tone)."""
    cols = slice(NFFT // 2, N - NFFT // 2) if interior else slice(None)
    P = np.asarray(P, dtype=np.float64)
    return (P * mask)[:, cols].sum() / P[:, cols].sum()


def signals():
    xc, _ = s.chirp(N, 0.05, 0.45)
    return dict(chirp=xc, impulses=ts.impulses(N, IMPULSES), tone=np.cos(2 * np.pi * 0.25 * np.arange(N)),
                both=xc + ts.impulses(N, IMPULSES, 8.0))


# (signal, mask, interior frames only, share of the reassigned energy, the same share of |Sx|^2 or None): DESIGN 4.14
TABLE = [
    ("chirp", lambda: chirp_mask(), True, 0.965, 0.186),
    ("chirp", lambda: dilate(chirp_mask()), True, 1.000, None),
    ("impulses", lambda: impulse_mask(), False, 1.000, 0.035),
    ("tone", lambda: tone_mask(), True, 1.000, None),
    ("both", lambda: dilate(chirp_mask() | impulse_mask()), False, 0.971, 0.438),
]


def table_shares(transform):
    """[(reassigned share, |Sx|^2 share)] of TABLE's rows; transform(x) -> (Rx, Sx)."""
    sig = signals()
    maps = {name: transform(x) for name, x in sig.items()}
    return [(share(maps[name][0], mask(), inner), share(np.abs(maps[name][1]) ** 2, mask(), inner))
            for name, mask, inner, _, _ in TABLE]


def model_maps(x):
    out = m.reassign_ref(x, s.gauss_window(NFFT, SIGMA), NFFT)
    return out[5], out[0]


@pytest.mark.parametrize("hop,pad,modulated,dtype", [(1, "reflect", True, np.complex128), (3, "zero", False, np.complex128),
                                                     (64, "wrap", True, np.complex128)])
def test_energy_identity(hop, pad, modulated, dtype):
    x = signals()["both"]
    V, w, tau, kk, tgt, Rx = m.reassign_ref(x, s.gauss_window(NFFT, SIGMA), NFFT, hop_len=hop, padtype=pad,
                                            modulated=modulated, dtype=dtype)
    kept = (np.abs(V) ** 2)[kk >= 0].sum()
    err = abs(Rx.sum() - kept) / kept
    print("sum Rx against the kept energy: %.3g" % err)
    assert Rx.dtype == np.float64 and (Rx >= 0).all()
    assert err <= 1e-14


@pytest.mark.parametrize("arith", ["fft", "dft"])
def test_an_isolated_impulse_puts_all_kept_energy_on_its_own_column(arith):
    n, t0 = 128, 333
    V, w, tau, kk, tgt, Rx = m.reassign_ref(ts.impulses(700, [t0]), s.gauss_window(n, n / 10.0), n, arith=arith)
    keep = kk >= 0
    assert keep.sum() >= 65 * 100 and (tgt[keep] == t0).all()
    assert (kk[keep] == np.nonzero(keep)[0]).all()                       # |V| does not depend on the row: no frequency move
    assert not np.delete(Rx, t0, axis=1).any() and Rx[:, t0].sum() > 0


def test_a_tone_puts_all_kept_energy_on_its_own_row():
    x = signals()["tone"]
    V, w, tau, kk, tgt, Rx = m.reassign_ref(x, s.gauss_window(NFFT, SIGMA), NFFT, padtype="wrap")     # 256 periods: no seam
    # (bins that hold nothing but the transform's rounding noise, 1e-14 of the peak, are kept too and point anywhere)
    big = np.abs(V) >= 1e-6 * np.abs(V).max()
    off = 1 - Rx[TONE_ROW].sum() / Rx.sum()
    print("strong bins %d, share off the tone's row %.3g" % (big.sum(), off))
    assert big.sum() >= 5 * N and (kk[big] == TONE_ROW).all()
    assert off <= 1e-12


def test_concentration_table():
    got = table_shares(model_maps)
    for (name, _, inner, want_r, want_s), (sr, ss) in zip(TABLE, got):
        print("%-8s reassigned %.4f (table %.3f)   |Sx|^2 %.4f (table %s)" % (name, sr, want_r, ss, want_s))
        assert abs(sr - want_r) <= 5e-4
        if want_s is not None:
            assert abs(ss - want_s) <= 5e-4


@pytest.mark.parametrize("n,hop", [(16, 1), (64, 3), (256, 1), (256, 100), (1024, 7), (64, 64)])
def test_no_time_target_is_further_than_the_reach(n, hop):
    x = signals()["both"] + 1e-3 * np.random.default_rng(0).standard_normal(N)
    V, w, tau, kk, tgt, _ = m.reassign_ref(x, s.gauss_window(n, n / 10.0), n, hop_len=hop, fs=250.0, squeeze=False)
    keep = kk >= 0
    H = -(-n // (2 * hop))
    r = (tgt - np.arange(V.shape[1])[None, :])[keep]
    print("H %d, max |r| %d" % (H, np.abs(r).max()))
    assert np.abs(r).max() <= H
    assert (kk[keep] >= 0).all() and (kk[keep] <= n // 2).all()
