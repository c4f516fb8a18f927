"""CPU checks of the numpy model of the reassigned scalogram (tests/helpers/reassign_cwt_ref.py): the facts
the definition rests on, and the concentration table DESIGN 4.15 quotes.  No GPU; the library only where a test says so
(its host-side wavelet tables)."""
import functools

import numpy as np

from tests.helpers import cwt_sst2_ref as c2
from tests.helpers import reassign_cwt_ref as m
from tests.helpers.tsst_ref import impulses

N = 512
GMW = ("gmw", 3.0, 60.0)
SCALES = 2.0 * 2.0 ** (np.arange(180) / 32)               # 180 log scales at nv 32 from 2
FREQS = c2.log_freqs(N, len(SCALES))                      # the 'maximal' log grid, ascending
T_IMP = (128, 256, 384)                                   # the three impulses of the mixed signal


# The transform is circular over the padded length P = 1024: a row whose wavelet is longer than the padding wraps onto
# itself, and Re(Wt/W) then mixes the two images (rows above scale ~ 32 here: DESIGN 4.15).  The impulse identity is
# checked on the scales whose wavelet, down to 1e-6 of the map's peak, fits the padded length.
FIT = 96                                                  # scales 2 ... 15.7


def run(x, padtype="reflect", scales=SCALES, **kw):
    return m.reassign_cwt_ref(x, GMW, scales, c2.log_freqs(N, len(scales)), "log", padtype=padtype, details=True, **kw)


def test_energy_identity():
    for x in (c2.chirp(N, 0.02, 0.45)[0] + impulses(N, T_IMP, 8.0), impulses(N, [200])):
        W, w, tau, kk, mm, Rx, d = run(x)
        kept = m.energy(W)[d["keep"]].sum()
        assert (Rx >= 0).all()
        assert abs(Rx.sum() - kept) <= 1e-12 * kept
        assert np.array_equal(kk == -1, ~d["keep"]) and np.array_equal(mm == -1, ~d["keep"])
        assert np.array_equal(np.isposinf(w), ~d["keep"]) and np.array_equal(np.isposinf(tau), ~d["keep"])


def test_impulse_names_its_own_column():
    """W(b) = k(b - t0) and Wt(b) = (t0 - b) k(b - t0): b + Re(Wt/W) = t0 at every scale.  Every bin with |W| >= 1e-6 max
    names the impulse's column (28597 bins at N = 512, offsets up to 311 samples).  The value of tau is held to 1e-9
    sample on a 64-sample signal: a bin of relative size r at offset d carries a rounding error of about eps d / r in
    fp64 (1.3e-8 at r = 1e-6, d = 59; measured 1.8e-8 ... 6.7e-8 at N = 512 in both of the model's arithmetics), so 1e-9
    is within the format's reach only where no bin inside the signal is that weak; at N = 64, t0 = 32 and scales
    2 ... 2.33 the weakest bin is 5e-3 of the peak and the measured error is 1.1e-11."""
    t0 = 200
    W, w, tau, kk, mm, Rx, d = run(impulses(N, [t0]), padtype="zero", scales=SCALES[:FIT])
    big = np.abs(W) >= 1e-6 * np.abs(W).max()
    assert big.sum() > 20000
    assert (mm[big] == t0).all()
    n, t0 = 64, 32
    W, w, tau, kk, mm, Rx, d = m.reassign_cwt_ref(impulses(n, [t0]), GMW, SCALES[:8], c2.log_freqs(n, 8), "log",
                                                  padtype="zero", details=True)
    big = np.abs(W) >= 1e-6 * np.abs(W).max()
    assert big.all() and (mm == t0).all()
    err = np.abs(tau - (t0 - np.arange(n))[None, :]).max()
    print("tau error %.3g samples" % err)
    assert err <= 1e-9


def test_tone_stays_where_it_is():
    f0 = 0.1
    x = np.cos(2 * np.pi * f0 * np.arange(N))
    W, w, tau, kk, mm, Rx, d = run(x)
    own = int(c2.bin_positions(np.array([f0]), FREQS, "log")[0][0])
    # columns whose wavelet support (taken where the row's response to a centred impulse is above 1e-8 of its peak) lies
    # inside the signal: the reflected tone has a phase jump at either end
    Wi = run(impulses(N, [N // 2]), padtype="zero")[0]
    reach = np.array([np.abs(np.nonzero(np.abs(r) >= 1e-8 * np.abs(r).max())[0] - N // 2).max() for r in Wi])
    j = np.arange(N)[None, :]
    inside = (j >= reach[:, None]) & (j < N - reach[:, None])
    big = (np.abs(W) >= 1e-2 * np.abs(W).max()) & inside
    assert big.sum() > 1000
    assert (kk[big] == own).all()
    assert np.abs(tau[big]).max() < 0.5
    assert (mm[big] == np.broadcast_to(j, W.shape)[big]).all()


def sst1_energy(x):
    """|Tx|^2 of the first-order `ssq_cwt` model: `cwt_sst2_ref`'s W scattered along frequency under its first-order w."""
    W, _, _, _, d = c2.cwt_sst2_ref(x, GMW, SCALES, FREQS, "log", details=True)
    keep = ~(np.abs(W) < 10 * float(np.finfo(np.float64).eps))
    bins, _ = c2.bin_positions(d["w1"], FREQS, "log")
    Tx = np.zeros(W.shape, dtype=np.complex128)
    cols = np.arange(W.shape[1])
    for i in range(W.shape[0]):
        np.add.at(Tx, (bins[i, keep[i]], cols[keep[i]]), W[i, keep[i]])
    return m.energy(Tx)


def chirp_ridge():
    _, fi = c2.chirp(N, 0.02, 0.45)
    return c2.bin_positions(fi, FREQS, "log")[0], np.arange(N)


def impulse_ridge(at):
    na = len(SCALES)
    return np.tile(np.arange(na), len(at)), np.repeat(np.asarray(at), na)


def _mixed_ridge():
    a, b = chirp_ridge(), impulse_ridge(T_IMP)
    return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])


# name, signal, the ridge's cells (rows, columns), the model's shares of the energy within +-1 cell of the ridge:
# (reassigned, first-order SST) -- DESIGN 4.15's table, computed by this module
TABLE = [
    ("impulse", lambda: impulses(N, [200]), lambda: impulse_ridge([200]), (0.93583, 0.08367)),
    ("chirp", lambda: c2.chirp(N, 0.02, 0.45)[0], chirp_ridge, (0.82236, 0.63710)),
    ("mixed", lambda: c2.chirp(N, 0.02, 0.45)[0] + impulses(N, T_IMP, 8.0), _mixed_ridge, (0.65357, 0.37883)),
]


def model_energy(x):
    return run(x)[5]


def table_shares(reassigned, sst=sst1_energy):
    """[(reassigned share, first-order SST share)] of TABLE's cases, from the two callables x -> energy map [na, N]."""
    out = []
    for name, sig, ridge, _ in TABLE:
        x = sig()
        mask = m.ridge_cells(len(SCALES), N, ridge(), 1)
        R, T = reassigned(x), sst(x)
        out.append((float(R[mask].sum() / R.sum()), float(T[mask].sum() / T.sum())))
    return out


@functools.lru_cache(maxsize=None)
def model_table():
    return table_shares(model_energy)


def test_concentration_table():
    for (name, _, _, want), got in zip(TABLE, model_table()):
        print("%-8s reassigned %.5f   first-order SST %.5f" % (name, *got))
        assert abs(got[0] - want[0]) <= 5e-5 and abs(got[1] - want[1]) <= 5e-5
    # the point of the transform: on the sweep with clicks, more of the energy is on the ridges than under ssq_cwt's
    # first-order squeeze, which leaves every click a cone
    assert model_table()[2][0] > model_table()[2][1]


def test_float32_rounding_of_the_input_moves_no_strong_target():
    """tests/test_gpu_reassign_cwt.py caps the share of strong bins of a float32 call that land on another (k', m') than
    the complex128 model's at 1e-3.  The cap is a condition, so the model itself must stay well inside it: on the
    float32-rounded signals of the five GPU cases, reported in float32 (on the library's host-side tables, as there), the
    model moves no strong bin at all (8939, 719, 22302, 23066 and 8721 strong bins)."""
    import tests.test_gpu_reassign_cwt as g
    for i in g.RUNS:
        W, _, _, kk, mm = g.model(i)
        _, _, _, kf, mf = g.model(i, "fft", True)
        big = g.strong(W)
        share = (((kf != kk) | (mf != mm)) & big).sum() / big.sum()
        print("%s: %d strong bins, share on another target %.3g" % (g.IDS[i], big.sum(), share))
        assert share <= 1e-4
