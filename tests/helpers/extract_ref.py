"""Numpy model of the synchroextracting and transient-extracting STFT (`upstream.set_stft`, `upstream.tet_stft`, DESIGN
4.23).  No GPU, no library.  Built ON the models of the transforms whose maps it reads: `sst2_ref.sst2_ref(details=True)`
for the frequency map and `tsst_ref.tsst_ref(squeeze=False)` for the group-delay map, with their `arith` / `dtype` /
`tables` switches.

    set (axis 0): w = fs |Re w2| where order = 2, |D| > gamma^2 and Re w2 is finite, else fs |Re w1| (order 1: fs |Re w1| on
                  every cell), in the real dtype, +inf where |V| <= gamma;  b = the clamped round-half-even bin of w on
                  np.linspace(0, fs / 2, F) in that dtype;  keep where live and b == k
    tet (axis 1): tau = `tsst_ref`'s, +inf where |V| <= gamma;  r = rint(tau / (hop / fs)) in the real dtype, BEFORE any
                  clip to the frame range;  keep where live and r == 0
    Te = where(keep, V, +0)
The two rules are also exposed on their own (`keep_freq`, `keep_time`): a test rebuilds `keep` from the map a call
reports, in the call's dtype, and holds `Te` to it bit for bit."""
from __future__ import annotations

import numpy as np

from . import sst2_ref as s2
from . import tsst_ref as ts


def bins_of(w, fs):
    """The mirror's bin rule (`phase_bin_upstream`: clamped round-half-even on np.linspace(0, fs / 2, F)) on a reported
    map `w` [..., F, n_frames], in w's own dtype -> int64; meaningless where w is inf."""
    rdt = w.dtype.type
    F = w.shape[-2]
    Sfs = np.linspace(0, .5 * fs, F)
    f0, dw = rdt(Sfs[0]), rdt(Sfs[1] - Sfs[0])
    with np.errstate(all="ignore"):
        v = np.maximum((w - f0) / dw, rdt(0))
        kk = np.minimum(np.rint(v), F - 1)
    return np.where(np.isnan(kk), 0, kk).astype(np.int64)


def keep_freq(w, fs):
    """SET's keep rule on a reported frequency map `w` [..., F, n_frames]: live (w is not +inf) and its bin is its row."""
    rows = np.arange(w.shape[-2], dtype=np.int64)[:, None]
    return ~np.isposinf(w) & (bins_of(w, fs) == rows)


def keep_time(tau, hop, fs):
    """TET's keep rule on a reported offset map `tau`: live (tau is not +inf) and rint(tau / (hop / fs)) == 0 in tau's dtype."""
    rdt = tau.dtype.type
    with np.errstate(all="ignore"):
        r = np.rint(tau / rdt(hop / fs))
    return ~np.isposinf(tau) & (r == 0)


def extract(V, keep):
    """where(keep, V, +0 + 0i) in V's dtype."""
    return np.where(keep, V, V.dtype.type(0))


def set_ref(x, window, n_fft, hop_len=1, fs=1.0, padtype="reflect", modulated=True, order=2, gamma=None, arith="fft",
            dtype=np.complex128, tables=None):
    """-> (Te, V, w, keep): the synchroextracting STFT of the model.  w real (+inf where a cell is not live)."""
    if order not in (1, 2):
        raise ValueError(order)
    V, w2, kk, _, d = s2.sst2_ref(x, window, n_fft, hop_len=hop_len, fs=fs, padtype=padtype, modulated=modulated,
                                  gamma=gamma, arith=arith, dtype=dtype, details=True, tables=tables)
    rdt = w2.dtype.type
    if order == 1:
        with np.errstate(all="ignore"):
            w = np.where(d["keep"], rdt(fs) * np.abs(d["re_w1"].astype(rdt)), rdt(np.inf)).astype(rdt)
    else:
        w = w2
    keep = keep_freq(w, fs)
    return extract(V, keep), V, w, keep


def tet_ref(x, window, n_fft, hop_len=1, fs=1.0, padtype="reflect", modulated=True, order=2, gamma=None, arith="fft",
            dtype=np.complex128, tables=None, cols=None):
    """-> (Te, V, tau, keep): the transient-extracting STFT of the model.  cols: the frames to compute (`tsst_ref`)."""
    V, tau, _, _ = ts.tsst_ref(x, window, n_fft, hop_len=hop_len, fs=fs, padtype=padtype, modulated=modulated,
                               order=order, gamma=gamma, arith=arith, dtype=dtype, tables=tables, squeeze=False, cols=cols)
    keep = keep_time(tau, hop_len, fs)
    return extract(V, keep), V, tau, keep


def tone_identity(Te, g):
    """(2 / sum(g)) Re sum_k c_k Te[k, m], c = 1/2 on rows 0 and F - 1 and 1 elsewhere: what gives a tone on a bin centre
    back from the cells SET keeps."""
    c = np.ones(Te.shape[0])
    c[0] = c[-1] = 0.5
    return (2.0 / np.sum(g)) * (c[:, None] * Te).sum(0).real
