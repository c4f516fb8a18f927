"""NumPy restatement of upstream ssqueezepy's synchrosqueezing step on a given transform (numba-free: upstream itself
does not import here), line by line after old/ssqueezepy/ssqueezing.py:13-245 and algos.py:44-252, :706-968.

The frequencies, when not given as an array, come from the mirror's own `_ssq_freqs` (ssqueezing.py:218-298; pinned
against oracle/upstream_oracle.py by the upstream tests); the bin expressions are oracle.upstream_oracle's
`_bins_lin` / `_bins_log` plus the two-segment map of algos.py:196-209.  Sums run in complex128 / float64."""
import numpy as np

from oracle import upstream_oracle as u

EPS64 = float(np.finfo(np.float64).eps)


def phase_cwt(Wx, dWx, gamma):
    """algos.py:721-729: inf where |Wx| < gamma, else |(B C - A D) / ((C^2 + D^2) 2 pi)|, in Wx's real dtype."""
    with np.errstate(all="ignore"):
        A, B, C, D = dWx.real, dWx.imag, Wx.real, Wx.imag
        w = np.abs((B * C - A * D) / ((C ** 2 + D ** 2) * 6.283185307179586))
    return np.where(np.abs(Wx) < gamma, np.inf, w).astype(Wx.real.dtype)


def phase_stft(Sx, dSx, Sfs, gamma):
    """algos.py:795-804 (oracle.upstream_oracle.phase_stft in Sx's real dtype)."""
    Sfs = np.asarray(Sfs, dtype=Sx.real.dtype)
    return u.phase_stft(Sx, dSx, Sfs, gamma).astype(Sx.real.dtype)


def transition_idx(v):
    """utils/cwt_utils.py:375-395 (`logscale_transition_idx`)."""
    from ssqueeze_rs_amd.upstream_scales import logscale_transition_idx
    v = np.asarray(v)
    if v.size < 3:                      # no second difference, so no transition (upstream's argmax of nothing raises)
        return None
    return logscale_transition_idx(v)


def bin_params(ssq_freqs, logscale):
    """algos.py:81-90 and :356-370 -> ('lin', vmin, dv) / ('log', vlmin, dvl) / ('pw', vlmin0, vlmin1, dvl0, dvl1,
    idx1); the array is read in its own dtype, as upstream reads it."""
    v = np.asarray(ssq_freqs)
    if not logscale:
        return ("lin", float(v[0]), max(float(v[1] - v[0]), EPS64))
    idx = transition_idx(v)
    vlmin = float(np.log2(v[0]))
    if idx is None:
        return ("log", vlmin, max(float(np.log2(v[1]) - np.log2(v[0])), EPS64))
    dvl0 = max(float(np.log2(v[1]) - np.log2(v[0])), EPS64)
    dvl1 = max(float(np.log2(v[idx]) - np.log2(v[idx - 1])), EPS64)
    return ("pw", vlmin, float(np.log2(v[idx - 1])), dvl0, dvl1, idx - 1)


def bins(w, params, omax, flipud):
    """The row k of every finite w (algos.py:173-252): clamped round half to even."""
    kind = params[0]
    with np.errstate(all="ignore"):
        if kind == "lin":
            k = u._bins_lin(w, params[1], params[2], omax)
        elif kind == "log":
            k = u._bins_log(w, params[1], params[2], omax)
        else:
            _, vlmin0, vlmin1, dvl0, dvl1, idx1 = params
            wl = np.log2(w)
            hi = np.minimum(np.rint((wl - vlmin1) / dvl1) + idx1, omax)
            lo = np.rint(np.maximum((wl - vlmin0) / dvl0, 0))
            k = np.where(wl > vlmin1, hi, lo)
            k = np.where(np.isnan(k), 0, k).astype(np.int64)
    return omax - k if flipud else k


def indexed_sum(Wx, w, ssq_freqs, const, logscale, flipud):
    """algos.py:153-252 (`indexed_sum_onfly`) on one [F, N] map: Tx[k, j] += Wx[i, j] * const[i] for finite w[i, j],
    rows in order."""
    F, N = Wx.shape
    const = np.broadcast_to(np.asarray(const, dtype=np.float64), (F,))
    out = np.zeros((F, N), dtype=np.complex128 if np.iscomplexobj(Wx) else np.float64)
    k = bins(w, bin_params(ssq_freqs, logscale), F - 1, flipud)
    cols = np.arange(N)
    for i in range(F):
        m = ~np.isinf(w[i])
        np.add.at(out, (k[i, m], cols[m]), Wx[i, m] * const[i])
    return out


def ssqueeze_fast(Wx, dWx, ssq_freqs, const, logscale, flipud, gamma, Sfs=None):
    """algos.py:126-150 with :860-968: the phase transform kept where |Wx| > gamma, binned and summed as above."""
    with np.errstate(all="ignore"):
        A, B, C, D = dWx.real, dWx.imag, Wx.real, Wx.imag
        q = (B * C - A * D) / ((C ** 2 + D ** 2) * 6.283185307179586)
        w = np.abs(q) if Sfs is None else np.abs(np.asarray(Sfs)[:, None] - q)
    w = np.where(np.abs(Wx) > gamma, w, np.inf)
    return indexed_sum(Wx, w, ssq_freqs, const, logscale, flipud)


def row_const(scales, scaletype, nv=None):
    """ssqueezing.py:122-127: ln2 / nv (per row for 'log-piecewise') or (s[1] - s[0]) / s for 'linear'."""
    s = np.asarray(scales, dtype=np.float64).reshape(-1)
    if scaletype.startswith("log"):
        return np.broadcast_to(np.log(2) / np.asarray(nv, dtype=np.float64).reshape(-1), s.shape).copy()
    return (s[1] - s[0]) / s


def ssqueeze(Wx, w, ssq_freqs, const, ssq_scaletype, squeezing="sum", flipud=False, dWx=None, gamma=None, Sfs=None):
    """ssqueezing.py:183-205 on a 2-D map with the frequencies, row weights and frequency type already settled:
    `Wx` replaced by the squeezing, then `indexed_sum_onfly` (w given) or `ssqueeze_fast` (dWx) -> Tx."""
    if callable(squeezing):
        Wx = squeezing(Wx)
    elif squeezing == "lebesgue":
        Wx = np.ones(Wx.shape, dtype=Wx.dtype) / len(Wx)
    elif squeezing == "abs":
        Wx = np.abs(Wx)
    logscale = ssq_scaletype.startswith("log")
    if w is None:
        return ssqueeze_fast(Wx, dWx, ssq_freqs, const, logscale, flipud, gamma, Sfs)
    return indexed_sum(Wx, w, ssq_freqs, const, logscale, flipud)
