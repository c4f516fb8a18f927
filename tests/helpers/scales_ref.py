"""NumPy restatement of upstream's scale utilities (old/ssqueezepy/utils/cwt_utils.py, algos.py:625-703) and of its
synchrosqueezing on non-exponential grids (ssqueezing.py:122-133, :247-283; algos.py:356-370, :860-897), with the
wavelets of oracle/upstream_oracle.py.  Test-only: the checks of `ssqueeze_rs_amd.upstream_scales` and of the upstream
reassignment kernel on 'log-piecewise' / 'linear' grids compare with this."""
import numpy as np

from oracle import upstream_oracle as u

EPS64 = float(np.finfo(np.float64).eps)


def _fn(wavelet):
    return u.wavelet_fn(wavelet)


def find_maximum(fn):                                      # algos.py:625-663 (defaults)
    best, k = -1, 0
    while True:
        t = np.linspace(10 * k, 10 * k + 10, 10000, endpoint=False)
        v = np.abs(fn(t))
        if v.max() > best:
            best, arg = v.max(), t[np.argmax(v)]
        elif v.max() < best:
            return arg, best
        k += 1
        if t.max() > 1000:
            raise ValueError("no maximum")


def find_first_occurrence(fn, value, step_start, step_limit):   # algos.py:666-703 (defaults)
    k = 0
    while True:
        t = np.linspace(step_start + 10 * k, step_start + 10 * k + 10, 10000, endpoint=False)
        over = t.max() > step_limit
        t = np.minimum(t, step_limit) if over else t
        v = np.abs(fn(t))
        if np.any(np.abs(v - value) <= np.abs(np.diff(v)).max()):
            return t[np.argmin(np.abs(v - value))]
        k += 1
        if over:
            raise ValueError("no occurrence")


def xi(scale, N):
    return scale * u.xifn(1.0, N)


def min_scale(wavelet, cutoff=-.5):                        # :412-432
    fn = _fn(wavelet)
    wp, peak = find_maximum(fn)
    lo, hi = (wp, 10 * wp) if cutoff > 0 else (0, wp)
    return find_first_occurrence(fn, abs(cutoff) * peak, lo, hi) / np.pi


def max_scale_maximal(wavelet, M, bin_loc=2):              # :435-457 (bin_amp 1)
    fn = _fn(wavelet)
    sc = (4 / np.pi) * find_maximum(fn)[0]
    x = xi(sc, M)
    p = fn(x)[:M // 2 + 1]
    m = np.argmax(p)
    return sc * (x[np.where(p[:m] < p.max())[0][-1]] / x[bin_loc])


def max_scale_minimal(wavelet, M, lo=.6, hi=.8):           # :630-696
    fn = _fn(wavelet)
    wp, peak = find_maximum(fn)
    wcut = find_first_occurrence(fn, lo * peak, 0, wp)
    w = np.arange(wcut, wp, step=1 / M)
    div = (wp - w[:-1]) * 2
    hits = np.where(np.diff((w[:-1] / div) % 1) < -.8)[0]
    if len(hits) == 0:
        raise Exception("no integer divisions")
    return div[hits[0] + 1] / (np.pi / (M / 2))


def scalebounds(wavelet, N, preset=None):                  # :66-189
    if preset == "naive":
        return 1, N
    M = u.p2up(N)[0]
    mx = max_scale_maximal(wavelet, M) if preset == "maximal" else max_scale_minimal(wavelet, M)
    return min_scale(wavelet), mx


def downsampling_idx(wavelet, scales, span=5, tol=3, N=2048):   # :459-581, method 'sum'
    P = _fn(wavelet)(np.asarray(scales).reshape(-1, 1) * u.xifn(1.0, N)[None, :])[:, :N // 2]
    n_groups = len(P) - span - 1
    i = 0
    for i in range(n_groups):
        g = P[i:i + span]
        if (g > .02 * g.max(axis=1)[:, None]).sum() / span > 4.:
            continue
        peaks = np.where(g == g.max(axis=1)[:, None])[1]
        if np.abs(peaks - np.argmax(np.prod(g, 0))).sum() < tol:
            break
    return i if i < n_groups - 1 else None


def make_scales(N, mn, mx, nv, scaletype, wavelet, downsample=4):   # :301-373
    na = int(np.ceil(nv * np.log2(mx / mn)))
    p0 = int(np.floor(nv * np.log2(mn)))
    if scaletype == "linear":
        a, b = 2 ** (p0 / nv), 2 ** ((p0 + na) / nv)
        return np.linspace(a, b, int(np.ceil(b / a))).reshape(-1, 1)
    s = 2 ** (np.arange(p0, p0 + na) / nv)
    if scaletype == "log-piecewise":
        idx = downsampling_idx(wavelet, s)
        if idx is not None:
            s = np.hstack([s[:idx], s[idx + downsample - 1::downsample]])
    return s.reshape(-1, 1)


def process_scales(spec, N, wavelet, nv=32):               # :196-262 for a string
    kind, _, preset = spec.partition(":")
    preset = preset or ("maximal" if kind == "log-piecewise" else None)
    mn, mx = scalebounds(wavelet, N, preset)
    return make_scales(N, mn, mx, nv, kind, wavelet)


def transition_idx(v):                                     # :375-395
    v = np.asarray(v).reshape(-1)
    d = np.abs(np.diff(np.log(v), 2))
    i = int(np.argmax(d))
    mx = d[i]
    d[i] = 0
    th = 1e-14 if v.dtype == np.float64 else 1e-6
    if not mx > 100 * d.mean() or not np.all(d < th):
        return None
    return i + 2


def scaletype(v):                                          # :264-298
    v = np.asarray(v).reshape(-1)
    th = 4e-15 if v.dtype == np.float64 else 8e-7
    if np.mean(np.abs(np.diff(np.log(v), 2))) < th:
        return "log"
    if np.mean(np.abs(np.diff(v, 2))) < th * 1e3:
        return "linear"
    if transition_idx(v) is None:
        raise ValueError("no scale type")
    return "log-piecewise"


# ------------------------------------------------------------------------------------- synchrosqueezing ----
def row_const(s, kind):                                    # ssqueezing.py:122-133
    s = np.asarray(s, dtype=np.float64).reshape(-1)
    if kind == "linear":
        return (s[1] - s[0]) / s
    ld = np.diff(np.log2(s))
    return np.log(2) * np.hstack([ld[:1], ld])             # ln2 / nv_from_scales


def piecewise_freqs(s, N, wavelet, dt=1.0):                # ssqueezing.py:247-283 (maprange 'peak')
    fn = _fn(wavelet)
    Np = u.p2up(N)[0]
    fc = lambda a: u.center_frequency_peak(fn, float(a), Np) / (2 * np.pi) / dt   # noqa: E731
    s = np.asarray(s, dtype=np.float64).reshape(-1)
    na, idx = len(s), transition_idx(s)
    fm, f1, fM = fc(s[-1]), fc(s[idx]), fc(s[0])

    def exp_fm(t, a, b):                                   # :294-298
        a_ = (a ** t.max() / b ** t.min()) ** (1 / (t.max() - t.min()))
        return a_ * (b ** (1 / t.max()) * (1 / a_) ** (1 / t.max())) ** t
    t2 = np.arange(na - idx - 1, na) / (na - 1)
    t1 = np.hstack([np.arange(0, na - idx - 1) / (na - 1), t2[0]])
    return np.hstack([exp_fm(t1, fm, f1)[:-1], exp_fm(t2, f1, fM)])


def bins(w, f, kind, idx=None, return_v=False):
    """algos.py:356-370, :860-897 on the ascending frequencies f: row index of every finite w (round half to even).
    idx: the transition of log-piecewise f (default: found on f itself).  return_v: also the unrounded bin position."""
    na = len(f)
    f = np.asarray(f, dtype=np.float64)
    with np.errstate(all="ignore"):
        if kind == "linear":
            v = np.maximum((w - f[0]) / (f[1] - f[0]), 0)
            k = np.minimum(np.round(v), na - 1).astype(np.int64)
            return (k, v) if return_v else k
        wl = np.log2(w)
        dvl0 = max(float(np.log2(f[1]) - np.log2(f[0])), EPS64)
        if kind == "log-piecewise" and idx is None:
            idx = transition_idx(f)
        if kind != "log-piecewise" or idx is None:
            v = np.nan_to_num(np.maximum((wl - np.log2(f[0])) / dvl0, 0), nan=0.0)
            k = np.minimum(np.round(v), na - 1).astype(np.int64)
            return (k, v) if return_v else k
        vlmin1 = float(np.log2(f[idx - 1]))
        dvl1 = max(float(np.log2(f[idx]) - np.log2(f[idx - 1])), EPS64)
        v_hi = (wl - vlmin1) / dvl1                         # rounded before the offset idx - 1 is added
        v_lo = np.nan_to_num((wl - np.log2(f[0])) / dvl0, nan=0.0)
        hi = np.minimum(np.round(v_hi) + (idx - 1), na - 1)
        lo = np.maximum(np.round(v_lo), 0)
        k = np.where(wl > vlmin1, hi, lo).astype(np.int64)
        return (k, np.where(wl > vlmin1, v_hi, v_lo)) if return_v else k


def squeeze(Wx, dWx, f, kind, const, squeezing="sum", flipud=True, gamma=None, idx=None):
    """ssqueezing.py:110-146 on given Wx / dWx [na, N]: Tx[k, j] += Wx[i, j] * const[i] -> (Tx, k)."""
    gamma = 10 * EPS64 if gamma is None else gamma
    na, N = Wx.shape
    with np.errstate(all="ignore"):
        A, B, C, D = dWx.real, dWx.imag, Wx.real, Wx.imag
        w = np.abs((B * C - A * D) / ((C ** 2 + D ** 2) * 6.283185307179586))
    keep = np.abs(Wx) > gamma
    k = bins(np.where(keep, w, 1.0), f, kind, idx)
    if flipud:
        k = na - 1 - k
    Wv = np.ones(Wx.shape, dtype=np.complex128) / na if squeezing == "lebesgue" else Wx.astype(np.complex128)
    Tx = np.zeros((na, N), dtype=np.complex128)
    cols = np.arange(N)
    for i in range(na):
        m = keep[i]
        np.add.at(Tx, (k[i, m], cols[m]), Wv[i, m] * const[i])
    return Tx, np.where(keep, k, -1)
