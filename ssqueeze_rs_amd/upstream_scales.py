"""Upstream's CWT scale utilities (old/ssqueezepy/utils/cwt_utils.py) for `ssqueeze_rs_amd.upstream`.

Host logic, as upstream's is: building the 'log' / 'log-piecewise' / 'linear' scale grids (`process_scales`,
`make_scales`, `cwt_scalebounds` and the searches beneath them) and classifying a given grid (`infer_scaletype`,
`logscale_transition_idx`, `nv_from_scales`).  The wavelet is evaluated by the library's own fp64 definition
(`ssq_upstream_psih`, the one the GPU wavelet tables and `adm_ssq` use), never by a second NumPy formula.  Wavelets:
'gmw' (bandpass, order 0) and 'morlet', as names or (name, {params}).  The `viz*` arguments are accepted and ignored.
Grids are returned as upstream returns them: float64, shape [na, 1].
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from . import _lib
from ._rs import _call, _ptr

pi = np.pi
DOWNSAMPLE = 4                         # configs.ini:40 (utils.cwt_utils.make_scales: downsample)


def _psih_fn(wavelet):
    """wavelet.fn: psih(w) at scale 1, fp64 (api_upstream.hip: psih_up)."""
    from .upstream import _wavelet       # (upstream imports this module)
    code, p0, p1 = _wavelet(wavelet)
    lib = _lib.load()

    def fn(w):
        w = np.ascontiguousarray(w, dtype=np.float64)
        out = np.empty(w.shape, dtype=np.float64)
        _call(lib.ssq_upstream_psih(code, p0, p1, _ptr(w), w.size, _ptr(out)))
        return out
    return fn


def _padded_len(N):
    """utils/common.py:32-51 (p2up), first output."""
    up, n1, n2 = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _call(_lib.load().ssq_upstream_p2up(int(N), C.byref(up), C.byref(n1), C.byref(n2)))
    return up.value


def _xifn(scale, N):
    """wavelets.py:473-483: [0, 1, .., N//2, -(N - N//2 - 1), .., -1] * (2 pi / N) * scale."""
    k = np.arange(N, dtype=np.float64)
    k[N // 2 + 1:] -= N
    return np.asarray(scale, dtype=np.float64) * (k * (2 * pi / N))


# ---------------------------------------------------------------------------------------------- searches (algos) ----
def find_maximum(fn, step_size=1e-3, steps_per_search=1e4, step_start=0, step_limit=1000, min_value=-1):
    """algos.py:625-663: max of |fn| (one maximum, non-decreasing up to it) and where it occurs."""
    steps_per_search = int(steps_per_search)
    largest_max = min_value
    increment = int(steps_per_search * step_size)
    search_idx = 0
    while True:
        start = step_start + increment * search_idx
        end = start + increment
        input_values = np.linspace(start, end, steps_per_search, endpoint=False)
        output_values = np.abs(np.asarray(fn(input_values)))
        output_max = output_values.max()
        if output_max > largest_max:
            largest_max = output_max
            input_value = input_values[np.argmax(output_values)]
        elif output_max < largest_max:
            break
        search_idx += 1
        if input_values.max() > step_limit:
            raise ValueError(("could not find function maximum with given (step_size, steps_per_search, step_start, "
                              "step_limit, min_value)=({}, {}, {}, {}, {})"
                              ).format(step_size, steps_per_search, step_start, step_limit, min_value))
    return input_value, largest_max


def find_first_occurrence(fn, value, step_size=1e-3, steps_per_search=1e4, step_start=0, step_limit=1000):
    """algos.py:666-703: the earliest input with |fn(input)| == value, searched in `step_size` steps."""
    steps_per_search = int(steps_per_search)
    increment = int(steps_per_search * step_size)
    step_limit_exceeded = False
    search_idx = 0
    while True:
        start = step_start + increment * search_idx
        end = start + increment
        input_values = np.linspace(start, end, steps_per_search, endpoint=False)
        if input_values.max() > step_limit:
            step_limit_exceeded = True
            input_values = np.clip(input_values, None, step_limit)
        output_values = np.abs(np.asarray(fn(input_values)))
        mxdiff = np.abs(np.diff(output_values)).max()
        if np.any(np.abs(output_values - value) <= mxdiff):
            idx = np.argmin(np.abs(output_values - value))
            break
        search_idx += 1
        if step_limit_exceeded:
            raise ValueError(("could not find input value to yield function output value={} with given (step_size, "
                              "steps_per_search, step_start, step_limit)=({}, {}, {}, {})"
                              ).format(value, step_size, steps_per_search, step_start, step_limit))
    return input_values[idx], output_values[idx]


# ------------------------------------------------------------------------------------------- grid classification ----
def infer_scaletype(scales):
    """cwt_utils.py:264-298 -> (scaletype, nv): 'log' (int nv), 'linear' (None) or 'log-piecewise' (nv per row,
    [na, 1]); thresholds by dtype (float64: 4e-15, float32: 8e-7; linear 1e3 times looser)."""
    scales = np.asarray(scales).reshape(-1, 1)
    if scales.dtype not in (np.float32, np.float64):
        raise TypeError("`scales.dtype` must be np.float32 or np.float64 (got %s)" % scales.dtype)
    th_log = 4e-15 if scales.dtype == np.float64 else 8e-7
    th_lin = th_log * 1e3
    if np.mean(np.abs(np.diff(np.log(scales), 2, axis=0))) < th_log:
        return "log", int(np.round(1 / np.diff(np.log2(scales), axis=0)[0].squeeze()))
    if np.mean(np.abs(np.diff(scales, 2, axis=0))) < th_lin:
        return "linear", None
    if logscale_transition_idx(scales) is None:
        raise ValueError("could not infer `scaletype` from `scales`; `scales` array must be linear or exponential. "
                         "(got diff(scales)=%s..." % np.diff(scales, axis=0)[:4])
    return "log-piecewise", nv_from_scales(scales)


def logscale_transition_idx(scales):
    """cwt_utils.py:375-395: `idx` splitting `scales` as [scales[:idx], scales[idx:]] at the one jump of the log step,
    or None (no jump, or more than one)."""
    scales = np.asarray(scales)
    scales_diff2 = np.abs(np.diff(np.log(scales), 2, axis=0))
    idx = np.argmax(scales_diff2) + 2
    diff2_max = scales_diff2.max()
    scales_diff2[idx - 2] = 0
    th = 1e-14 if scales.dtype == np.float64 else 1e-6
    if not np.any(diff2_max > 100 * np.abs(scales_diff2).mean()):
        return None
    if not np.all(np.abs(scales_diff2) < th):
        return None
    return idx


def nv_from_scales(scales):
    """cwt_utils.py:397-410: voices per octave per row, 1 / diff(log2 scales) with the first repeated ([na, 1] for a
    2-D input)."""
    scales = np.asarray(scales)
    logdiffs = 1 / np.diff(np.log2(scales), axis=0)
    nv = np.vstack([logdiffs[:1], logdiffs])
    idx = logscale_transition_idx(scales)
    if idx is not None:
        nv_transition_idx = np.argmax(np.abs(np.diff(nv, axis=0))) + 1
        assert nv_transition_idx == idx, "%s != %s" % (nv_transition_idx, idx)
    return nv


# --------------------------------------------------------------------------------------------------- scale bounds ----
def find_min_scale(wavelet, cutoff=1):
    """cwt_utils.py:412-432: the scale whose largest radian bin (pi) evaluates psih to `cutoff` * its peak, right of
    the peak for cutoff > 0, left of it otherwise."""
    fn = _psih_fn(wavelet)
    w_peak, peak = find_maximum(fn)
    step_start, step_limit = (w_peak, 10 * w_peak) if cutoff > 0 else (0, w_peak)
    w_cutoff, _ = find_first_occurrence(fn, value=abs(cutoff) * peak, step_start=step_start, step_limit=step_limit)
    return w_cutoff / pi


def find_max_scale(wavelet, N, bin_loc=1, bin_amp=1):
    """cwt_utils.py:435-457: the scale at which psih is `bin_amp` of its peak at the `bin_loc`-th bin."""
    fn = _psih_fn(wavelet)
    wc_ct, _ = find_maximum(fn)                       # wavelets.center_frequency(kind='peak-ct') (:739-743)
    scalec_ct = (4 / pi) * wc_ct
    xi = _xifn(scalec_ct, N)
    psih = fn(xi)[:N // 2 + 1]
    midx = np.argmax(psih)
    w_bin = xi[np.where(psih[:midx] < psih.max() * bin_amp)[0][-1]]
    return scalec_ct * (w_bin / xi[bin_loc])


def find_max_scale_alt(wavelet, N, min_cutoff=.1, max_cutoff=.8):
    """cwt_utils.py:630-696: the scale whose bins land symmetrically about psih's peak, between `min_cutoff` and
    `max_cutoff` of it, with the fewest divisions from dc."""
    if max_cutoff <= 0 or min_cutoff <= 0:
        raise ValueError("`max_cutoff` and `min_cutoff` must be positive (got %s, %s)" % (max_cutoff, min_cutoff))
    elif max_cutoff <= min_cutoff:
        raise ValueError("must have `max_cutoff > min_cutoff` (got %s, %s)" % (max_cutoff, min_cutoff))
    fn = _psih_fn(wavelet)
    w_peak, peak = find_maximum(fn)
    w_cutoff, _ = find_first_occurrence(fn, value=min_cutoff * peak, step_start=0, step_limit=w_peak)
    w_ltp = np.arange(w_cutoff, w_peak, step=1 / N)
    div_size = (w_peak - w_ltp[:-1]) * 2
    n_divs = w_ltp[:-1] / div_size
    try:
        idx = np.where(np.diff(n_divs % 1) < -.8)[0][0]
    except IndexError:
        raise Exception("Failed to find suffciently-integer xi divisions; try widening (min_cutoff, max_cutoff)")
    div_scale = div_size[idx + 1]
    w_1div = pi / (N / 2)
    return div_scale / w_1div


def find_downsampling_scale(wavelet, scales, span=5, tol=3, method='sum', nonzero_th=.02, nonzero_tol=4., N=None,
                            viz=False, viz_last=False):
    """cwt_utils.py:459-581 (method 'sum', the only one built): the index of the first scale past which `span`
    neighbouring wavelets peak within `tol` bins of their joint peak, on N (default 2048) bins; None if none is."""
    if method != 'sum':
        raise ValueError("find_downsampling_scale: only method='sum' is built")
    N = N or 2048
    if isinstance(wavelet, np.ndarray):
        Psih = wavelet
    else:
        fn = _psih_fn(wavelet)
        s = np.asarray(scales, dtype=np.float64).reshape(-1, 1)
        Psih = fn(s * _xifn(1.0, N)[None, :])              # Wavelet.__call__(scale=scales, N=N) (wavelets.py:62-86)
    if len(Psih) != len(scales):
        raise ValueError("len(Psih) != len(scales) (%s != %s)" % (len(Psih), len(scales)))
    Psih = Psih[:, :Psih.shape[1] // 2]
    n_scales = len(Psih)
    n_groups = n_scales - span - 1
    i = 0
    for i in range(n_groups):
        psihs = Psih[i:i + span]
        psihs_nonzeros = (psihs > nonzero_th * psihs.max(axis=1)[:, None])
        if psihs_nonzeros.sum() / span > nonzero_tol:
            continue
        psihs_peaks = np.where(psihs == psihs.max(axis=1)[:, None])
        joint_peak = np.argmax(np.prod(psihs, 0))
        if np.abs(psihs_peaks[1] - joint_peak).sum() < tol:
            break
    return i if (i < n_groups - 1) else None


def cwt_scalebounds(wavelet, N, preset=None, min_cutoff=None, max_cutoff=None, cutoff=None, bin_loc=None,
                    bin_amp=None, use_padded_N=True, viz=False):
    """cwt_utils.py:66-189 -> (min_scale, max_scale) for `preset` 'maximal', 'minimal', 'naive' or None."""
    defaults = dict(min_cutoff=.6, max_cutoff=.8, cutoff=-.5)
    if preset is not None:
        if any((min_cutoff, max_cutoff, cutoff)):
            warnings.warn("`preset` will override `min_cutoff, max_cutoff, cutoff`")
        elif preset == 'minimal' and any((bin_amp, bin_loc)):
            warnings.warn("`preset='minimal'` ignores `bin_amp` & `bin_loc`")
        if preset not in ('maximal', 'minimal', 'naive'):
            raise ValueError("`preset` must be one of: 'maximal', 'minimal', 'naive' (got %s)" % preset)
        if preset in ('naive', 'maximal'):
            min_cutoff, max_cutoff = None, None
            if preset == 'maximal':
                cutoff = -.5
        else:
            min_cutoff, max_cutoff, cutoff = defaults.values()
    else:
        if min_cutoff is None:
            min_cutoff = defaults['min_cutoff']
        elif min_cutoff <= 0:
            raise ValueError("`min_cutoff` must be >0 (got %s)" % min_cutoff)
        if max_cutoff is None:
            max_cutoff = defaults['max_cutoff']
        elif max_cutoff < min_cutoff:
            raise ValueError("must have `max_cutoff > min_cutoff` (got %s, %s)" % (max_cutoff, min_cutoff))
    bin_loc = bin_loc or (2 if preset == 'maximal' else None)
    bin_amp = bin_amp or (1 if preset == 'maximal' else None)
    cutoff = cutoff if (cutoff is not None) else defaults['cutoff']

    if preset == 'naive':
        return 1, N
    M = _padded_len(N) if use_padded_N else N
    min_scale = find_min_scale(wavelet, cutoff=cutoff)
    if preset in ('minimal', None):
        max_scale = find_max_scale_alt(wavelet, M, min_cutoff=min_cutoff, max_cutoff=max_cutoff)
    else:
        max_scale = find_max_scale(wavelet, M, bin_loc=bin_loc, bin_amp=bin_amp)
    return min_scale, max_scale


# ------------------------------------------------------------------------------------------------- making scales ----
def make_scales(N, min_scale=None, max_scale=None, nv=32, scaletype='log', wavelet=None, downsample=None):
    """cwt_utils.py:301-373 -> scales [na, 1] float64.  'log-piecewise' keeps every `downsample`-th (default 4,
    configs.ini:40) scale past `find_downsampling_scale`."""
    if scaletype == 'log-piecewise' and wavelet is None:
        raise ValueError("must pass `wavelet` for `scaletype == 'log-piecewise'`")
    if min_scale is None and max_scale is None and wavelet is not None:
        min_scale, max_scale = cwt_scalebounds(wavelet, N, use_padded_N=True)
    else:
        min_scale = min_scale or 1
        max_scale = max_scale or N
    downsample = int(DOWNSAMPLE if downsample is None else downsample)

    na = int(np.ceil(nv * np.log2(max_scale / min_scale)))
    mn_pow = int(np.floor(nv * np.log2(min_scale)))
    mx_pow = mn_pow + na
    if scaletype == 'log':
        scales = 2 ** (np.arange(mn_pow, mx_pow) / nv)
    elif scaletype == 'log-piecewise':
        scales = 2 ** (np.arange(mn_pow, mx_pow) / nv)
        idx = find_downsampling_scale(wavelet, scales)
        if idx is not None:
            scales1 = scales[:idx]
            scales2 = scales[idx + downsample - 1::downsample]
            scales = np.hstack([scales1, scales2])
    elif scaletype == 'linear':
        min_scale, max_scale = 2 ** (mn_pow / nv), 2 ** (mx_pow / nv)
        na = int(np.ceil(max_scale / min_scale))
        scales = np.linspace(min_scale, max_scale, na)
    else:
        raise ValueError("`scaletype` must be 'log' or 'linear'; got: %s" % scaletype)
    return scales.reshape(-1, 1)


def process_scales(scales, N, wavelet=None, nv=None, get_params=False, use_padded_N=True):
    """cwt_utils.py:196-262: makes the grid of a string `scales` ('log', 'log-piecewise' = 'log-piecewise:maximal',
    'linear', each optionally ':maximal' / ':minimal' / ':naive'), or validates an array; -> scales [na, 1], with
    `get_params` (scales, scaletype, na, nv)."""
    preset = None
    if isinstance(scales, str):
        if ':' in scales:
            scales, preset = scales.split(':')
        elif scales == 'log-piecewise':
            preset = 'maximal'
        if scales not in ('log', 'log-piecewise', 'linear'):
            raise ValueError("`scales` must be one of: 'log', 'log-piecewise', 'linear' (got %s)" % scales)
        if nv is None:
            nv = 32
        if wavelet is None:
            raise ValueError("must set `wavelet` if `scales` isn't array")
        scaletype = scales
    elif isinstance(scales, np.ndarray):
        if scales.squeeze().ndim != 1:
            raise ValueError("`scales`, if array, must be 1D (got shape %s)" % str(scales.shape))
        scaletype, _nv = infer_scaletype(scales)
        if scaletype == 'log':
            if nv is not None and _nv != nv:
                raise Exception("`nv` used in `scales` differs from `nv` passed (%s != %s)" % (_nv, nv))
            nv = _nv
        elif scaletype == 'log-piecewise':
            nv = _nv
        scales = scales.reshape(-1, 1)
    else:
        raise TypeError("`scales` must be a string or Numpy array (got %s)" % type(scales))
    if nv is not None and not isinstance(nv, np.ndarray):
        if not (nv > 0 and float(nv).is_integer()):
            raise ValueError(f"'nv' must be a positive integer (got {nv})")
        nv = int(nv)
    if not isinstance(scales, str):
        return scales if not get_params else (scales, scaletype, len(scales), nv)

    min_scale, max_scale = cwt_scalebounds(wavelet, N=N, preset=preset, use_padded_N=use_padded_N)
    scales = make_scales(N, min_scale, max_scale, nv=nv, scaletype=scaletype, wavelet=wavelet)
    return scales if not get_params else (scales, scaletype, len(scales), nv)
