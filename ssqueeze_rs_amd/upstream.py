"""`ssqueeze_rs_amd.upstream` -- the upstream-parity mode and the inverses on the MI355X engine.

The Rust crate this package replaces was derived from ssqueezepy, vendored at /root/reference/old/ssqueezepy; the two
are numerically DIFFERENT variants (pad split, modulation, diff-window, wavelet normalisation, bin rule, constants --
SURVEY 8(a) lists them).  This module mirrors upstream's callables -- same names, keyword names, defaults, return
arity -- for the supported subset, backed by the *_v / inverse entry points of libssq_hip.so (include/ssq_hip.h).
Host logic upstream does in Python (window sizing, scale-type inference, frequency vectors) is Python here too;
everything per sample runs in HIP kernels.  There is no CPU fallback.

Supported subset (anything else raises ValueError naming the option):
  * `window`: ndarray (upstream's default DPSS / named windows come from scipy.signal, which callers can pass in);
  * `scales`: an explicit ndarray of any grid upstream accepts -- 'log', 'log-piecewise' or 'linear', classified by
    `infer_scaletype` (utils/cwt_utils.py:264-298).  Upstream's own grids come from `process_scales('log-piecewise', N,
    wavelet)` and the other scale utilities of utils/cwt_utils.py (`make_scales`, `cwt_scalebounds`, ...; module
    `upstream_scales`, re-exported here); the string forms of `scales` themselves are not accepted;
  * `ssq_cwt(ssq_freqs=)`: None (the scale type of `scales`), 'log', 'linear', 'log-piecewise' or an array (its type
    inferred, ssqueezing.py:193-194); log-piecewise frequencies are binned by the two-segment rule (algos.py:860-877)
    and every row is weighted as ssqueezing.py:122-133 weighs it;
  * wavelets 'gmw' (gamma, beta; bandpass norm, order 0) and 'morlet' (mu) -- names, or (name, {params});
  * higher-order GMWs through `cwt_higher_order` (_cwt.py:515-608), `ssq_cwt(order=)` and `cwt(order=<tuple / list /
    range>, average=)`: orders 0 .. 16, bandpass norm (`l1_norm=True`); an averaged order set is one transform with the
    averaged wavelet (the transform is linear in it), `average=False` runs every order from one forward FFT per signal.
    `cwt` keeps rejecting a bare int `order` other than 0 (the suite pins that ValueError); `order=(k,)` or
    `cwt_higher_order(x, order=k)` is the same transform;
  * difftype 'trig'; squeezing 'sum' / 'lebesgue'; padtype 'reflect' / 'zero' / 'symmetric' / 'replicate' /
    'wrap' (all of utils/common.py:54-158, fetched by index mapping on the device: csrc/pad_index.h);
  * `issq_cwt` / `issq_stft`: the full inverse, and the component inversion by curves `cc`, `cw`
    (_ssq_cwt.py:381-417): float64 [K + 1, N], or [B, K + 1, N] for a batched `Tx` [B, F, N] with the curves of a
    batched `extract_ridges`; the full inverses `istft`, `issq_stft`, `issq_cwt` and `icwt` take a 2-D map or a batch
    [B, F, N] -> [B, N] from one call (one window / wavelet / scale grid for the batch; `icwt(x_mean=)` a scalar or
    one mean per signal); power-of-two `n_fft` 16 .. 4096 with `hop_len <= n_fft` of a batched `istft` run the
    streaming kernel of csrc/istft_fused.hip when a signal has at least 256 tiles of frames, every other
    shape the three-kernel path of the 2-D call per signal;
  * `ssqueeze` (ssqueezing.py:13-245) on a transform the caller holds, from `w` or `dWx`, CWT or STFT, 2-D or batched
    3-D: `ssq_freqs` None / 'log' / 'linear' / 'log-piecewise' / an array, maprange 'peak' / 'maximal', squeezing
    'sum' / 'lebesgue' / 'abs' / a function (from `dWx`: 'sum' only), `was_padded`, `flipud`; STFT needs an array
    `ssq_freqs` (and `Sfs` with ssq_freqs[0] == Sfs[0] from `dSx`); `phase_cwt` (difftype 'trig') and `phase_stft`;
  * `ssq_stft2`: the second-order ("vertical") synchrosqueezed STFT, which upstream does not have (the definition is this
    project's: DESIGN 4.11, csrc/stft_sst2.hip): the conventions of `ssq_stft` (ndarray window, the five padtypes,
    'sum' / 'lebesgue', `flipud`, `modulated`, batches) with a power-of-two `n_fft` from 16 to 4096; its `Tx` inverts
    through `issq_stft` like a first-order one;
  * `mssq_stft`: the multisynchrosqueezed STFT (Yu, Wang and Zhao 2019; orders 1 and 2), which upstream does not have
    (the definition is this project's: DESIGN 4.17, csrc/stft_msst.hip): `ssq_stft2`'s frequency map asked again at the
    bin a coefficient landed on, `n_iter` steps in all (1 .. 64), which narrows the ridge of a signal whose modulation is
    not linear inside the window; the conventions of `ssq_stft2`; its `Tx` keeps every column's sum, so it inverts
    through `issq_stft` like a first-order one; `msst_walk` runs the walk alone on an int32 map the caller holds;
  * `tssq_stft`: the time-reassigned synchrosqueezed STFT (orders 1 and 2), which upstream does not have (the definition
    is this project's: DESIGN 4.13, csrc/stft_tsst.hip): every coefficient moves along time to its group delay, which
    concentrates impulses and fast chirps; the conventions of `ssq_stft2` (ndarray window, the five padtypes,
    `modulated`, batches, a power-of-two `n_fft` from 16 to 4096); no inverse (its row sums give the spectrum at n_fft
    points only);
  * `tmssq_stft`: the time-reassigned multisynchrosqueezed STFT (Yu, Lin, Ma and He 2020; orders 1 and 2), which upstream
    does not have (the definition is this project's: DESIGN 4.21, csrc/stft_tmsst.hip): `tssq_stft`'s time map asked
    again at the frame a coefficient landed on, `n_iter` steps in all (1 .. 64, with n_iter ceil(n_fft / (2 hop_len)) <=
    16384), which narrows the ridge of an impulsive or dispersive signal whose group delay is not linear inside the
    window; the conventions of `tssq_stft`; no inverse; `tmsst_walk` runs the walk alone on an int32 map the caller holds;
  * `set_stft` and `tet_stft`: the synchroextracting (Yu, Yu and Zhang 2017; Bao et al. 2019) and the transient-extracting
    (Yu 2019) STFT, orders 1 and 2, which upstream does not have (the definition is this project's: DESIGN 4.23,
    csrc/stft_extract.hip): a coefficient is kept where `ssq_stft2`'s frequency names its own row (`set_stft`) or
    `tssq_stft`'s group delay its own column (`tet_stft`) and zeroed elsewhere, in ONE kernel that writes every cell once;
    the conventions of `tssq_stft`; `Te` keeps the rows of `Sx`, a sparse input for `extract_ridges`; no inverse;
  * `reassign_stft`: the reassigned spectrogram (Kodera et al.; Auger and Flandrin 1995), which upstream does not have
    (the definition is this project's: DESIGN 4.14, csrc/stft_reassign.hip): every bin's energy |Sx|^2 moves along
    frequency and time at once, to its instantaneous frequency and group delay (first order); the conventions of
    `tssq_stft`; real, non-negative, energy-conserving, accumulated in fixed point (`REASSIGN_QUANTUM_LOG2`); no inverse;
  * `ssq_cwt2`: the second-order synchrosqueezed CWT, which upstream does not have either (the definition is this
    project's: DESIGN 4.12, csrc/cwt_sst2.hip): the conventions of `ssq_cwt` (ndarray scales of the three grids,
    `ssq_freqs` None / a string / an array, maprange 'peak' / 'maximal', 'sum' / 'lebesgue', the five padtypes, `flipud`,
    batches) for the order-0 'gmw' and 'morlet' wavelets; its `Tx` inverts through `issq_cwt` like a first-order one;
  * `mssq_cwt`: the multisynchrosqueezed CWT (orders 1 and 2), the CWT counterpart of `mssq_stft`, which upstream does not
    have (the definition is this project's: DESIGN 4.20, csrc/cwt_msst.hip): `ssq_cwt2`'s frequency map asked again at
    the row nearest in log frequency to the bin a coefficient landed on (`mssq_cwt_row_of_bin`), `n_iter` steps in all
    (1 .. 64), for 2 .. 2049 scales; the conventions of `ssq_cwt2`; a coefficient keeps its own row weight and its phase,
    so `Tx` keeps every column's weighted sum and inverts through `issq_cwt` like a first-order one; `mssq_cwt_walk` runs
    the walk alone on a frequency map the caller holds;
  * `reassign_cwt`: the reassigned scalogram (Auger and Flandrin 1995, III), which upstream does not have (the definition
    is this project's: DESIGN 4.15, csrc/cwt_reassign.hip): every coefficient's energy |Wx|^2 moves along frequency and
    time at once, to its instantaneous frequency and group delay (first order); the conventions of `ssq_cwt2` without
    row weights and `squeezing`; real, non-negative, energy-conserving, accumulated by 64-bit integer atomic adds in
    fixed point (`reassign_cwt_quantum_log2`); no inverse;
  * `tssq_cwt`: the time-reassigned synchrosqueezed CWT (orders 1 and 2), which upstream does not have (the definition
    is this project's: DESIGN 4.16, csrc/cwt_tsst.hip): every complex coefficient moves along time inside its own row,
    to its group delay, rotated to keep its phase reference, so clicks and fast sweeps concentrate and add coherently;
    the conventions of `ssq_cwt2` without `ssq_freqs`, `maprange`, `squeezing`, `flipud` and row weights; accumulated by
    64-bit integer atomic adds in fixed point (`tssq_cwt_quantum_log2`); no inverse (a per-row marginal identity);
  * `tmssq_cwt`: the time-reassigned multisynchrosqueezed CWT (orders 1 and 2), the CWT counterpart of `tmssq_stft`,
    which upstream does not have (the definition is this project's: DESIGN 4.22, csrc/cwt_tmsst.hip): `tssq_cwt`'s time
    map asked again at the column a coefficient landed on, `n_iter` steps in all (1 .. 64), which narrows the ridge of a
    dispersive signal; a target may lie anywhere in its row, so the walk kernel stages a tile in LDS and reads the far
    steps from device memory; the conventions, the accumulation and the quantum of `tssq_cwt`; no inverse;
    `tmssq_cwt_walk` runs the walk alone on an int32 map the caller holds;
  * `set_cwt` and `tet_cwt`: the synchroextracting and the transient-extracting CWT (orders 1 and 2), the CWT
    counterparts of `set_stft` and `tet_stft`, which upstream does not have (the definition is this project's: DESIGN
    4.24, csrc/cwt_extract.hip): a coefficient is kept where `ssq_cwt2`'s frequency falls in the band of its own row
    (`set_cwt`, the bands of `set_cwt_row_edges`) or `tssq_cwt`'s group delay names its own column (`tet_cwt`) and zeroed
    elsewhere, by ONE operator kernel that writes every cell once; the conventions of `tssq_cwt`; no inverse;
  * `lmssq_stft`: the local maximum synchrosqueezed STFT (Yu, Wang, Zhao and Liu 2019), which upstream does not have (the
    definition is this project's: DESIGN 4.25, csrc/stft_lmsst.hip): a coefficient moves to the row where |Sx| has its
    maximum inside a window of +- `delta` rows (default `lmsst_default_delta`, the window's main lobe); no derivative of
    the window, ONE transform per frame, decided in LDS by ONE kernel that writes every cell of `Tx` once; the
    conventions of `mssq_stft`; every column keeps its sum, so `Tx` inverts through `issq_stft`;
  * `lmssq_cwt`: the local maximum synchrosqueezed CWT, the CWT counterpart of `lmssq_stft`, which upstream does not have
    (the definition is this project's: DESIGN 4.26, csrc/cwt_lmsst.hip): a coefficient moves to the frequency of the row
    where |Wx| has its maximum inside +- `delta` rows (default `lmssq_cwt_default_delta`), with its own row weight; ONE
    inverse transform per row, for 2 .. 2049 scales; the conventions of `mssq_cwt`; `Tx` inverts through `issq_cwt`;
    `lmsst_rows` runs the window maximum alone on a real map the caller holds;
  * `conceft_cwt`: ConceFT, the multitaper synchrosqueezed CWT (Daubechies, Wang and Wu 2016), which upstream does not
    have (the definition is this project's: DESIGN 4.18, csrc/cwt_conceft.hip): `ssq_cwt` under M random unit
    combinations of the GMWs of J orders (`conceft_vectors`, gauged by the orders' admittances `gmw_adm_ssq`), averaged,
    which keeps a ridge sharp where noise scatters the single-wavelet reassignment; the 2 J planes of
    `cwt_higher_order` are computed once and every draw is formed, binned and summed from them in one fused kernel, no
    atomics, bitwise the same whatever the batch; the conventions of `ssq_cwt` for the 'gmw' wavelet and squeezing
    'sum'; its `Tx` inverts through `issq_cwt` like a first-order one;
  * `conceft_stft`: ConceFT on the STFT, the multitaper synchrosqueezed STFT (Daubechies, Wang and Wu 2016), which
    upstream does not have (the definition is this project's: DESIGN 4.19, csrc/stft_conceft.hip): the first-order
    synchrosqueezed STFT under M random unit combinations of J tapers (an ndarray [J, win_len], or the orthonormal
    Hermite windows of `hermite_windows`), gauged by the tapers' centre samples and averaged; the 2 J planes are computed
    once in fp64 and every draw is formed, binned and summed from them in one kernel, no atomics, bitwise the same
    whatever the batch and the workspace; the conventions of `ssq_stft2` (the five padtypes, `flipud`, `modulated`,
    batches, a power-of-two `n_fft` from 16 to 4096) with squeezing 'sum'; its `Tx` inverts through
    `issq_stft(Tx, window=tapers[0])`;
  * `extract_ridges` (ridge_extraction.py:11-233) on any 2-D (or batched 3-D) real, integer or complex map, with the
    serial backward trace (`parallel` is accepted and ignored).
dtype: float64 in -> complex128 (upstream's 'float64'); float32 in -> complex64 (upstream's default 'float32').

Parity: unpinned against upstream itself (it does not import here: numba missing); tests compare with the numba-free
restatement oracle/upstream_oracle.py and pin upstream's own reconstruction thresholds
(old/tests/reconstruction_test.py:111-123, :160-206).  Ridges: unpinned likewise; tests compare with the numba-free
restatement tests/helpers/ridge_oracle.py (the forward DP bitwise) and pin upstream's one stated fact,
old/tests/ridge_extraction_test.py:17-26 (`test_basic`).
"""
from __future__ import annotations

import ctypes as C
import math
import warnings
from types import SimpleNamespace

import numpy as np

from . import _lib
from ._lib import SQUEEZE, SSQ_F32, SSQ_F64, WAVELET
from ._rs import _call, _cdtype, _ptr
from .upstream_scales import (cwt_scalebounds, find_downsampling_scale, find_first_occurrence,  # noqa: F401
                              find_max_scale, find_max_scale_alt, find_maximum, find_min_scale, infer_scaletype,
                              logscale_transition_idx, make_scales, nv_from_scales, process_scales)

VARIANT_UPSTREAM, VARIANT_MODULATED, VARIANT_FLIPUD = 1, 2, 4
FREQS = {"log": 0, "linear": 1, "log-piecewise": 2}     # include/ssq_hip.h: SSQ_FREQS_LOG, _LINEAR, _LOG_PIECEWISE
EPS32, EPS64 = float(np.finfo(np.float32).eps), float(np.finfo(np.float64).eps)
# utils/common.py:54-158; include/ssq_hip.h: SSQ_PAD_*.  (`_lib.PAD` is the reference drop-in's table: two names.)
PAD_MODES = {"reflect": 0, "zero": 1, "symmetric": 2, "replicate": 3, "wrap": 4}
GMW_MAX_ORDER = 16                      # the highest GMW order the library builds (csrc/cwt_kernels.h: kGmwMaxOrder)


# ------------------------------------------------------------------------------------------------------- helpers ----
def _signal(x):
    if not isinstance(x, np.ndarray) or x.ndim not in (1, 2):
        raise TypeError("`x` must be a 1D or 2D numpy array")
    if x.dtype not in (np.float32, np.float64):
        x = x.astype(np.float64)
    batched = x.ndim == 2
    xa = np.ascontiguousarray(x if batched else x[None, :])
    return xa, batched, (SSQ_F32 if xa.dtype == np.float32 else SSQ_F64)


def _rdtype(code):
    return np.float32 if code == SSQ_F32 else np.float64


def _ccode(dtype):
    """The library's dtype code of a complex64 / complex128 map."""
    return SSQ_F32 if dtype == np.complex64 else SSQ_F64


def _eps(code):
    return EPS32 if code == SSQ_F32 else EPS64


def _gamma_arg(gamma):
    """`gamma` as the library takes it: -1 asks for its default (10 eps of the dtype)."""
    return -1.0 if gamma is None else float(gamma)


def _unbatch(batched, *arrays):
    """The arrays that are not None, without the batch axis where the call's input had none."""
    return [a if batched else a[0] for a in arrays if a is not None]


def _squeeze_code(squeezing):
    if squeezing not in SQUEEZE:
        raise ValueError(f"squeezing {squeezing!r}: 'sum' and 'lebesgue' are built")
    return SQUEEZE[squeezing]


def _order12(order, built):
    if isinstance(order, (bool, np.bool_)) or order not in (1, 2):
        raise ValueError(f"order {order!r}: {built}")
    return int(order)


def _shape_checked(lib, rc):
    """A `*_workspace_bytes` result: negative is the C entry's refusal of the shape (made on the host, no GPU)."""
    if rc < 0:
        raise ValueError(lib.ssq_last_error().decode("utf-8", "replace"))


def _pad_code(padtype):
    """Pad code of upstream's `padtype` (`padsignal`, utils/common.py:54-158).  The kernels fetch padded samples through
    one index map (csrc/pad_index.h), no padded copy: 'reflect' is one mirror about the end sample and 'zero' zeros,
    as before; 'symmetric', 'replicate' and 'wrap' are np.pad's 'symmetric', 'edge' and 'wrap' in closed form, for any
    pad width.  Upstream slices 'symmetric' out of ONE reversed copy (common.py:144-149), which agrees with np.pad
    while a pad is no wider than the signal and comes up short beyond that; np.pad is followed there."""
    if not isinstance(padtype, str) or padtype not in PAD_MODES:
        raise ValueError(f"padtype {padtype!r}: must be one of 'reflect', 'zero', 'symmetric', 'replicate', 'wrap'")
    return PAD_MODES[padtype]


def get_window(window, win_len, n_fft=None):
    """old/ssqueezepy/_stft.py:257-309 for an ndarray window: centre zero-pad to n_fft."""
    if not isinstance(window, np.ndarray):
        raise ValueError("`window` must be an ndarray here (named / default DPSS windows: scipy.signal.get_window, "
                         "scipy.signal.windows.dpss(win_len, max(4, win_len//8), sym=False))")
    window = np.asarray(window, dtype=np.float64)
    if n_fft is None:
        return window
    if win_len > n_fft:
        raise ValueError("Can't have `win_len > n_fft` ({} > {})".format(win_len, n_fft))
    pl = (n_fft - win_len) // 2
    pr = n_fft - win_len - pl
    if len(window) < (win_len + pl + pr):
        window = np.pad(window, [pl, pr])
    return np.ascontiguousarray(window)


def _wavelet(wavelet):
    name, kw = (wavelet, {}) if isinstance(wavelet, str) else wavelet
    if name == "gmw":
        if kw.get("norm", "bandpass") != "bandpass" or kw.get("order", 0) != 0 or kw.get("centered_scale", False):
            raise ValueError("gmw: only norm='bandpass', order=0, centered_scale=False are built")
        return WAVELET["gmw"], float(kw.get("gamma", 3.0)), float(kw.get("beta", 60.0))
    if name == "morlet":
        return WAVELET["morlet"], float(kw.get("mu", 13.4)), 0.0
    raise ValueError(f"wavelet {name!r}: the MI355X engine builds 'gmw' and 'morlet'")


def gmw_k_constants(gamma, beta, k):
    """_gmw.py:366-395 (`_gmw_k_constants`, bandpass norm) in fp64: the coefficients of the order-k GMW's polynomial in
    y = 2 w^gamma, psih_k(w) = sum_m k_consts[m] y^m * exp(-beta ln wc + wc^gamma + beta ln w - w^gamma)."""
    gamma, beta, k = float(gamma), float(beta), int(k)
    r = (2 * beta + 1) / gamma
    c = r - 1
    coeff = math.sqrt(math.exp(math.lgamma(r) + math.lgamma(k + 1) - math.lgamma(k + r)))
    out = np.zeros(k + 1, dtype=np.float64)
    for m in range(k + 1):
        fact = math.exp(math.lgamma(k + c + 1) - math.lgamma(c + m + 1) - math.lgamma(k - m + 1))
        out[m] = (-1) ** m * fact / math.gamma(m + 1)
    return out * coeff * 2


def gmw_order_coefficients(gamma, beta, orders, average=True):
    """The polynomials the library evaluates for the GMW orders `orders`: [len(orders), n] float64, each order's
    `gmw_k_constants` padded with zeros to n = max(orders) + 1; with `average`, [1, n]: their mean over the orders (the
    averaged wavelet, whose transform is the mean of the orders' transforms)."""
    orders = [int(k) for k in orders]
    n = max(orders) + 1
    polys = np.zeros((len(orders), n), dtype=np.float64)
    for i, k in enumerate(orders):
        polys[i, :k + 1] = gmw_k_constants(gamma, beta, k)
    return polys.mean(axis=0, keepdims=True) if average else polys


def _wavelet_name(wavelet):
    return wavelet if isinstance(wavelet, str) else wavelet[0]


def _order_args(order, average, wavelet, l1_norm=True, higher=False):
    """_cwt.py:236-241 and cwt_higher_order's _process_args (:566-590) -> None for the plain transform, else
    (orders, average) with upstream's rules: an int order is one transform; a tuple / list / range averages unless
    `average` is False; a single order with `average=True` warns and does not average.  `higher`: cwt_higher_order's
    own entry, which takes every order (0 included) through the GMW check."""
    is_set = isinstance(order, (tuple, list, range))
    orders = tuple(order) if is_set else (order,)
    for k in orders:
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"`order` must be an int or a tuple / list / range of ints (got {order!r})")
        if k < 0:
            raise ValueError(f"`order` must be >= 0 (got {order!r})")
        if k > GMW_MAX_ORDER:
            raise ValueError(f"`order` above {GMW_MAX_ORDER} is not built (got {order!r})")
    if not orders:
        raise ValueError("`order` is empty")
    if not (is_set or higher) and orders[0] == 0:
        return None                                        # _cwt.py:236: `order > 0` only
    if _wavelet_name(wavelet) != "gmw":
        raise ValueError("`order`: the wavelet must be GMW for higher-order transforms (got %r)" % (wavelet,))
    if not l1_norm and any(k != 0 for k in orders):
        raise ValueError("`order` with `l1_norm=False`: upstream's energy-normalised GMW is not built")
    if len(orders) == 1 and average:
        warnings.warn("`average` ignored with single `order`")
        average = False
    return tuple(int(k) for k in orders), bool(average or (average is None and is_set))


def _own_dtype(a):
    """1-D view of an array in its own float dtype (float32 / float64; anything else as float64): upstream's scale-type
    and transition tests (cwt_utils.py:264-298, :375-395) take their thresholds from it."""
    a = np.asarray(a)
    return (a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)).reshape(-1)


def _scales(scales):
    """-> (s float64 [na], scaletype, nv, s_own) by utils/cwt_utils.py:264-298; s_own: the array in its own dtype, on
    which the transition of a log-piecewise grid is found (float32 grids have float32 thresholds, as upstream).  An
    array within 4e-12 of exponential spacing is 'log' with int nv (this mirror's check of float64 grids since it was
    built); any other goes through `infer_scaletype` ('linear': nv None; 'log-piecewise': nv per row) and raises
    ValueError where upstream does, or where upstream's transforms fail later (a log-piecewise segment of one scale)."""
    if not isinstance(scales, np.ndarray):
        raise ValueError("`scales` must be an explicit ndarray (the string forms are not accepted; "
                         "`process_scales(scales, N, wavelet)` builds upstream's grids)")
    s = np.ascontiguousarray(scales, dtype=np.float64).reshape(-1)
    s_own = _own_dtype(scales)
    if len(s) < 2:
        raise ValueError("`scales` must hold at least 2 scales")
    with np.errstate(divide="ignore", invalid="ignore"):
        d2 = np.mean(np.abs(np.diff(np.log(s), 2)))
    if not d2 >= 4e-15 * 1e3:
        return s, "log", int(np.round(1 / np.diff(np.log2(s))[0])), s_own
    with np.errstate(divide="ignore", invalid="ignore"):
        scaletype, nv = infer_scaletype(s_own)
    if scaletype == "log-piecewise":
        idx = logscale_transition_idx(s_own)
        if idx is None or idx < 2 or len(s) - idx < 2:     # upstream's _exp_fm / icwt fail on a one-scale segment
            raise ValueError("log-piecewise `scales` need at least 2 scales on either side of the transition")
    return s, scaletype, nv, s_own


def _dt(fs, t, N):
    """utils/cwt_utils.py:698-720 (_process_fs_and_t)."""
    if t is not None:
        if len(t) != N:
            raise ValueError("`t` must be of same length as `x`")
        return float((t[-1] - t[0]) / (N - 1))
    return 1.0 / float(fs) if fs is not None else 1.0


def adm_ssq(wavelet) -> float:
    """utils/cwt_utils.py:28-47."""
    code, p0, p1 = _wavelet(wavelet)
    out = C.c_double(0)
    _call(_lib.load().ssq_upstream_adm(code, p0, p1, 0, C.byref(out)))
    return out.value


def adm_cwt(wavelet) -> float:
    """utils/cwt_utils.py:50-63."""
    code, p0, p1 = _wavelet(wavelet)
    out = C.c_double(0)
    _call(_lib.load().ssq_upstream_adm(code, p0, p1, 1, C.byref(out)))
    return out.value


def p2up(n):
    """utils/common.py:32-51."""
    up, n1, n2 = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _call(_lib.load().ssq_upstream_p2up(int(n), C.byref(up), C.byref(n1), C.byref(n2)))
    return up.value, n1.value, n2.value


# --------------------------------------------------------------------------------------------------- STFT family ----
SST2_MIN_N_FFT, SST2_MAX_N_FFT = 16, 4096     # csrc/stft_sst2.hip: one frame is held by n_fft / 16 lanes of a workgroup


def _stft_front(x, window, n_fft, win_len, hop_len, fs, t, pow2_for=None):
    """The front end of the STFT family: the signal, `fs`, the `n_fft` and `win_len` defaults, the sized window and
    the dtypes of the results.  `pow2_for`: the name of a transform whose kernels take a
    power-of-two `n_fft` only (None: any length)."""
    f = SimpleNamespace()
    f.xa, f.batched, f.code = _signal(x)
    f.batch, f.N = f.xa.shape
    f.fs = 1.0 / _dt(fs, t, f.N)
    n_fft = n_fft or min(f.N // hop_len, 512)
    if pow2_for is not None:
        if (not isinstance(n_fft, (int, np.integer)) or isinstance(n_fft, (bool, np.bool_))
                or not SST2_MIN_N_FFT <= n_fft <= SST2_MAX_N_FFT or n_fft & (n_fft - 1)):
            raise ValueError(f"n_fft {n_fft!r}: {pow2_for} takes a power of two from {SST2_MIN_N_FFT} to {SST2_MAX_N_FFT}")
        n_fft = int(n_fft)
    if win_len is None:
        win_len = len(window) if isinstance(window, np.ndarray) else n_fft
    f.n_fft, f.win = n_fft, get_window(window, win_len, n_fft)
    f.n_freqs = n_fft // 2 + 1
    f.cdt, f.rdt = _cdtype(f.code), _rdtype(f.code)
    return f


def _stft_shape(f, hop_len):
    """The shape of the family's maps.  Its callers ask for the GPU first: `hop_len = 0` with an `n_fft` given divides by
    zero here, after `require_gpu()`, as it always has."""
    f.n_frames = (f.N - 1) // hop_len + 1
    return f.batch, f.n_freqs, f.n_frames


def _variant(modulated, flipud=False):
    return VARIANT_UPSTREAM | (VARIANT_MODULATED if modulated else 0) | (VARIANT_FLIPUD if flipud else 0)


def _Sfs(f):
    return np.linspace(0, .5 * f.fs, f.n_freqs, dtype=f.rdt)               # _ssq_stft.py:248-257


def _times(f, hop_len):
    return (np.arange(f.n_frames) * hop_len / f.fs).astype(f.rdt)


def stft(x, window=None, n_fft=None, win_len=None, hop_len=1, fs=None, t=None, padtype="reflect", modulated=True,
         derivative=False, dtype=None):
    """ssqueezepy.stft (old/ssqueezepy/_stft.py:13-193) -> Sx, or (Sx, dSx) with derivative=True."""
    lib = _lib.load()
    f = _stft_front(x, window, n_fft, win_len, hop_len, fs, t)
    _lib.require_gpu()
    shape = _stft_shape(f, hop_len)
    Sx = _lib.pinned_empty(shape, f.cdt)
    dSx = _lib.pinned_empty(shape, f.cdt) if derivative else None
    _call(lib.ssq_stft_host_v(f.code, _ptr(f.xa), f.batch, f.N, _ptr(f.win), f.n_fft, hop_len, f.fs,
                              _pad_code(padtype), _variant(modulated), _ptr(Sx), _ptr(dSx)))   # (padtype: after the GPU)
    out = _unbatch(f.batched, Sx, dSx)
    return tuple(out) if derivative else out[0]


def istft(Sx, window=None, n_fft=None, win_len=None, hop_len=1, N=None, modulated=True, win_exp=1):
    """ssqueezepy.istft (old/ssqueezepy/_stft.py:196-254).  `Sx` [n_fft//2 + 1, n_frames] -> [N]; extension: a batch
    [B, n_fft//2 + 1, n_frames] -> [B, N] from one call (one window, n_fft, hop_len, N for all of it; signal b's result
    does not depend on B)."""
    lib = _lib.load()
    if not isinstance(Sx, np.ndarray) or Sx.ndim not in (2, 3) or Sx.dtype not in (np.complex64, np.complex128):
        raise TypeError("`Sx` must be a 2D (or batched 3D [B, n_fft//2 + 1, n_frames]) complex64 / complex128 array")
    n_fft = n_fft or (Sx.shape[-2] - 1) * 2
    win_len = win_len or n_fft
    N = N or hop_len * Sx.shape[-1]
    if Sx.shape[-2] != n_fft // 2 + 1:
        raise ValueError("`Sx` has %d rows, n_fft=%d needs %d" % (Sx.shape[-2], n_fft, n_fft // 2 + 1))
    if Sx.ndim == 3 and Sx.shape[0] < 1:
        raise ValueError("`Sx` holds no signal (B == 0)")
    win = get_window(window, win_len, n_fft)
    code = _ccode(Sx.dtype)
    _lib.require_gpu()
    Sc = np.ascontiguousarray(Sx)
    if Sx.ndim == 3:
        x = np.empty((Sc.shape[0], N), dtype=_rdtype(code))
        _call(lib.ssq_istft_batch_host(code, _ptr(Sc), Sc.shape[0], Sc.shape[2], _ptr(win), n_fft, hop_len, N,
                                       int(bool(modulated)), int(win_exp), _ptr(x)))
        return x
    x = np.empty(N, dtype=_rdtype(code))
    _call(lib.ssq_istft_host(code, _ptr(Sc), Sc.shape[1], _ptr(win), n_fft, hop_len, N, int(bool(modulated)),
                             int(win_exp), _ptr(x)))
    return x


def ssq_stft(x, window=None, n_fft=None, win_len=None, hop_len=1, fs=None, t=None, modulated=True, ssq_freqs=None,
             padtype="reflect", squeezing="sum", gamma=None, preserve_transform=None, dtype=None, astensor=True,
             flipud=False, get_w=False, get_dWx=False):
    """ssqueezepy.ssq_stft (old/ssqueezepy/_ssq_stft.py:12-137) -> (Tx, Sx, ssq_freqs, Sfs[, w][, dSx])."""
    lib = _lib.load()
    if ssq_freqs is not None:
        raise ValueError("`ssq_freqs` other than None (= Sfs, linear) is not built")
    squeeze = _squeeze_code(squeezing)
    f = _stft_front(x, window, n_fft, win_len, hop_len, fs, t)
    _lib.require_gpu()
    shape = _stft_shape(f, hop_len)
    Tx, Sx = _lib.pinned_empty(shape, f.cdt), _lib.pinned_empty(shape, f.cdt)
    dSx = _lib.pinned_empty(shape, f.cdt) if get_dWx else None
    wk = _lib.pinned_empty(shape, f.cdt) if get_w else None
    freqs = np.empty(f.n_freqs, dtype=np.float64)
    _call(lib.ssq_ssq_stft_host_v(f.code, _ptr(f.xa), f.batch, f.N, _ptr(f.win), f.n_fft, hop_len, f.fs,
                                  _pad_code(padtype), squeeze, _gamma_arg(gamma),     # (padtype: after the GPU)
                                  _variant(modulated, flipud), _ptr(Tx), _ptr(freqs), _ptr(Sx), _ptr(dSx), _ptr(wk)))
    w = wk.real.copy() if get_w else None
    return (*_unbatch(f.batched, Tx, Sx), freqs.astype(f.rdt), _Sfs(f), *_unbatch(f.batched, w, dSx))


def ssq_stft2(x, window=None, n_fft=None, win_len=None, hop_len=1, fs=None, t=None, modulated=True, padtype="reflect",
              squeezing="sum", gamma=None, flipud=False, get_w=False):
    """Second-order ("vertical") synchrosqueezed STFT -> (Tx, Sx, ssq_freqs, Sfs[, w2]); not in upstream (Oberlin,
    Meignen and Perrier 2015; Behera, Meignen and Oberlin 2018), conventions of `ssq_stft`.

    With g the sized window, g1 and g2 its first and second spectral derivatives (Nyquist term zeroed), tg = u g,
    tg1 = u g1 (u = sample index - n_fft // 2) and V, V1, V2, Vt, Vt1 the STFTs of `x` with them, per sample:
        w1 = k / n_fft - (V1 / V) / (2 pi i)       D = Vt V1 - Vt1 V       q = (V2 V - V1^2) / (2 pi i D)
        w2 = w1 - q Vt / V
    A bin's frequency is fs |Re w2| where |D| > gamma^2 and Re w2 is finite, else fs |Re w1| (`ssq_stft`'s w); bins with
    |V| > gamma (default 10 eps of the dtype) are reassigned by `ssq_stft`'s rule, every column's rows in ascending
    order (no atomics: the result does not depend on the batch).  For a linear chirp under a Gaussian window Re w2 is
    the instantaneous frequency, where the first-order w is biased by the chirp rate.  `Sx` equals `stft(x, ...)`;
    `w2` (get_w=True) is +inf where a bin is not kept.  `Tx` sums to the same rows as a first-order one, so
    `issq_stft`, `extract_ridges` and the component inversion take it unchanged.

    float32 in gives complex64 / float32 out, but the transforms and the operator run in fp64 for either dtype (the
    operator is a quotient of two differences of products: fp32 transforms of 1024 points and more put over one
    strong bin in a thousand into another bin than fp64 ones); the bin is taken from the `w2` the call reports.

    `n_fft` must be a power of two from 16 to 4096 (ValueError otherwise, before any GPU work).  Every (dtype, n_fft)
    in that range is built without register spills or scratch (profiles/sst2_resources.txt), so none is refused on
    those grounds."""
    lib = _lib.load()
    squeeze = _squeeze_code(squeezing)
    f = _stft_front(x, window, n_fft, win_len, hop_len, fs, t, "ssq_stft2")
    pad = _pad_code(padtype)
    _lib.require_gpu()
    shape = _stft_shape(f, hop_len)
    Tx, Sx = _lib.pinned_empty(shape, f.cdt), _lib.pinned_empty(shape, f.cdt)
    w2 = _lib.pinned_empty(shape, f.rdt) if get_w else None
    freqs = np.empty(f.n_freqs, dtype=np.float64)
    _call(lib.ssq_ssq_stft2_host(f.code, _ptr(f.xa), f.batch, f.N, _ptr(f.win), f.n_fft, hop_len, f.fs, pad,
                                 squeeze, _gamma_arg(gamma), _variant(modulated, flipud), _ptr(Tx),
                                 _ptr(freqs), _ptr(Sx), _ptr(w2)))
    return (*_unbatch(f.batched, Tx, Sx), freqs.astype(f.rdt), _Sfs(f), *_unbatch(f.batched, w2))


MSST_MAX_ITER = 64                      # csrc/stft_msst.hip: kWalkMaxIter, a bound on work (not a measured number)
MSST_MAX_ROWS = 2049                    # csrc/stft_msst.hip: kWalkMaxRows, the rows of n_fft = 4096


def _n_iter(n_iter):
    if (not isinstance(n_iter, (int, np.integer)) or isinstance(n_iter, (bool, np.bool_))
            or not 1 <= n_iter <= MSST_MAX_ITER):
        raise ValueError(f"n_iter {n_iter!r}: an int from 1 to {MSST_MAX_ITER}")
    return int(n_iter)


def mssq_stft(x, window=None, n_fft=None, win_len=None, hop_len=1, fs=None, t=None, modulated=True, padtype="reflect",
              squeezing="sum", gamma=None, flipud=False, order=2, n_iter=4, get_w=False, get_bins=False):
    """Multisynchrosqueezed STFT -> (Tx, Sx, ssq_freqs, Sfs[, w][, bins]); not in upstream (Yu, Wang and Zhao 2019),
    conventions of `ssq_stft2`.  Where `ssq_stft2` applies its frequency map once, this asks the map again at the bin a
    coefficient landed on, `n_iter` steps in all: on a signal whose modulation is not linear inside the window the
    one-step estimate taken off the ridge is biased, and the estimate taken where it points is closer.

    Per column, with F = n_fft // 2 + 1 rows, let m[k] be the one-step bin of row k: the clamped round-half-even bin of
    the reported frequency `w` on np.linspace(0, fs / 2, F) (the rule of `ssq_stft2`), taken in the call's dtype from the
    `w` the call reports and before any `flipud`; m[k] = -1 where the bin is not kept (|V| <= gamma).  `order=2` uses the
    w2 of `ssq_stft2`, including its fallback to w1 where |D| <= gamma^2; `order=1` uses fs |Re w1| on every bin (it runs
    the same three transforms as order 2 and costs the same).  The walk:
        c1[k] = m[k]
        c(i+1)[k] = m[ci[k]]  if ci[k] >= 0 and m[ci[k]] >= 0,  else ci[k]          (i = 1 .. n_iter - 1)
    A chain stops on a bin that has no map of its own and on a fixed point; a cycle keeps turning until `n_iter` runs
    out.  Then, for every kept k, rows ascending inside a column, in the call's dtype and without atomics:
        Tx[r(c_n[k]), j] += Sx[k, j] dw  ('sum')    or    dw / F  ('lebesgue');        r(b) = F - 1 - b under `flipud`, else b
    `n_iter=1`, `order=2` is `ssq_stft2` bit for bit.  Coefficients move along frequency only and keep their phase, so
    every column keeps its sum: `issq_stft`, `extract_ridges` and the component inversion take `Tx` unchanged.

    `Sx` equals `stft(x, ...)`; `w` (get_w=True) is the ONE-step frequency map, +inf where a bin is not kept; `bins`
    (get_bins=True) is int32: the row of `Tx` each coefficient went to, -1 where it was not kept.  `msst_walk` runs the
    walk alone on a map the caller holds.

    `n_fft` must be a power of two from 16 to 4096, `order` 1 or 2, `n_iter` an int from 1 to 64 (a bound on work: the
    model signals of DESIGN 4.17 stopped moving by 32) and `squeezing` 'sum' or 'lebesgue' (ValueError otherwise, before
    any GPU work).  The walk runs out of LDS, a tile of columns at a time (csrc/stft_msst.hip); its kernel and every
    instantiation of the operator are built without register spills or scratch (profiles/msst_resources.txt,
    profiles/sst2_resources.txt)."""
    lib = _lib.load()
    order = _order12(order, "mssq_stft builds orders 1 and 2")
    n_iter = _n_iter(n_iter)
    squeeze = _squeeze_code(squeezing)
    f = _stft_front(x, window, n_fft, win_len, hop_len, fs, t, "mssq_stft")
    pad = _pad_code(padtype)
    _lib.require_gpu()
    shape = _stft_shape(f, hop_len)
    Tx, Sx = _lib.pinned_empty(shape, f.cdt), _lib.pinned_empty(shape, f.cdt)
    w = _lib.pinned_empty(shape, f.rdt) if get_w else None
    bins = _lib.pinned_empty(shape, np.int32) if get_bins else None
    freqs = np.empty(f.n_freqs, dtype=np.float64)
    _call(lib.ssq_mssq_stft_host(f.code, _ptr(f.xa), f.batch, f.N, _ptr(f.win), f.n_fft, hop_len, f.fs, pad,
                                 squeeze, _gamma_arg(gamma), _variant(modulated, flipud), order, n_iter,
                                 _ptr(Tx), _ptr(freqs), _ptr(Sx), _ptr(w), _ptr(bins)))
    return (*_unbatch(f.batched, Tx, Sx), freqs.astype(f.rdt), _Sfs(f), *_unbatch(f.batched, w, bins))


def msst_walk(bins, n_iter):
    """The walk of `mssq_stft` alone, on a map the caller holds -> int32, same shape.  `bins`: int32 [F, n] or
    [B, F, n] (F <= 2049), a target indexes the row axis itself and -1 means no map; per column
        c1[k] = bins[k];   c(i+1)[k] = bins[ci[k]] if ci[k] >= 0 and bins[ci[k]] >= 0, else ci[k]     (i = 1 .. n_iter - 1)
    and the result is c_n.  Runs the kernel of `mssq_stft` (csrc/stft_msst.hip); a non-int32 array, targets outside
    -1 .. F - 1 and an `n_iter` that is not an int from 1 to 64 raise ValueError before any GPU work."""
    lib = _lib.load()
    n_iter = _n_iter(n_iter)
    if not isinstance(bins, np.ndarray) or bins.dtype != np.int32 or bins.ndim not in (2, 3):
        raise ValueError("`bins` must be an int32 ndarray [F, n] or [B, F, n]")
    b3 = np.ascontiguousarray(bins if bins.ndim == 3 else bins[None])
    B, F, n = b3.shape
    if not 1 <= F <= MSST_MAX_ROWS or B < 1 or n < 1:
        raise ValueError(f"`bins` of shape {bins.shape}: 1 .. {MSST_MAX_ROWS} rows, and no empty axis")
    if b3.min() < -1 or b3.max() >= F:
        raise ValueError(f"`bins` holds targets outside -1 .. F - 1 = {F - 1}")
    _lib.require_gpu()
    out = np.empty_like(b3)
    _call(lib.ssq_msst_walk_host(_ptr(b3), B, F, n, n_iter, _ptr(out)))
    return _unbatch(bins.ndim == 3, out)[0]


def msst_tile_cols(n_rows):
    """Columns of the LDS tile one workgroup of the walk kernel owns for maps of `n_rows` rows (no GPU needed)."""
    c = _lib.load().ssq_msst_tile_cols(int(n_rows))
    if c < 0:
        raise ValueError(f"n_rows {n_rows!r}: 1 .. {MSST_MAX_ROWS}")
    return int(c)


LMSST_MAX_DELTA = 256                   # csrc/stft_lmsst.hip: kLmsstMaxDelta, a bound on work (not a measured number)
LMSST_LOBE_LEVEL = 1e-3                 # where a main lobe counts as over: 60 dB down -- part of the definition, not measured


def _delta(delta, n_rows, default):
    """`delta` checked: None asks `default()`; an int from 1 to min(n_rows - 1, 256)."""
    if delta is None:
        delta = default()
    top = min(n_rows - 1, LMSST_MAX_DELTA)
    if not isinstance(delta, (int, np.integer)) or isinstance(delta, (bool, np.bool_)) or not 1 <= delta <= top:
        raise ValueError(f"delta {delta!r}: an int from 1 to min(rows - 1, {LMSST_MAX_DELTA}) = {top}")
    return int(delta)


def lmsst_default_delta(window, n_fft):
    """The default `delta` of `lmssq_stft`: the half-width in rows of the window's main lobe.  With G = |rfft(g)| of the
    window sized to `n_fft` (`get_window`) and F = n_fft // 2 + 1, the smallest d >= 1 with G[d] <= 1e-3 G[0] (the lobe has
    fallen 60 dB) or G[d + 1] >= G[d] (the lobe has ended); F - 1 if there is none; at most 256.  The 1e-3 is part of the
    definition, not a measurement.  numpy on the host, no GPU."""
    if not isinstance(window, np.ndarray):
        raise ValueError("`window` must be an ndarray")
    g = get_window(window, len(window), int(n_fft))
    G = np.abs(np.fft.rfft(g, int(n_fft)))
    F = len(G)
    d = F - 1
    for k in range(1, F - 1):
        if G[k] <= LMSST_LOBE_LEVEL * G[0] or G[k + 1] >= G[k]:
            d = k
            break
    return int(max(1, min(d, F - 1, LMSST_MAX_DELTA)))


def lmssq_stft(x, window=None, n_fft=None, win_len=None, hop_len=1, fs=None, t=None, modulated=True, padtype="reflect",
               squeezing="sum", gamma=None, flipud=False, delta=None, get_bins=False):
    """Local maximum synchrosqueezed STFT -> (Tx, Sx, ssq_freqs, Sfs[, bins]); not in upstream (Yu, Wang, Zhao and Liu
    2019), conventions of `mssq_stft`.  Where the rest of the family moves a coefficient to the frequency that a quotient
    of STFTs estimates, this moves it to the row where |Sx| has its maximum inside a window of +- `delta` rows.  It needs
    no derivative of the window (no g', t g or g''): ONE transform per frame against the three of `ssq_stft2`, any window,
    and a target that is an argmax, not a ratio, which degrades slowest under noise.

    Per column, with F = n_fft // 2 + 1 rows and an int `delta` >= 1:
        A[k] = re^2 + im^2 of Sx[k] as the call reports it (rounded to the call's dtype), evaluated in fp64 with the two
               products and the sum rounded one by one (numpy's re*re + im*im on float64, bit for bit)
        m[k] = the row of the maximum of A over rows max(0, k - delta) .. min(F - 1, k + delta), scanned ascending and
               taken only where strictly greater, so the lowest row wins a tie; rows that are not kept take part
    A cell is kept where |V| > gamma on the fp64 coefficient (default 10 eps of the dtype; `ssq_stft2`'s rule).  Then, for
    every kept k, rows ascending inside a column, in the call's dtype and without atomics (`mssq_stft`'s accumulation):
        Tx[r(m[k]), j] += Sx[k, j] dw  ('sum')    or    dw / F  ('lebesgue');        r(b) = F - 1 - b under `flipud`, else b
    A kept k always has a kept target (A[m[k]] >= A[k]).  Coefficients move along frequency only and keep their phase, so
    every column keeps its sum: `issq_stft`, `extract_ridges` and the component inversion take `Tx` unchanged.

    `Sx` equals `stft(x, ...)` up to the rounding of another FFT arrangement (a real-input transform, not `ssq_stft2`'s
    packed pair); `bins` (get_bins=True) is int32: the row of `Tx` each coefficient went to, -1 where it was not kept.
    float32 in gives complex64 out; the transform runs in fp64 for either dtype.

    `delta=None` asks for `lmsst_default_delta(window, n_fft)`, the half-width of the window's main lobe (its 1e-3 level is
    part of the definition, not a measurement); else an int from 1 to min(F - 1, 256) -- 256 is a bound on work, not a
    measured number.  `delta = F - 1` sends every kept cell of a column to the column's largest row.

    The limit: LMSST puts energy on the SPECTROGRAM's ridge, which on a fast FM is not the instantaneous frequency (on the
    FM model of DESIGN 4.25, 56 % of the energy lies within one bin of the true frequency where `ssq_stft2` has 85 %).  It
    complements the second-order transforms and does not replace them.

    `n_fft` must be a power of two from 16 to 4096 and `squeezing` 'sum' or 'lebesgue'; a bool, a float or an
    out-of-range `delta` is refused (ValueError, before any GPU work).  One kernel decides a column in LDS and writes every
    cell of `Tx` once (csrc/stft_lmsst.hip); every (dtype, n_fft) is built without register spills or scratch
    (profiles/lmsst_resources.txt)."""
    lib = _lib.load()
    squeeze = _squeeze_code(squeezing)
    f = _stft_front(x, window, n_fft, win_len, hop_len, fs, t, "lmssq_stft")
    pad = _pad_code(padtype)
    delta = _delta(delta, f.n_freqs, lambda: lmsst_default_delta(f.win, f.n_fft))
    _lib.require_gpu()
    shape = _stft_shape(f, hop_len)
    Tx, Sx = _lib.pinned_empty(shape, f.cdt), _lib.pinned_empty(shape, f.cdt)
    bins = _lib.pinned_empty(shape, np.int32) if get_bins else None
    freqs = np.empty(f.n_freqs, dtype=np.float64)
    _call(lib.ssq_lmssq_stft_host(f.code, _ptr(f.xa), f.batch, f.N, _ptr(f.win), f.n_fft, hop_len, f.fs, pad, squeeze,
                                  _gamma_arg(gamma), _variant(modulated, flipud), delta, _ptr(Tx), _ptr(freqs), _ptr(Sx),
                                  _ptr(bins)))
    return (*_unbatch(f.batched, Tx, Sx), freqs.astype(f.rdt), _Sfs(f), *_unbatch(f.batched, bins))


def tssq_stft(x, window=None, n_fft=None, win_len=None, hop_len=1, fs=None, t=None, modulated=True, padtype="reflect",
              order=2, gamma=None, get_tau=False):
    """Time-reassigned synchrosqueezed STFT -> (Tx, Sx, times, Sfs[, tau]); not in upstream (He, Tu, Bao, Hu and Zhang
    2019), conventions of `ssq_stft2`.  Where `ssq_stft` and `ssq_stft2` move energy along frequency, this moves every
    coefficient along TIME to its estimated group delay: an impulse, a fast chirp or a dispersive arrival, whose ridge
    runs along frequency, lands on its own column.

    With n = n_fft, the five windows of `ssq_stft2` (g, its spectral derivatives g1 and g2, tg = u g, tg1 = u g1,
    u = sample index - n // 2), V, V1, V2, Vt, Vt1 the STFTs of `x` with them and frame m centred on sample m hop_len,
    per sample and in fp64 for either dtype:
        d1 = Re(Vt / V)          D = Vt V1 - Vt1 V          num = V2 V - V1^2          d2 = Re(Vt / V + V1 D / (V num))
    d1 is the first-order group-delay offset; d2 is the time at which the locally fitted linear chirp crosses frequency
    k / n, exact for linear group delay.  `order=2` uses d2 where |num| > gamma^2, d2 is finite and |d2| <= n / 2, else
    (and always with `order=1`, which computes V and Vt only) d1; the offset is clamped to [-n / 2, n / 2].  `tau`
    (get_tau=True) is offset / fs in seconds, relative to the frame's own time, +inf where a bin is not kept; bins with
    |V| > gamma (default 10 eps of the dtype) are kept.  The target column comes from the reported `tau` in its dtype:
        r = rint(tau / (hop_len / fs))  (0 where not finite)          m' = clip(m + r, 0, n_frames - 1)
        Tx[k, m'] += Sx[k, m] exp(-2 pi i ((k (m - m') hop_len) mod n) / n)
    The factor re-references the phase from the source frame's centre to the target's (the same for `modulated=False`):
    with it an impulse at t0 lands on column t0 with magnitude sum(g) in every row; without it its contributions cancel.
    Every cell is the sum of its contributions in ascending source frame (a compensated fp64 sum, no atomics), so the
    result does not depend on the batch or on the kernel's tiling.  `Sx` equals `stft(x, ...)`; `times` =
    arange(n_frames) hop_len / fs.  There is no inverse: for every row k
        sum_m' Tx[k, m'] e^(-2 pi i k m' hop_len / n)  =  sum_(kept m) Sx[k, m] e^(-2 pi i k m hop_len / n),
    the signal's spectrum at n_fft points, which determines it only modulo n_fft samples.

    `n_fft` must be a power of two from 16 to 4096 and `order` 1 or 2 (ValueError otherwise, before any GPU work).  Every
    (dtype, n_fft, order) is built without register spills or scratch (profiles/tsst_resources.txt)."""
    lib = _lib.load()
    order = _order12(order, "tssq_stft builds orders 1 and 2")
    f = _stft_front(x, window, n_fft, win_len, hop_len, fs, t, "tssq_stft")
    if gamma is not None and math.isnan(float(gamma)):
        raise ValueError("gamma is NaN")
    pad = _pad_code(padtype)
    _lib.require_gpu()
    shape = _stft_shape(f, hop_len)
    Tx, Sx = _lib.pinned_empty(shape, f.cdt), _lib.pinned_empty(shape, f.cdt)
    tau = _lib.pinned_empty(shape, f.rdt) if get_tau else None
    _call(lib.ssq_tssq_stft_host(f.code, _ptr(f.xa), f.batch, f.N, _ptr(f.win), f.n_fft, hop_len, f.fs, pad, order,
                                 _gamma_arg(gamma), _variant(modulated), _ptr(Tx), _ptr(Sx), _ptr(tau)))
    return (*_unbatch(f.batched, Tx, Sx), _times(f, hop_len), _Sfs(f), *_unbatch(f.batched, tau))


TMSST_MAX_REACH = 16384                 # csrc/stft_tsst.h: kTsstWideReach, the farthest a walked coefficient may land


def _tmsst_reach(n_iter, reach, what):
    if n_iter * reach > TMSST_MAX_REACH:
        raise ValueError(f"{what}: n_iter * reach = {n_iter} * {reach} exceeds {TMSST_MAX_REACH} (the final relative "
                         "target is an int16, and a tile of targets with both halos is staged in LDS)")


def tmssq_stft(x, window=None, n_fft=None, win_len=None, hop_len=1, fs=None, t=None, modulated=True, padtype="reflect",
               order=2, gamma=None, n_iter=4, get_tau=False, get_targets=False):
    """Time-reassigned multisynchrosqueezed STFT -> (Tx, Sx, times, Sfs[, tau][, targets]); not in upstream (Yu, Lin, Ma
    and He 2020), conventions of `tssq_stft`.  Where `tssq_stft` applies its time map once, this asks the map again at the
    frame a coefficient landed on, `n_iter` steps in all: on an impulsive or dispersive signal whose group delay is not
    linear inside the window the one-step estimate taken off the ridge is biased, and the estimate taken where it points
    is closer.  It is the dual of `mssq_stft`.

    Everything up to the one-step target is `tssq_stft`'s: the five windows, d1, d2 and the fallback, the clamp to
    +- n_fft / 2, `tau` in the call's dtype (+inf where |V| <= gamma), r = rint(tau / (hop_len / fs)), and for a kept bin
    t[k, m] = clip(m + r, 0, n_frames - 1).  Then, per row k, with H = ceil(n_fft / (2 hop_len)):
        c1[m] = t[m]
        c(i+1)[m] = t[ci[m]]  if bin (k, ci[m]) is kept,  else ci[m]                    (i = 1 .. n_iter - 1)
        Tx[k, c_n[m]] += Sx[k, m] exp(-2 pi i ((k (m - c_n[m]) hop_len) mod n_fft) / n_fft)     kept m, ascending source frame
    A chain stops on a frame whose bin in that row is not kept and on a fixed point; a cycle keeps turning until `n_iter`
    runs out.  The rotation takes the total displacement, so the per-row marginal identity of `tssq_stft` holds as it
    does there.  Every cell is the compensated fp64 sum of its contributions in ascending source frame, rounded once: no
    atomics, bitwise independent of the batch and of the tiling.  `n_iter=1` is `tssq_stft` bit for bit.  There is no
    inverse.

    `Sx` equals `stft(x, ...)`; `tau` (get_tau=True) is the ONE-step map, +inf where a bin is not kept; `targets`
    (get_targets=True) is int32: the frame of `Tx` each coefficient went to, -1 where it was not kept.  `tmsst_walk` runs
    the walk alone on a map the caller holds.

    `n_fft` must be a power of two from 16 to 4096, `order` 1 or 2, `n_iter` an int from 1 to 64, and n_iter H <= 16384
    (|c_n[m] - m| <= n_iter H: the final relative target is an int16, and a tile of targets with both halos is staged in
    LDS; n_fft 4096 at hop 1 allows n_iter <= 8); ValueError otherwise, before any GPU work.  The walk and both scatter
    stages are built without register spills or scratch (profiles/tmsst_resources.txt)."""
    lib = _lib.load()
    order = _order12(order, "tmssq_stft builds orders 1 and 2")
    n_iter = _n_iter(n_iter)
    f = _stft_front(x, window, n_fft, win_len, hop_len, fs, t, "tmssq_stft")
    if gamma is not None and math.isnan(float(gamma)):
        raise ValueError("gamma is NaN")
    pad = _pad_code(padtype)
    if isinstance(hop_len, (int, np.integer)) and hop_len >= 1:
        _tmsst_reach(n_iter, (f.n_fft // 2 - 1) // int(hop_len) + 1, "tmssq_stft")
    _lib.require_gpu()
    shape = _stft_shape(f, hop_len)
    Tx, Sx = _lib.pinned_empty(shape, f.cdt), _lib.pinned_empty(shape, f.cdt)
    tau = _lib.pinned_empty(shape, f.rdt) if get_tau else None
    targets = _lib.pinned_empty(shape, np.int32) if get_targets else None
    _call(lib.ssq_tmssq_stft_host(f.code, _ptr(f.xa), f.batch, f.N, _ptr(f.win), f.n_fft, hop_len, f.fs, pad, order,
                                  _gamma_arg(gamma), _variant(modulated), n_iter, _ptr(Tx), _ptr(Sx), _ptr(tau),
                                  _ptr(targets)))
    return (*_unbatch(f.batched, Tx, Sx), _times(f, hop_len), _Sfs(f), *_unbatch(f.batched, tau, targets))


def tmsst_walk(targets, n_iter, reach):
    """The walk of `tmssq_stft` alone, on a map the caller holds -> int32, same shape.  `targets`: int32 [F, n] or
    [B, F, n], a target indexes the frame axis itself and -1 means none; per row
        c1[m] = targets[m];   c(i+1)[m] = targets[ci[m]] if targets[ci[m]] >= 0, else ci[m]        (i = 1 .. n_iter - 1)
    and the result is c_n (-1 where targets[m] is).  `reach`: how far a target may lie from its own frame (the H of
    `tmssq_stft`).  Runs the kernel of `tmssq_stft` (csrc/stft_tmsst.hip); a non-int32 array, a kept target outside
    0 .. n - 1 or farther than `reach` from its frame, `reach < 1`, n_iter * reach > 16384 and an `n_iter` that is not an
    int from 1 to 64 raise ValueError before any GPU work."""
    lib = _lib.load()
    n_iter = _n_iter(n_iter)
    if not isinstance(reach, (int, np.integer)) or isinstance(reach, (bool, np.bool_)) or reach < 1:
        raise ValueError(f"reach {reach!r}: an int >= 1")
    _tmsst_reach(n_iter, int(reach), "tmsst_walk")
    if not isinstance(targets, np.ndarray) or targets.dtype != np.int32 or targets.ndim not in (2, 3):
        raise ValueError("`targets` must be an int32 ndarray [F, n] or [B, F, n]")
    t3 = np.ascontiguousarray(targets if targets.ndim == 3 else targets[None])
    B, F, n = t3.shape
    if B < 1 or F < 1 or n < 1:
        raise ValueError(f"`targets` of shape {targets.shape}: no empty axis")
    if t3.min() < -1 or t3.max() >= n:
        raise ValueError(f"`targets` holds targets outside -1 .. n - 1 = {n - 1}")
    if (np.abs(t3.astype(np.int64) - np.arange(n)) > reach)[t3 >= 0].any():
        raise ValueError(f"`targets` holds a target farther than reach = {reach} from its own frame")
    _lib.require_gpu()
    out = np.empty_like(t3)
    _call(lib.ssq_tmsst_walk_host(_ptr(t3), B, F, n, n_iter, int(reach), _ptr(out)))
    return _unbatch(targets.ndim == 3, out)[0]


def tmsst_tile_frames(reach, n_iter):
    """Target frames of the tile one workgroup of the walk kernel owns for one-step targets within `reach` frames walked
    `n_iter` steps (no GPU needed)."""
    c = _lib.load().ssq_tmsst_tile_frames(int(reach), int(n_iter))
    if c < 0:
        raise ValueError(f"reach {reach!r}, n_iter {n_iter!r}: reach >= 1, n_iter 1 .. {MSST_MAX_ITER}, "
                         f"n_iter * reach <= {TMSST_MAX_REACH}")
    return int(c)


def _extract_stft(name, axis, x, window, n_fft, win_len, hop_len, fs, t, modulated, padtype, order, gamma, get_Sx, get_map):
    """The body of `set_stft` (axis 0) and `tet_stft` (axis 1) -> (f, Te, Sx | None, map | None), batch axis dropped."""
    lib = _lib.load()
    order = _order12(order, f"{name} builds orders 1 and 2")
    f = _stft_front(x, window, n_fft, win_len, hop_len, fs, t, name)
    if gamma is not None and math.isnan(float(gamma)):
        raise ValueError("gamma is NaN")
    pad = _pad_code(padtype)
    _lib.require_gpu()
    shape = _stft_shape(f, hop_len)
    Te = _lib.pinned_empty(shape, f.cdt)
    Sx = _lib.pinned_empty(shape, f.cdt) if get_Sx else None
    mp = _lib.pinned_empty(shape, f.rdt) if get_map else None
    _call(lib.ssq_extract_stft_host(f.code, _ptr(f.xa), f.batch, f.N, _ptr(f.win), f.n_fft, hop_len, f.fs, pad, axis, order,
                                    _gamma_arg(gamma), _variant(modulated), _ptr(Te), _ptr(Sx), _ptr(mp)))
    unb = lambda a: None if a is None else (a if f.batched else a[0])                # noqa: E731
    return f, unb(Te), unb(Sx), unb(mp)


def set_stft(x, window=None, n_fft=None, win_len=None, hop_len=1, fs=None, t=None, modulated=True, padtype="reflect",
             order=2, gamma=None, get_Sx=True, get_w=False):
    """Synchroextracting STFT -> (Te, Sx | None, Sfs[, w]); not in upstream (Yu, Yu and Zhang 2017; second order: Bao et
    al. 2019), conventions of `ssq_stft2`.  Where the synchrosqueezed transforms MOVE a coefficient to the frequency it
    estimates, this KEEPS a coefficient only where its estimated instantaneous frequency is the frequency of its own
    row, and zeroes the rest: what is left is the ridge itself, unsmeared, with the STFT's own amplitudes and phases.

    With the five windows and STFTs of `ssq_stft2` (in fp64 for either dtype, on the widened signal) and F = n_fft // 2
    + 1 rows, a cell is live where |V| > gamma (default 10 eps of the dtype) and
        w = fs |Re w2| where order = 2, |D| > gamma^2 and Re w2 is finite, else fs |Re w1|       (`ssq_stft2`'s `w2`)
        w = fs |Re w1| on every cell for order = 1              (ONE transform, x (g + i g1), a third of order 2's work)
    rounded once to the call's dtype, +inf where the cell is not live (`w`, get_w=True).  With b the clamped
    round-half-even bin of the reported `w` on np.linspace(0, fs / 2, F), taken in the call's dtype (the rule of
    `ssq_stft2`):
        Te[k, m] = Sx[k, m]  where the cell is live and b == k,     else +0 + 0i.
    There is no `squeezing`, `flipud` or `ssq_freqs`: the rows of `Te` are the rows of `Sx`, at `Sfs`.  `Te` holds exactly
    the coefficients that `mssq_stft(order=order, n_iter=1)` leaves on their own row.  `Sx` (None with get_Sx=False,
    which saves its store and its copy) equals `stft(x, ...)`.  One kernel writes every cell exactly once, so signal b's
    bits do not depend on the batch.

    There is no inverse, and SET is not a reconstruction method for strongly modulated components (the ridge cells alone
    give back a fast chirp with a relative error of 0.5).  What stands in for one is the identity of a tone on a bin
    centre, (2 / sum(g)) Re sum_k c_k Te[k, m] = x[m] with c = 1/2 on rows 0 and F - 1 and 1 elsewhere, which holds to
    1e-8.

    `n_fft` must be a power of two from 16 to 4096 and `order` 1 or 2 (ValueError otherwise, before any GPU work).  Every
    (dtype, n_fft, order) is built without register spills or scratch (profiles/extract_resources.txt)."""
    f, Te, Sx, w = _extract_stft("set_stft", 0, x, window, n_fft, win_len, hop_len, fs, t, modulated, padtype, order, gamma,
                                 get_Sx, get_w)
    return (Te, Sx, _Sfs(f), *((w,) if get_w else ()))


def tet_stft(x, window=None, n_fft=None, win_len=None, hop_len=1, fs=None, t=None, modulated=True, padtype="reflect",
             order=2, gamma=None, get_Sx=True, get_tau=False):
    """Transient-extracting STFT -> (Te, Sx | None, times, Sfs[, tau]); not in upstream (Yu 2019), conventions of
    `tssq_stft`.  The dual of `set_stft`: it KEEPS a coefficient only where its estimated group delay is its own column,
    and zeroes the rest, so an impulse, a click or a dispersive arrival is left on the columns where it happens.

    With the windows and STFTs of `tssq_stft` (in fp64 for either dtype) a cell is live where |V| > gamma (default 10
    eps of the dtype) and `tau` (get_tau=True) is `tssq_stft`'s reported offset in seconds, in the call's dtype, +inf
    where the cell is not live: order = 2 uses d2 with its fallback to d1, clamped to +- n_fft / 2 samples; order = 1 uses
    d1 (ONE transform, x (g + i tg)).  With
        r = rint(tau / (hop_len / fs))  in the call's dtype,
        Te[k, m] = Sx[k, m]  where the cell is live and r == 0,     else +0 + 0i.
    r is the relative target BEFORE `tssq_stft`'s clip to the frame range: an edge cell that the clip would bring back
    onto itself is not kept.  `Te` holds exactly the coefficients that `tssq_stft` leaves on their own column for that
    reason (for frequency, the counterpart is `mssq_stft(order=order, n_iter=1)` and `set_stft`).  An isolated unit
    impulse at sample t0 is kept on column t0 / hop_len only, with |Te[k, t0]| = g[n_fft // 2] in every row.  `Sx` (None
    with get_Sx=False) equals `stft(x, ...)`; `times` = arange(n_frames) hop_len / fs.  One kernel writes every cell
    exactly once, so signal b's bits do not depend on the batch.

    There is no inverse (for a tone on a bin centre `set_stft` has an identity that stands in for one; a transient has
    none).

    `n_fft` must be a power of two from 16 to 4096 and `order` 1 or 2 (ValueError otherwise, before any GPU work).  Every
    (dtype, n_fft, order) is built without register spills or scratch (profiles/extract_resources.txt)."""
    f, Te, Sx, tau = _extract_stft("tet_stft", 1, x, window, n_fft, win_len, hop_len, fs, t, modulated, padtype, order,
                                   gamma, get_Sx, get_tau)
    return (Te, Sx, _times(f, hop_len), _Sfs(f), *((tau,) if get_tau else ()))


# csrc/stft_reassign.hip: kReassignQuantumLog2. `reassign_stft` accumulates |Sx|^2 in 64-bit fixed point with the quantum
# q = P 2^REASSIGN_QUANTUM_LOG2, P the smallest power of two >= the signal's max |Sx|^2.
REASSIGN_QUANTUM_LOG2 = -38


def reassign_stft(x, window=None, n_fft=None, win_len=None, hop_len=1, fs=None, t=None, modulated=True,
                  padtype="reflect", gamma=None, get_w=False, get_tau=False):
    """Reassigned spectrogram -> (Rx, Sx, times, Sfs[, w][, tau]); not in upstream (Kodera, Gendrin and de Villedary 1978;
    Auger and Flandrin 1995: `librosa.reassigned_spectrogram`, MATLAB's `spectrogram(..., 'reassigned')`), conventions
    of `tssq_stft`.  Where `ssq_stft` / `ssq_stft2` move STFT coefficients along frequency and `tssq_stft` along time,
    this moves every bin's ENERGY |Sx|^2 in both directions at once, to its instantaneous frequency and its group delay:
    ridges that run along time and ridges that run along frequency (a sweep with clicks on it) sharpen together.

    With n = n_fft, F = n // 2 + 1, g the sized window, g1 its spectral derivative (Nyquist term zeroed), tg = u g
    (u = sample index - n // 2), V, V1, Vt the STFTs of `x` with them and frame m centred on sample m hop_len, per sample
    and in fp64 for either dtype:
        w   = fs |k / n - Im(V1 / V) / (2 pi)|             (`ssq_stft2`'s first-order frequency)
        tau = clamp(Re(Vt / V), -n / 2, n / 2) / fs        (`tssq_stft`'s order-1 group-delay offset, seconds)
    each rounded once to the call's dtype; a bin is kept where |V| > gamma (default 10 eps of the dtype), and `w`
    (get_w=True) and `tau` (get_tau=True) are +inf where it is not.  The targets come from the reported maps, in their
    dtype:
        k' = `ssq_stft2`'s bin rule on w: clamped round-half-even on Sfs = np.linspace(0, fs / 2, F), no flip
        m' = clip(m + rint(tau / (hop_len / fs)), 0, n_frames - 1)
        Rx[k', m'] += |Sx[k, m]|^2                         (of the reported Sx, formed in fp64)
    First order only, on purpose: (m + tau, w) is the centroid of the smoothed Wigner distribution, which lies ON the
    line of a linear chirp for any window, so there is no chirp-rate bias to remove; the two second-order operators of
    `ssq_stft2` and `tssq_stft` do not compose (one is a frequency at the frame's time, the other a time at the row's
    frequency: the pair is off the line).

    `Rx` is real and non-negative, in the call's real dtype, and conserves energy: sum(Rx) = sum of |Sx|^2 over the kept
    bins.  It is accumulated in 64-bit fixed point with the quantum q = P 2^-38 (`REASSIGN_QUANTUM_LOG2`), P the smallest
    power of two >= the signal's max |Sx|^2 -- about 2^-38 of the signal's peak energy, roughly -114 dB: every
    contribution is rounded to a multiple of q, and the integer adds commute, so a cell's bits do not depend on the order
    of the adds, the kernel's tiling or the batch.  `Sx` equals `stft(x, ...)`; `times` = arange(n_frames) hop_len / fs.
    There is no inverse (the phase is gone).

    `n_fft` must be a power of two from 16 to 4096 (ValueError otherwise, and for a NaN `gamma` or an unknown `padtype`,
    before any GPU work).  Every (dtype, n_fft) is built without register spills or scratch
    (profiles/reassign_resources.txt)."""
    lib = _lib.load()
    f = _stft_front(x, window, n_fft, win_len, hop_len, fs, t, "reassign_stft")
    if gamma is not None and math.isnan(float(gamma)):
        raise ValueError("gamma is NaN")
    pad = _pad_code(padtype)
    _lib.require_gpu()
    shape = _stft_shape(f, hop_len)
    Rx, Sx = _lib.pinned_empty(shape, f.rdt), _lib.pinned_empty(shape, f.cdt)
    w = _lib.pinned_empty(shape, f.rdt) if get_w else None
    tau = _lib.pinned_empty(shape, f.rdt) if get_tau else None
    _call(lib.ssq_reassign_stft_host(f.code, _ptr(f.xa), f.batch, f.N, _ptr(f.win), f.n_fft, hop_len, f.fs, pad,
                                     _gamma_arg(gamma), _variant(modulated), _ptr(Rx), _ptr(Sx), _ptr(w), _ptr(tau)))
    return (*_unbatch(f.batched, Rx, Sx), _times(f, hop_len), _Sfs(f), *_unbatch(f.batched, w, tau))


def issq_stft(Tx, window=None, cc=None, cw=None, n_fft=None, win_len=None, hop_len=1, modulated=True):
    """ssqueezepy.issq_stft (old/ssqueezepy/_ssq_stft.py:139-198).  `cc`, `cw` None: the full inverse [N] in Tx's real
    dtype ([B, N] for a batched `Tx` [B, F, N]).  Otherwise the component inversion of `issq_cwt`, scaled by 2 / window[len(window) // 2]: float64
    [K + 1, N], or [B, K + 1, N] for a batched `Tx` [B, F, N]."""
    if not modulated:
        raise ValueError("inversion with `modulated == False` is unsupported.")
    if hop_len != 1:
        raise ValueError("inversion with `hop_len != 1` is unsupported.")
    comp = _component_args(Tx, cc, cw)
    if comp is None:
        _full_map(Tx, "Tx")
    n_fft = n_fft or (Tx.shape[-2] - 1) * 2
    win = get_window(window, win_len or n_fft, n_fft)
    scale = 2.0 / float(win[len(win) // 2])
    return _issq(Tx, scale) if comp is None else _issq_components(*comp, scale)


class _RowCountError(AssertionError, ValueError):
    """`icwt`'s row-count refusal: upstream's AssertionError (_cwt.py:398), and a ValueError like every other refusal."""


def _full_map(Tx, name):
    """The refusals of a full inverse's map, 2-D [F, N] or batched 3-D [B, F, N], before any GPU work."""
    if not isinstance(Tx, np.ndarray) or Tx.ndim not in (2, 3) or Tx.dtype not in (np.complex64, np.complex128):
        raise TypeError(f"`{name}` must be a 2D (or batched 3D [B, F, N]) complex64 / complex128 array")
    if Tx.ndim == 3 and Tx.shape[0] < 1:
        raise ValueError(f"`{name}` holds no signal (B == 0)")


def _issq(Tx, scale, row_scale=None):
    """scale * sum_rows row_scale[row] * Re Tx[row] -> [N], or [B, N] for a batched Tx (entry b bitwise the 2-D call)."""
    lib = _lib.load()
    _full_map(Tx, "Tx")
    code = _ccode(Tx.dtype)
    _lib.require_gpu()
    Tc = np.ascontiguousarray(Tx)
    rs = None if row_scale is None else np.ascontiguousarray(row_scale, dtype=np.float64)
    if Tx.ndim == 3:
        x = np.empty((Tc.shape[0], Tc.shape[2]), dtype=_rdtype(code))
        _call(lib.ssq_issq_batch_host(code, _ptr(Tc), Tc.shape[0], Tc.shape[1], Tc.shape[2], float(scale), _ptr(rs),
                                      _ptr(x)))
        return x
    x = np.empty(Tc.shape[1], dtype=_rdtype(code))
    _call(lib.ssq_issq_host(code, _ptr(Tc), Tc.shape[0], Tc.shape[1], float(scale), _ptr(rs), _ptr(x)))
    return x


def _component_args(Tx, cc, cw):
    """_ssq_cwt.py:406-417 (`_process_component_inversion_args`) and the shapes `_invert_components` (:381-403) works
    with -> None for the full inverse, else (Tx, cc, cw, batched): Tx [B, F, N], cc and cw [B, N, K] int32 values.
    A 1-D cc / cw (a [B, N] one for a batched Tx) is one component; both are cast with astype('int32') (floats
    truncate toward zero); cc must have one row per column of Tx; cw at least K columns, of which the first K are
    read, broadcast against cc as upstream's `cc[:, n] + cw[:, n]` broadcasts.  Raises before any GPU work."""
    if cc is None and cw is None:
        return None
    if cc is None or cw is None:
        raise ValueError("`cc` and `cw` must be passed together (both None: the full inverse)")
    if not isinstance(Tx, np.ndarray) or Tx.ndim not in (2, 3) or Tx.dtype not in (np.complex64, np.complex128):
        raise TypeError("`Tx` must be a 2D [F, N] (or batched 3D [B, F, N]) complex64 / complex128 array")
    batched = Tx.ndim == 3
    Tb = Tx if batched else Tx[None]
    B, F, N = Tb.shape
    lead = 1 if batched else 0

    def as_curves(a, name):
        a = np.asarray(a)
        if a.ndim == lead + 1:
            a = a[..., None]
        if a.ndim != lead + 2:
            raise ValueError(f"`{name}` must be {'2D [B, N] or 3D [B, N, K]' if batched else '1D [N] or 2D [N, K]'}"
                             f" (got shape {a.shape})")
        return a.astype("int32")
    cc, cw = as_curves(cc, "cc"), as_curves(cw, "cw")
    if cc.shape[:-1] != ((B, N) if batched else (N,)):
        raise ValueError(f"`cc` must have one row per column of `Tx` ({N}){' per signal' if batched else ''} "
                         f"(got shape {cc.shape})")
    K = cc.shape[-1]
    if K < 1:
        raise ValueError("`cc` must hold at least one component")
    if cw.shape[-1] < K:
        raise ValueError(f"`cw` must have at least as many columns as `cc` ({cw.shape[-1]} < {K})")
    try:
        cw = np.broadcast_to(cw[..., :K], cc.shape)
    except ValueError:
        raise ValueError(f"`cw` of shape {cw.shape} does not broadcast against `cc` of shape {cc.shape}") from None
    return Tb, cc, cw, batched


def _issq_components(Tb, cc, cw, batched, scale):
    """_ssq_cwt.py:381-403 (`_invert_components`) times `scale` on the GPU (issq_components.hip) -> float64
    [K + 1, N] (or [B, K + 1, N]): the band sums of Re Tx, then the remainder over the rows of no band."""
    lib = _lib.load()
    B, F, N = Tb.shape
    K = cc.shape[-1]
    code = _ccode(Tb.dtype)
    _lib.require_gpu()
    Tc = np.ascontiguousarray(Tb)
    cc64 = np.ascontiguousarray(cc, dtype=np.int64).reshape(B, N, K)
    cw64 = np.ascontiguousarray(cw, dtype=np.int64).reshape(B, N, K)
    x = np.empty((B, K + 1, N), dtype=np.float64)
    _call(lib.ssq_issq_components_host(code, _ptr(Tc), B, F, N, _ptr(cc64), _ptr(cw64), 0, K, float(scale), _ptr(x)))
    return _unbatch(batched, x)[0]


# ---------------------------------------------------------------------------------------------------- CWT family ----
def cwt(x, wavelet="gmw", scales="log-piecewise", fs=None, t=None, nv=32, l1_norm=True, derivative=False,
        padtype="reflect", rpadded=False, vectorized=True, astensor=True, cache_wavelet=None, order=0, average=None,
        nan_checks=None, patience=0):
    """ssqueezepy.cwt (old/ssqueezepy/_cwt.py:12-318) -> (Wx, scales[, dWx]).  `scales` must be an explicit array of any
    upstream grid ('log', 'log-piecewise', 'linear'; `process_scales(<string>, N, wavelet)` builds upstream's default
    grids, the strings themselves are not accepted); `vectorized`, `astensor`, `cache_wavelet`,
    `nan_checks`, `patience` select code paths with identical numbers upstream and are accepted and unused.
    `order` / `average`: an order set (tuple / list / range) gives higher-order GMWs as `cwt_higher_order` -- the mean
    over the orders, or a list of arrays (one per order) with `average=False`.  A bare int `order` other than 0 raises
    ValueError, as it always has here: `order=(k,)` or `cwt_higher_order(x, order=k)` computes order k."""
    if isinstance(order, (int, np.integer)) and not isinstance(order, (bool, np.bool_)) and order > 0:
        raise ValueError("`cwt`: a bare int `order` other than 0 is not accepted; pass `order=(k,)` or call "
                         "`cwt_higher_order(x, order=k)`")
    return _cwt(x, wavelet, scales, fs, t, nv, l1_norm, derivative, padtype, rpadded,
                _order_args(order, average, wavelet, l1_norm))


def cwt_higher_order(x, wavelet="gmw", order=1, average=None, astensor=True, **kw):
    """ssqueezepy.cwt_higher_order (old/ssqueezepy/_cwt.py:515-608) -> (Wx, scales[, dWx]); `kw` are `cwt`'s.
    Wx (and dWx) is the mean over the orders, or a list with one array per order (`average=False`)."""
    kw = dict(kw)
    for k in ("vectorized", "cache_wavelet", "nan_checks", "patience"):
        kw.pop(k, None)
    args = _order_args(order, average, wavelet, kw.get("l1_norm", True), higher=True)
    a = [kw.pop(k, d) for k, d in (("scales", "log-piecewise"), ("fs", None), ("t", None), ("nv", 32), ("l1_norm", True),
                                   ("derivative", False), ("padtype", "reflect"), ("rpadded", False))]
    if kw:
        raise TypeError(f"cwt_higher_order: unexpected keyword arguments {sorted(kw)}")
    return _cwt(x, wavelet, *a, args)


def _cwt(x, wavelet, scales, fs, t, nv, l1_norm, derivative, padtype, rpadded, order_args):
    lib = _lib.load()
    xa, batched, code = _signal(x)
    batch, N = xa.shape
    dt = _dt(fs, t, N)
    wcode, p0, p1 = _wavelet(wavelet)
    s = _scales(scales)[0]                                 # (`nv` is not read: an ndarray's own holds, _cwt.py:226-227)
    orders, average = order_args if order_args else ((0,), True)
    if all(k == 0 for k in orders) and (average or len(orders) == 1):
        order_args = None                                  # the order-0 wavelet itself: the plain table (code 2)
    polys = gmw_order_coefficients(p0, p1, orders, average) if order_args else None
    groups = 1 if polys is None else polys.shape[0]
    _lib.require_gpu()
    cols = p2up(N)[0] if rpadded else N
    shape = (batch, groups * len(s), cols)
    Wx = _lib.pinned_empty(shape, _cdtype(code))
    dWx = _lib.pinned_empty(shape, _cdtype(code)) if derivative else None
    if polys is None:
        _call(lib.ssq_cwt_host_v(code, _ptr(xa), batch, N, wcode, p0, p1, _ptr(s), len(s), dt, int(bool(l1_norm)),
                                 _pad_code(padtype), int(bool(rpadded)), VARIANT_UPSTREAM, _ptr(Wx), _ptr(dWx)))
    else:
        polys = np.ascontiguousarray(polys)
        _call(lib.ssq_cwt_host_gmwk(code, _ptr(xa), batch, N, p0, p1, _ptr(polys), polys.shape[1], groups, _ptr(s),
                                    len(s), dt, int(bool(l1_norm)), _pad_code(padtype), int(bool(rpadded)),
                                    VARIANT_UPSTREAM, _ptr(Wx), _ptr(dWx)))
    sc = s.astype(_rdtype(code))

    def split(A):                                          # [batch, groups * na, cols] -> per order, batch axis dropped
        A = A.reshape(batch, groups, len(s), cols)
        parts = [A[:, g] if batched else A[0, g] for g in range(groups)]
        return parts if groups > 1 else parts[0]
    Wx = split(Wx)
    dWx = split(dWx) if derivative else None
    return (Wx, sc, dWx) if derivative else (Wx, sc)


def _ssq_freqs(s, N, wcode, p0, p1, dt, maprange, scaletype, s_own=None, was_padded=True):
    """ssqueezing.py:218-290 (ascending); s_own: the scales in the caller's dtype (the transition of 'log-piecewise' is
    found on them, as upstream finds it on its `scales`); was_padded: centre frequencies on the p2up(N) grid, else on
    the N-point one (:301-304)."""
    na = len(s)
    n_grid = p2up(N)[0] if was_padded else N

    def peak_freq(scale):                                  # ssqueezing.py:301-310 (maprange 'peak')
        wc = C.c_double(0)
        _call(_lib.load().ssq_upstream_center_frequency(wcode, p0, p1, float(scale), n_grid, C.byref(wc)))
        return wc.value / (2 * np.pi) / dt
    if maprange == "maximal":
        fm, fM = 1 / (dt * N), 1 / (2 * dt)
    elif maprange == "peak":
        fm, fM = peak_freq(s[-1]), peak_freq(s[0])
    else:
        raise ValueError(f"maprange {maprange!r}: 'peak' and 'maximal' are built")
    if scaletype == "log-piecewise":
        idx = logscale_transition_idx(s if s_own is None else s_own)
        if idx is None:
            scaletype = "log"
        else:                                              # :253-279: exponential from fm to f1, then from f1 to fM
            f1 = peak_freq(s[idx])
            t1 = np.arange(0, na - idx - 1) / (na - 1)
            t2 = np.arange(na - idx - 1, na) / (na - 1)
            t1 = np.hstack([t1, t2[0]])

            def exp_fm(t, fmin, fmax):                     # :294-298 (_exp_fm)
                tmin, tmax = t.min(), t.max()
                a = (fmin ** tmax / fmax ** tmin) ** (1 / (tmax - tmin))
                b = fmax ** (1 / tmax) * (1 / a) ** (1 / tmax)
                return a * b ** t
            f = np.hstack([exp_fm(t1, fm, f1)[:-1], exp_fm(t2, f1, fM)])
            ssq_idx = logscale_transition_idx(f)
            if ssq_idx is None:
                raise Exception("couldn't find logscale transition index of generated `ssq_freqs`; something went "
                                "wrong")
            assert (na - ssq_idx) == idx, "{} != {}".format(na - ssq_idx, idx)
            return f
    if scaletype == "log":
        return fm * np.power(fM / fm, np.arange(na) / (na - 1))
    if scaletype == "linear":
        return np.linspace(fm, fM, na)
    raise ValueError(f"ssq_freqs {scaletype!r}: 'log', 'log-piecewise' and 'linear' are built")


def _row_const(s, scaletype, nv):
    """ssqueezing.py:122-133: the weight of every row, ln2 / nv (nv per row for 'log-piecewise', re-inferred from the
    array as :168-169 does) or (s[1] - s[0]) / s for 'linear'."""
    if scaletype == "log":
        return np.full(len(s), np.log(2) / nv)
    if scaletype == "log-piecewise":
        return np.ascontiguousarray(np.log(2) / np.asarray(nv, dtype=np.float64).reshape(-1))
    return np.ascontiguousarray((s[1] - s[0]) / s)


def _freq_type(ssq_freqs, cwt_scaletype, maprange, generate):
    """ssqueezing.py:172-194, the frequencies a transform is squeezed onto -> (f_asc float64 ascending, their scaletype,
    f_idx: their 'log-piecewise' transition or None).  A string names the type, None takes the scales' (this mirror has
    always binned exponential scales on 'log' frequencies) and `generate(scaletype)` makes them; an array has its type
    inferred."""
    if isinstance(ssq_freqs, np.ndarray):
        f_own = _own_dtype(ssq_freqs)
        scaletype, _ = infer_scaletype(f_own)                                                     # :193-194
        f_asc = np.ascontiguousarray(f_own, dtype=np.float64)
    elif ssq_freqs is None or isinstance(ssq_freqs, str):
        scaletype = ssq_freqs if isinstance(ssq_freqs, str) else cwt_scaletype
        if scaletype == "log-piecewise" and maprange == "maximal":
            raise ValueError("can't have `ssq_scaletype = log-piecewise` or tuple with `maprange = 'maximal'` "
                             "(got %s)" % str(maprange))                                          # :181-184
        f_asc = f_own = np.ascontiguousarray(generate(scaletype), dtype=np.float64)   # (in float64, as upstream's)
    else:
        raise ValueError("`ssq_freqs` must be None, 'log', 'log-piecewise', 'linear' or an array")
    # algos.py:356-370: the two-segment rule at the frequencies' transition, found in their own dtype; none: one segment
    f_idx = logscale_transition_idx(f_own) if scaletype == "log-piecewise" else None
    if scaletype == "log-piecewise" and f_idx is None:
        scaletype = "log"
    return f_asc, scaletype, f_idx


def _cwt_freq_grid(scales, nv, ssq_freqs, maprange, N, wcode, p0, p1, dt):
    """The scale and frequency grids of `ssq_cwt` / `ssq_cwt2` -> (s float64 [na], row_const, f_asc float64 ascending,
    scaletype of the frequencies, f_idx: their 'log-piecewise' transition or None).  Every refusal of the two grids."""
    s, cwt_scaletype, _nv, s_own = _scales(scales)
    if cwt_scaletype == "log" and nv is not None and nv != _nv:
        raise Exception("`nv` used in `scales` differs from `nv` passed (%s != %s)" % (_nv, nv))
    row_const = _row_const(s, cwt_scaletype, _nv)
    if isinstance(ssq_freqs, np.ndarray) and ssq_freqs.size != len(s):
        raise ValueError("`ssq_freqs` must have one frequency per scale (%s != %s)" % (ssq_freqs.size, len(s)))
    f_asc, scaletype, f_idx = _freq_type(ssq_freqs, cwt_scaletype, maprange, lambda scaletype: _ssq_freqs(
        s, N, wcode, p0, p1, dt, maprange, scaletype, s_own))
    return s, row_const, f_asc, scaletype, f_idx


def _cwt_front(x, wavelet, scales, fs, t, gamma, padtype):
    """The front end of `ssq_cwt2`, `reassign_cwt`, `tssq_cwt` and `conceft_cwt`: the signal, the sampling period, the
    wavelet and the checks on them, on `scales`, `gamma` and `padtype` that all four make before their grids."""
    f = SimpleNamespace()
    f.xa, f.batched, f.code = _signal(x)
    f.batch, f.N = f.xa.shape
    if f.N < 2:
        raise ValueError("`x` must hold at least 2 samples")
    f.dt = _dt(fs, t, f.N)
    if not (f.dt > 0 and math.isfinite(f.dt)):
        raise ValueError("`fs` / `t` must give a positive sampling period")
    f.wcode, f.p0, f.p1 = _wavelet(wavelet)
    if not f.p0 > 0 or (f.wcode == WAVELET["gmw"] and not f.p1 > 0):
        raise ValueError(f"wavelet {wavelet!r}: the parameters must be positive")
    if isinstance(scales, np.ndarray) and scales.dtype.kind in "fiu" and not (np.isfinite(scales).all() and (scales > 0).all()):
        raise ValueError("`scales` must be positive and finite")
    if gamma is not None and math.isnan(float(gamma)):
        raise ValueError("`gamma` is NaN")
    f.gamma, f.pad = _gamma_arg(gamma), _pad_code(padtype)
    f.cdt, f.rdt = _cdtype(f.code), _rdtype(f.code)
    return f


def _finite_freq_grid(f, scales, nv, ssq_freqs, maprange):
    """`_cwt_freq_grid` for a front end's signal and wavelet, refusing frequencies that are not finite."""
    grid = _cwt_freq_grid(scales, nv, ssq_freqs, maprange, f.N, f.wcode, f.p0, f.p1, f.dt)
    if not np.isfinite(grid[2]).all():
        raise ValueError("`ssq_freqs` must be finite")
    return grid


def ssq_cwt(x, wavelet="gmw", scales="log-piecewise", nv=None, fs=None, t=None, ssq_freqs=None, padtype="reflect",
            squeezing="sum", maprange="peak", difftype="trig", difforder=None, gamma=None, vectorized=True,
            preserve_transform=None, astensor=True, order=0, nan_checks=None, patience=0, flipud=True,
            cache_wavelet=None, get_w=False, get_dWx=False):
    """ssqueezepy.ssq_cwt (old/ssqueezepy/_ssq_cwt.py:12-311) -> (Tx, Wx, ssq_freqs, scales[, w][, dWx])."""
    lib = _lib.load()
    if difftype != "trig":
        raise ValueError("only difftype='trig' is built")
    squeeze = _squeeze_code(squeezing)
    # _ssq_cwt.py:228-241: Wx of the order (set) averaged, dWx by `trigdiff` of the padded Wx -- the derivative transform of
    # the averaged wavelet up to rounding; ssq_freqs below stay the order-0 wavelet's (ssqueeze gets `wavelet` itself)
    order_args = _order_args(order, isinstance(order, (tuple, list, range)), wavelet)
    if order_args and all(k == 0 for k in order_args[0]):
        order_args = None
    xa, batched, code = _signal(x)
    batch, N = xa.shape
    dt = _dt(fs, t, N)
    wcode, p0, p1 = _wavelet(wavelet)
    s, row_const, f_asc, scaletype, f_idx = _cwt_freq_grid(scales, nv, ssq_freqs, maprange, N, wcode, p0, p1, dt)
    _lib.require_gpu()
    shape = (batch, len(s), N)
    cdt = _cdtype(code)
    Tx, Wx = _lib.pinned_empty(shape, cdt), _lib.pinned_empty(shape, cdt)
    dWx = _lib.pinned_empty(shape, cdt) if get_dWx else None
    wk = _lib.pinned_empty(shape, cdt) if get_w else None
    variant = VARIANT_UPSTREAM | (VARIANT_FLIPUD if flipud else 0)
    g = _gamma_arg(gamma)
    if order_args is None:
        _call(lib.ssq_ssq_cwt_host_rows(code, _ptr(xa), batch, N, wcode, p0, p1, _ptr(s), len(s), dt, _ptr(row_const),
                                        _ptr(f_asc), FREQS[scaletype], f_idx or 0, _pad_code(padtype),
                                        squeeze, g, variant, _ptr(Tx), _ptr(Wx), _ptr(dWx), _ptr(wk)))
    else:
        poly = np.ascontiguousarray(gmw_order_coefficients(p0, p1, *order_args))
        _call(lib.ssq_ssq_cwt_host_gmwk_rows(code, _ptr(xa), batch, N, p0, p1, _ptr(poly), poly.shape[1], 1, _ptr(s),
                                             len(s), dt, _ptr(row_const), _ptr(f_asc), FREQS[scaletype], f_idx or 0,
                                             _pad_code(padtype), squeeze, g, variant, _ptr(Tx), _ptr(Wx),
                                             _ptr(dWx), _ptr(wk)))
    rdt = _rdtype(code)
    w = wk.real.copy() if get_w else None
    return (*_unbatch(batched, Tx, Wx), f_asc[::-1].astype(rdt), s.astype(rdt),                # ssqueezing.py:199-205
            *_unbatch(batched, w, dWx))


def ssq_cwt2(x, wavelet="gmw", scales="log-piecewise", nv=None, fs=None, t=None, ssq_freqs=None, padtype="reflect",
             squeezing="sum", maprange="peak", gamma=None, flipud=True, get_w=False):
    """Second-order ("vertical") synchrosqueezed CWT -> (Tx, Wx, ssq_freqs, scales[, w2]); not in upstream (Oberlin and
    Meignen 2017), conventions of `ssq_cwt`.

    Per sample, with P, n1, n2 = p2up(N), xh the DFT of the padded signal, xi_k = 2 pi k / P for k <= P/2 (analytic
    tables: zero above) and, for scale a, T0 = psih(a xi), T1 = a psih'(a xi) in fp64 (both halved at 2k == P):
        W = F^-1[xh T0]   W1 = F^-1[xh i xi T0]   W2 = F^-1[xh (-xi^2) T0]   Wt = F^-1[xh (-i) T1]   Wt1 = F^-1[xh xi T1]
        D = W^2 + Wt1 W - Wt W1      c = (W2 W - W1^2) / D      om1 = W1 / W      om2 = om1 - c Wt / W
    A bin's frequency is |Im om2| / (2 pi dt) where |D| > gamma^2 and Im om2 is finite, else |Im om1| / (2 pi dt)
    (`ssq_cwt`'s w), and +inf where |W| < gamma (default 10 eps of the dtype).  For a signal whose logarithm is
    quadratic in time (a Gaussian-modulated linear chirp) Im om2 is the instantaneous frequency for any wavelet, where
    the first-order w is biased by the chirp rate times the wavelet's time spread.  `Wx` is W, upstream's L1-normalised
    `cwt`; `Tx` is `ssqueeze(Wx, w2, ...)`: every column's rows in ascending order, no atomics (the result does not
    depend on the batch), upstream's row weights, so `issq_cwt`, `extract_ridges` and the component inversion take it
    unchanged.  `w2` (get_w=True) is real, +inf where a bin is not kept.

    float32 in gives complex64 / float32 out, but the transforms and the operator run in fp64 for either dtype (the
    operator is a quotient of two differences of products); `Wx` and `w2` are rounded once and the scatter runs in the
    call's dtype on the rounded values.

    Built: wavelets 'gmw' (order 0, bandpass norm) and 'morlet'; an ndarray `scales` of any of the three grids;
    `ssq_freqs` None, a string or an array; maprange 'peak' / 'maximal'; 'sum' / 'lebesgue'; the five padtypes; 1-D or
    batched 2-D `x`.  Anything else raises ValueError before any GPU work."""
    lib = _lib.load()
    squeeze = _squeeze_code(squeezing)
    f = _cwt_front(x, wavelet, scales, fs, t, gamma, padtype)
    s, row_const, f_asc, scaletype, f_idx = _finite_freq_grid(f, scales, nv, ssq_freqs, maprange)
    _lib.require_gpu()
    shape = (f.batch, len(s), f.N)
    Tx, Wx = _lib.pinned_empty(shape, f.cdt), _lib.pinned_empty(shape, f.cdt)
    w2 = _lib.pinned_empty(shape, f.rdt) if get_w else None
    _call(lib.ssq_ssq_cwt2_host(f.code, _ptr(f.xa), f.batch, f.N, f.wcode, f.p0, f.p1, _ptr(s), len(s), f.dt,
                                _ptr(row_const), _ptr(f_asc), FREQS[scaletype], f_idx or 0, f.pad, squeeze,
                                f.gamma, VARIANT_FLIPUD if flipud else 0, 0, _ptr(Tx), _ptr(Wx), _ptr(w2)))
    return (*_unbatch(f.batched, Tx, Wx), f_asc[::-1].astype(f.rdt), s.astype(f.rdt), *_unbatch(f.batched, w2))


REASSIGN_CWT_QUANTUM_LOG2_MAX = 38      # csrc/cwt_reassign.hip: kCwtRQuantumBitsMax
REASSIGN_CWT_MAX_CELLS = 1 << 40        # na * N of one signal


def reassign_cwt_quantum_log2(na, N):
    """log2 of `reassign_cwt`'s quantum relative to Pmax, the smallest power of two >= the signal's max |Wx|^2:
    -min(38, 62 - L) with L = ceil(log2(na N)).  A contribution is at most 2^min(38, 62 - L) quanta and a cell takes at
    most na N <= 2^L of them, so a cell stays below 2^62."""
    cells = int(na) * int(N)
    if cells < 1:
        raise ValueError("`na` and `N` must be positive")
    L = (cells - 1).bit_length()
    return -min(REASSIGN_CWT_QUANTUM_LOG2_MAX, 62 - L)


def reassign_cwt(x, wavelet="gmw", scales="log-piecewise", nv=None, fs=None, t=None, ssq_freqs=None, padtype="reflect",
                 maprange="peak", gamma=None, flipud=True, get_w=False, get_tau=False, get_targets=False):
    """Reassigned scalogram -> (Rx, Wx, ssq_freqs, scales[, w][, tau][, kk, mm]); not in upstream (Auger and Flandrin
    1995, III), conventions of `ssq_cwt2`.  Where `ssq_cwt` / `ssq_cwt2` move CWT coefficients along frequency, this
    moves every coefficient's ENERGY |Wx|^2 along frequency and time at once, to its instantaneous frequency and its
    group delay: a click's cone, which widens with scale in the scalogram and in both synchrosqueezed CWTs, collapses
    onto the click's own column, and a sweep sharpens as under `ssq_cwt`.

    Per sample, with P, n1, n2 = p2up(N), xh, xi_k, T0 and T1 those of `ssq_cwt2`, in fp64 for either dtype:
        W = F^-1[xh T0]     W1 = F^-1[xh i xi T0]     Wt = F^-1[xh (-i) T1]        (columns n1 .. n1 + N - 1)
        w   = |Im(W1 / W)| / (2 pi dt)                     (`ssq_cwt`'s first-order frequency)
        tau = clamp(Re(Wt / W), -N, N) dt                  (the group-delay offset, seconds; t0 - b for an impulse at t0)
    each rounded once to the call's dtype; a bin is kept unless |W| < gamma (default 10 eps of the dtype), and `w`
    (get_w=True) and `tau` (get_tau=True) are +inf where it is not.  The targets come from the reported maps, in their
    dtype:
        k' = `ssqueeze`'s bin rule on w, on the `ssq_freqs` grid ('log', 'linear', 'log-piecewise'), flipped by `flipud`
        m' = clip(j + rint(tau / dt), 0, N - 1)
        Rx[k', m'] += |Wx[i, j]|^2                         (of the reported Wx, formed in fp64; no row weights)
    `kk`, `mm` (get_targets=True) are the int32 maps of k' and m', -1 where a bin is not kept.

    First order only, on purpose, for `reassign_stft`'s reason: (b + tau, w) is the centroid of the signal's smoothed
    Wigner distribution (here the affine smoothing by the wavelet's), which lies ON the line of a linear chirp, so there
    is no chirp-rate bias to remove; the second-order operators of `ssq_cwt2` (a frequency at the column's time) and its
    time counterpart (a time at the row's frequency) do not compose: the pair is off the line.

    `Rx` is real and non-negative, in the call's real dtype, and conserves energy: sum(Rx) = sum of |Wx|^2 over the kept
    bins.  It is accumulated by 64-bit integer atomic adds in device memory, in fixed point with the quantum
    q = Pmax 2^`reassign_cwt_quantum_log2(na, N)`, Pmax the smallest power of two >= the signal's max |Wx|^2: every
    contribution is rounded to a multiple of q, and the integer adds commute, so a cell's bits depend neither on the
    order of the adds, nor on the chunking, nor on the batch.  A signal of zeros gives an all-zero `Rx`; so does one with
    a non-finite sample (its `Wx`, `w` and `tau` are NaN and no energy is defined).  `Wx` equals `ssq_cwt2`'s.  There is
    no inverse (the phase is gone).

    Built: what `ssq_cwt2` builds (wavelets 'gmw' order 0 and 'morlet'; an ndarray `scales` of any of the three grids;
    `ssq_freqs` None, a string or an array; maprange 'peak' / 'maximal'; the five padtypes; 1-D or batched 2-D `x`) with
    na N <= 2^40.  Anything else raises ValueError before any GPU work."""
    lib = _lib.load()
    f = _cwt_front(x, wavelet, scales, fs, t, gamma, padtype)
    s, _, f_asc, scaletype, f_idx = _finite_freq_grid(f, scales, nv, ssq_freqs, maprange)
    _shape_checked(lib, lib.ssq_reassign_cwt_workspace_bytes(f.code, f.batch, f.N, len(s), None))
    _lib.require_gpu()
    shape = (f.batch, len(s), f.N)
    Rx, Wx = _lib.pinned_empty(shape, f.rdt), _lib.pinned_empty(shape, f.cdt)
    w = _lib.pinned_empty(shape, f.rdt) if get_w else None
    tau = _lib.pinned_empty(shape, f.rdt) if get_tau else None
    kk, mm = (_lib.pinned_empty(shape, np.int32) for _ in range(2)) if get_targets else (None, None)
    _call(lib.ssq_reassign_cwt_host(f.code, _ptr(f.xa), f.batch, f.N, f.wcode, f.p0, f.p1, _ptr(s), len(s), f.dt,
                                    _ptr(f_asc), FREQS[scaletype], f_idx or 0, f.pad, f.gamma,
                                    VARIANT_FLIPUD if flipud else 0, 0, _ptr(Rx), _ptr(Wx), _ptr(w), _ptr(tau), _ptr(kk),
                                    _ptr(mm)))
    return (*_unbatch(f.batched, Rx, Wx), f_asc[::-1].astype(f.rdt), s.astype(f.rdt),
            *_unbatch(f.batched, w, tau, kk, mm))


TSSQ_CWT_QUANTUM_LOG2_MAX = 38          # csrc/cwt_tsst.hip: kCwtTQuantumBitsMax
TSSQ_CWT_MAX_CELLS = 1 << 40            # na * N of one signal
TSSQ_CWT_MAX_N = 1 << 26                # samples of one signal (the limit of the `ssq_cwt2` pipeline)


def tssq_cwt_quantum_log2(N):
    """log2 of `tssq_cwt`'s quantum relative to A, the smallest power of two >= sqrt(Pmax), Pmax the smallest power of two
    >= the signal's max |Wx|^2: -min(38, 61 - ceil(log2 N)).  A part of a contribution is at most 2^min(38, 61 - L)
    quanta and a cell takes at most N <= 2^L of them (one row), so a cell stays below 2^61."""
    N = int(N)
    if N < 1:
        raise ValueError("`N` must be positive")
    return -min(TSSQ_CWT_QUANTUM_LOG2_MAX, 61 - (N - 1).bit_length())


def tssq_cwt_row_freqs(wavelet, scales):
    """nu [na] float64, cycles/sample: the frequency of every row of `tssq_cwt`, wc / (2 pi scale) with the wavelet's peak
    wc = (beta / gamma)^(1 / gamma) for 'gmw' and mu for 'morlet' -- the values the library is given."""
    wcode, p0, p1 = _wavelet(wavelet)
    if not (p0 > 0 and math.isfinite(p0)) or (wcode == WAVELET["gmw"] and not (p1 > 0 and math.isfinite(p1))):
        raise ValueError(f"wavelet {wavelet!r}: the parameters must be positive")
    s = np.ascontiguousarray(scales, dtype=np.float64).reshape(-1)
    if not (np.isfinite(s).all() and (s > 0).all()):
        raise ValueError("`scales` must be positive and finite")
    wc = (p1 / p0) ** (1 / p0) if wcode == WAVELET["gmw"] else p0
    return np.ascontiguousarray(wc / (2 * np.pi * s))


def _tssq_cwt_args(bytes_fn, x, wavelet, scales, nv, fs, t, padtype, order, gamma, work_limit_bytes):
    """The checks `tssq_cwt` and `tmssq_cwt` share, before any GPU work -> (order, the front end, scales, nu, the
    work_limit_bytes argument).  bytes_fn: the transform's *_workspace_bytes."""
    order = _order12(order, "1 and 2 are built")
    f = _cwt_front(x, wavelet, scales, fs, t, gamma, padtype)
    if not (math.isfinite(f.p0) and math.isfinite(f.p1)):                   # (the front end: positive; here finite too)
        raise ValueError(f"wavelet {wavelet!r}: the parameters must be positive")
    s, scaletype, _nv, _ = _scales(scales)
    if scaletype == "log" and nv is not None and nv != _nv:                  # (a ValueError here, `_cwt_freq_grid`: Exception)
        raise ValueError("`nv` used in `scales` differs from `nv` passed (%s != %s)" % (_nv, nv))
    nu = tssq_cwt_row_freqs(wavelet, s)
    if not (np.isfinite(nu).all() and (nu > 0).all()):
        raise ValueError("`scales` give row frequencies that are not positive and finite")
    mn = C.c_int64(0)
    _shape_checked(_lib.load(), bytes_fn(f.code, f.batch, f.N, len(s), order, C.byref(mn)))
    limit = 0 if work_limit_bytes is None else int(work_limit_bytes)
    if work_limit_bytes is not None and limit < mn.value:
        raise ValueError(f"`work_limit_bytes` must be at least {mn.value} for this shape")
    return order, f, s, nu, limit


def tssq_cwt(x, wavelet="gmw", scales="log-piecewise", nv=None, fs=None, t=None, padtype="reflect", order=2, gamma=None,
             get_tau=False, get_targets=False, work_limit_bytes=None):
    """Time-reassigned synchrosqueezed CWT -> (Tx, Wx, scales, row_freqs[, tau][, mm]); not in upstream, conventions of
    `ssq_cwt2`.  Where `ssq_cwt` / `ssq_cwt2` move CWT coefficients along frequency, this moves every complex coefficient
    along TIME inside its own row, to its group delay: a click's cone collapses onto the click's column (as under
    `reassign_cwt`), but the coefficients keep their phase and add coherently, and a fast sweep is put on the column where
    it crosses each row.

    Per sample, with P, n1, n2 = p2up(N), xh, xi_k, T0, T1 and the five maps those of `ssq_cwt2`, in fp64 for either dtype
    (order 1 forms W and Wt alone), and nu_i = wc / (2 pi scales[i]) cycles/sample (`tssq_cwt_row_freqs`):
        d1  = Re(Wt / W)                                   (the group-delay offset; t0 - b for an impulse at t0)
        D   = W^2 + Wt1 W - Wt W1        num = W2 W - W1^2
        d2  = d1 - Im((D / num) (2 pi nu_i + i W1 / W))    (the time at which the locally fitted chirp crosses nu_i)
        off = d2 where order = 2, |num| > gamma^2, d2 is finite and |d2| <= N, else d1; clamped to [-N, N]
        tau = off dt, rounded once to the call's dtype; +inf where |W| < gamma (default 10 eps of the dtype)
        m'  = clip(j + rint(tau / dt), 0, N - 1)           in the call's dtype, on the reported tau
        Tx[i, m'] += Wx[i, j] exp(-2 pi i frac(nu_i (j - m')))       (of the reported Wx, the product in fp64)
    d2 is exact for a linear chirp under any wavelet (the dual of `ssq_cwt2`'s frequency).  The rotation re-references a
    coefficient's phase from column j to column m' at the row's frequency; without it an impulse's contributions would
    sum to psih(0) = 0.  Rows do not mix: `Tx` is [na, N] on the scale rows of `Wx`, and there are no `ssq_freqs`, row
    weights, `maprange`, `squeezing` or `flipud`.  `row_freqs` is nu / dt in Hz, in the call's real dtype.  `tau`
    (get_tau=True) is in seconds, +inf where a bin is not kept; `mm` (get_targets=True) is the int32 map of m', -1 there.

    `Tx` is accumulated by 64-bit integer atomic adds in device memory, in fixed point with the quantum
    q = A 2^`tssq_cwt_quantum_log2(N)`, A the smallest power of two >= sqrt(Pmax), Pmax the smallest power of two >= the
    signal's max |Wx|^2: both parts of every contribution are rounded to a multiple of q, and the integer adds commute, so
    a cell's bits depend neither on the order of the adds, nor on the chunking (`work_limit_bytes`), nor on the batch.  A
    signal of zeros gives an all-zero `Tx`; so does one with a non-finite sample.  `Wx` equals `ssq_cwt2`'s.

    There is no inverse; what stands in for one is a marginal identity per row:
    sum_m' Tx[i, m'] exp(-2 pi i nu_i m') = sum over the kept j of Wx[i, j] exp(-2 pi i nu_i j).

    Built: wavelets 'gmw' (order 0, bandpass norm) and 'morlet'; an ndarray `scales` of any of the three grids; the five
    padtypes; orders 1 and 2; 1-D or batched 2-D `x`; N <= 2^26 and na N <= 2^40.  Anything else raises ValueError before
    any GPU work."""
    lib = _lib.load()
    order, f, s, nu, limit = _tssq_cwt_args(lib.ssq_tssq_cwt_workspace_bytes, x, wavelet, scales, nv, fs, t, padtype, order,
                                            gamma, work_limit_bytes)
    _lib.require_gpu()
    shape = (f.batch, len(s), f.N)
    Tx, Wx = _lib.pinned_empty(shape, f.cdt), _lib.pinned_empty(shape, f.cdt)
    tau = _lib.pinned_empty(shape, f.rdt) if get_tau else None
    mm = _lib.pinned_empty(shape, np.int32) if get_targets else None
    _call(lib.ssq_tssq_cwt_host(f.code, _ptr(f.xa), f.batch, f.N, f.wcode, f.p0, f.p1, _ptr(s), _ptr(nu), len(s), f.dt,
                                f.pad, order, f.gamma, limit, _ptr(Tx), _ptr(Wx), _ptr(tau), _ptr(mm)))
    return (*_unbatch(f.batched, Tx, Wx), s.astype(f.rdt), (nu / f.dt).astype(f.rdt), *_unbatch(f.batched, tau, mm))


def tmssq_cwt(x, wavelet="gmw", scales="log-piecewise", nv=None, fs=None, t=None, padtype="reflect", order=2, n_iter=4,
              gamma=None, get_tau=False, get_targets=False, work_limit_bytes=None):
    """Time-reassigned multisynchrosqueezed CWT -> (Tx, Wx, scales, row_freqs[, tau][, mm]); not in upstream (the
    iteration of Yu, Lin, Ma and He 2020 on `tssq_cwt`'s time map), conventions of `tssq_cwt`.  Where `tssq_cwt` applies
    its time map once, this asks the map again at the column a coefficient landed on, `n_iter` steps in all: on a
    dispersive signal whose group delay is not linear across a row's wavelet the one-step estimate taken off the ridge is
    biased, and the estimate taken where it points is closer.  It is the CWT counterpart of `tmssq_stft` and the dual of
    `mssq_cwt`.

    Everything up to the one-step target is `tssq_cwt`'s: the maps, d1, d2 and the fallback, the clamp to +- N, `tau` in
    the call's dtype (+inf where |W| < gamma) and t[i, j] = clip(j + rint(tau / dt), 0, N - 1) in the call's dtype on
    the reported tau.  Then, per row i:
        c1[j] = t[j]
        c(k+1)[j] = t[ck[j]]  if bin (i, ck[j]) is kept,  else ck[j]                    (k = 1 .. n_iter - 1)
        Tx[i, c_n[j]] += Wx[i, j] exp(-2 pi i frac(nu_i (j - c_n[j])))                  kept j
    A chain stops on a column whose bin in that row is not kept and on a fixed point; a cycle keeps turning until
    `n_iter` runs out.  The rotation takes the total displacement, so the per-row marginal identity of `tssq_cwt` holds
    as it does there.  Rows do not mix.  `Tx` is accumulated as `tssq_cwt`'s, by 64-bit integer atomic adds in fixed
    point with the same quantum (`tssq_cwt_quantum_log2`: a cell still takes at most N contributions), so it is bitwise
    independent of the order of the adds, of the chunking (`work_limit_bytes`) and of the batch.  `n_iter=1` is
    `tssq_cwt` bit for bit.  There is no inverse.

    `Wx` equals `tssq_cwt`'s; `tau` (get_tau=True) is the ONE-step map, +inf where a bin is not kept; `mm`
    (get_targets=True) is int32: the column of `Tx` each coefficient went to, -1 where it was not kept.
    `tmssq_cwt_walk` runs the walk alone on a map the caller holds.

    A one-step target may lie anywhere in its row (the offset is clamped to +- N, not to a window), so the walk kernel
    stages a tile of targets with a halo in LDS (`tmssq_cwt_tile_cols`) and reads the steps that leave it from device
    memory; it is built without register spills or scratch (profiles/tmssq_cwt_resources.txt).  `order` 1 or 2, `n_iter`
    an int from 1 to 64, and the limits of `tssq_cwt`; ValueError otherwise, before any GPU work."""
    lib = _lib.load()
    n_iter = _n_iter(n_iter)
    order, f, s, nu, limit = _tssq_cwt_args(lib.ssq_tmssq_cwt_workspace_bytes, x, wavelet, scales, nv, fs, t, padtype, order,
                                            gamma, work_limit_bytes)
    _lib.require_gpu()
    shape = (f.batch, len(s), f.N)
    Tx, Wx = _lib.pinned_empty(shape, f.cdt), _lib.pinned_empty(shape, f.cdt)
    tau = _lib.pinned_empty(shape, f.rdt) if get_tau else None
    mm = _lib.pinned_empty(shape, np.int32) if get_targets else None
    _call(lib.ssq_tmssq_cwt_host(f.code, _ptr(f.xa), f.batch, f.N, f.wcode, f.p0, f.p1, _ptr(s), _ptr(nu), len(s), f.dt,
                                 f.pad, order, f.gamma, n_iter, limit, _ptr(Tx), _ptr(Wx), _ptr(tau), _ptr(mm)))
    return (*_unbatch(f.batched, Tx, Wx), s.astype(f.rdt), (nu / f.dt).astype(f.rdt), *_unbatch(f.batched, tau, mm))


def _row_edges(nu, dt):
    """e [na + 1] float64, Hz: +inf, the log midpoints sqrt(nu[i-1] nu[i]) / dt of strictly decreasing nu, 0."""
    if len(nu) < 2 or not (np.diff(nu) < 0).all():
        raise ValueError("`scales` must give strictly decreasing row frequencies (strictly increasing scales)")
    e = np.empty(len(nu) + 1, dtype=np.float64)
    e[0], e[-1] = np.inf, 0.0
    e[1:-1] = np.sqrt(nu[:-1] * nu[1:]) / dt
    return e


def set_cwt_row_edges(wavelet, scales, fs=None):
    """e [na + 1] float64, Hz: the edges of `set_cwt`'s rows, the one array the library, the model and the tests read.
    With nu = `tssq_cwt_row_freqs(wavelet, scales)`, which must be strictly decreasing (ValueError otherwise), and dt =
    1 / fs (1 without `fs`):
        e[0] = +inf,    e[i] = sqrt(nu[i-1] nu[i]) / dt  (i = 1 .. na - 1),    e[na] = 0.
    Row i keeps a frequency w with e[i+1] <= w < e[i]: the outer rows are open-ended, and on an edge the higher-frequency
    row wins.  Rows are constant-Q, so the midpoint is taken in log frequency on every scale grid (as `mssq_cwt_row_of_bin`
    takes the nearest row).  Rows and bins are different index sets on the CWT, which is why this is not `ssq_freqs`."""
    fs = 1.0 if fs is None else float(fs)
    if not (fs > 0 and math.isfinite(fs)):
        raise ValueError("`fs` must give a positive sampling period")
    return _row_edges(tssq_cwt_row_freqs(wavelet, scales), 1.0 / fs)


def _extract_cwt(axis, x, wavelet, scales, nv, fs, t, padtype, order, gamma, get_Wx, get_map, work_limit_bytes):
    """The body of `set_cwt` (axis 0) and `tet_cwt` (axis 1) -> (Te, Wx | None, scales, row_freqs[, map]), batch axis
    dropped for 1-D `x`."""
    lib = _lib.load()
    order, f, s, nu, limit = _tssq_cwt_args(lib.ssq_extract_cwt_workspace_bytes, x, wavelet, scales, nv, fs, t, padtype,
                                            order, gamma, work_limit_bytes)
    edges = _row_edges(nu, f.dt) if axis == 0 else None
    _lib.require_gpu()
    shape = (f.batch, len(s), f.N)
    Te = _lib.pinned_empty(shape, f.cdt)
    Wx = _lib.pinned_empty(shape, f.cdt) if get_Wx else None
    mp = _lib.pinned_empty(shape, f.rdt) if get_map else None
    _call(lib.ssq_extract_cwt_host(f.code, _ptr(f.xa), f.batch, f.N, f.wcode, f.p0, f.p1, _ptr(s), _ptr(nu), _ptr(edges),
                                   len(s), f.dt, f.pad, axis, order, f.gamma, limit, _ptr(Te), _ptr(Wx), _ptr(mp)))
    unb = lambda a: None if a is None else (a if f.batched else a[0])                # noqa: E731
    return (unb(Te), unb(Wx), s.astype(f.rdt), (nu / f.dt).astype(f.rdt), *((unb(mp),) if get_map else ()))


def set_cwt(x, wavelet="gmw", scales="log-piecewise", nv=None, fs=None, t=None, padtype="reflect", order=2, gamma=None,
            get_Wx=True, get_w=False, work_limit_bytes=None):
    """Synchroextracting CWT -> (Te, Wx | None, scales, row_freqs[, w]); not in upstream (the CWT counterpart of
    `set_stft`: Yu, Yu and Zhang 2017; second order: Bao et al. 2019), conventions of `tssq_cwt`.  Where `ssq_cwt2` and
    `mssq_cwt` MOVE a coefficient to the frequency it estimates, this KEEPS a coefficient only where its estimated
    instantaneous frequency falls in the band of its own row, and zeroes the rest: what is left is the ridge itself, with
    the CWT's own amplitudes and phases.

    Per sample, with the maps of `ssq_cwt2` in fp64 for either dtype, a cell is live unless |W| < gamma (default 10 eps
    of the dtype; the CWT family's rule) and
        w = |Im om2| / (2 pi dt) where order = 2, |D| > gamma^2 and Im om2 is finite, else |Im om1| / (2 pi dt)
                                                                                               (`ssq_cwt2`'s `w2`)
        w = |Im om1| / (2 pi dt) on every cell for order = 1   (W and W1 alone: TWO inverse transforms a row, not five)
    rounded once to the call's dtype, +inf where the cell is not live (`w`, get_w=True).  With e = `set_cwt_row_edges`
    (+inf, the log midpoints of the rows' frequencies in Hz, 0), each edge rounded once to the call's dtype:
        Te[i, j] = Wx[i, j]  where the cell is live and e[i+1] <= w < e[i],     else +0 + 0i.
    The comparison is made in the call's dtype on the reported `w`; a NaN is kept nowhere, the outer rows are open-ended
    and on an edge the higher-frequency row wins.  The rows' own frequencies are used, not `ssq_freqs`: a bin grid is
    many-to-one onto rows.  There are no `ssq_freqs`, `maprange`, `squeezing`, `flipud` or row weights: `Te` is [na, N]
    on the rows of `Wx`.  `Wx` (None with get_Wx=False, which saves its store and its copy) equals `ssq_cwt2`'s;
    `row_freqs` is nu / dt in Hz in the call's real dtype.  One operator kernel writes every cell exactly once, so signal
    b's bits depend neither on the batch nor on the chunking (`work_limit_bytes`).

    There is no inverse; for a tone on a row's frequency, Re sum_i Te[i, j] gives the tone back (6e-6 at order 2 on the
    shape of DESIGN 4.24).

    Built: what `tssq_cwt` builds, without its na N limit; `scales` must be strictly increasing, so that the rows'
    frequencies strictly decrease.  Anything else raises ValueError before any GPU work.  The kernel is built without
    register spills or scratch (profiles/extract_cwt_resources.txt)."""
    return _extract_cwt(0, x, wavelet, scales, nv, fs, t, padtype, order, gamma, get_Wx, get_w, work_limit_bytes)


def tet_cwt(x, wavelet="gmw", scales="log-piecewise", nv=None, fs=None, t=None, padtype="reflect", order=2, gamma=None,
            get_Wx=True, get_tau=False, work_limit_bytes=None):
    """Transient-extracting CWT -> (Te, Wx | None, scales, row_freqs[, tau]); not in upstream (the CWT counterpart of
    `tet_stft`: Yu 2019), conventions of `tssq_cwt`.  The dual of `set_cwt`: it KEEPS a coefficient only where its
    estimated group delay is its own column, and zeroes the rest, so a click's cone is left as the click's column and a
    fast sweep as the columns where it crosses each row.

    Per sample, with the maps of `tssq_cwt` in fp64 for either dtype, a cell is live unless |W| < gamma (default 10 eps
    of the dtype) and `tau` (get_tau=True) is `tssq_cwt`'s reported offset in seconds, in the call's dtype, +inf where the
    cell is not live: order = 2 uses d2 with its fallback to d1; order = 1 uses d1 (W and Wt alone: TWO inverse
    transforms a row, not five); both clamped to +- N samples.  With
        r = rint(tau / dt)  in the call's dtype,
        Te[i, j] = Wx[i, j]  where the cell is live and r == 0,     else +0 + 0i.
    r is the relative target BEFORE `tssq_cwt`'s clip to [0, N - 1]: an edge cell that the clip would bring back onto
    itself is not kept.  A NaN is kept nowhere.  `Te` is [na, N] on the rows of `Wx`; `Wx` (None with get_Wx=False)
    equals `tssq_cwt`'s and `ssq_cwt2`'s; `row_freqs` is nu / dt in Hz in the call's real dtype.  One operator kernel
    writes every cell exactly once: none of `tssq_cwt`'s maxima, accumulators, targets or atomic adds, and a workspace
    without their 20 bytes a cell.

    There is no inverse.

    Built: what `tssq_cwt` builds, without its na N limit.  Anything else raises ValueError before any GPU work.  The
    kernel is built without register spills or scratch (profiles/extract_cwt_resources.txt)."""
    return _extract_cwt(1, x, wavelet, scales, nv, fs, t, padtype, order, gamma, get_Wx, get_tau, work_limit_bytes)


TMSSQ_CWT_WALK_MAX_N = 1 << 30          # csrc/cwt_tmsst.hip: columns of a map handed to `tmssq_cwt_walk`


def tmssq_cwt_walk(targets, n_iter):
    """The walk of `tmssq_cwt` alone, on a map the caller holds -> int32, same shape.  `targets`: int32 [rows, n] or
    [B, rows, n], a target indexes the column axis itself (anywhere in 0 .. n - 1) and -1 means none; per row
        c1[j] = targets[j];   c(k+1)[j] = targets[ck[j]] if targets[ck[j]] >= 0, else ck[j]        (k = 1 .. n_iter - 1)
    and the result is c_n (-1 where targets[j] is).  Runs the kernel of `tmssq_cwt` (csrc/cwt_tmsst.hip); a non-int32
    array, an empty axis, n > 2^30, a target outside -1 .. n - 1 and an `n_iter` that is not an int from 1 to 64 raise
    ValueError before any GPU work."""
    lib = _lib.load()
    n_iter = _n_iter(n_iter)
    if not isinstance(targets, np.ndarray) or targets.dtype != np.int32 or targets.ndim not in (2, 3):
        raise ValueError("`targets` must be an int32 ndarray [rows, n] or [B, rows, n]")
    t3 = np.ascontiguousarray(targets if targets.ndim == 3 else targets[None])
    B, R, n = t3.shape
    if B < 1 or R < 1 or n < 1:
        raise ValueError(f"`targets` of shape {targets.shape}: no empty axis")
    if n > TMSSQ_CWT_WALK_MAX_N:
        raise ValueError(f"`targets` of {n} columns: at most 2^30")
    if t3.min() < -1 or t3.max() >= n:
        raise ValueError(f"`targets` holds targets outside -1 .. n - 1 = {n - 1}")
    _lib.require_gpu()
    out = np.empty_like(t3)
    _call(lib.ssq_tmssq_cwt_walk_host(_ptr(t3), B, R, n, n_iter, _ptr(out)))
    return _unbatch(targets.ndim == 3, out)[0]


def tmssq_cwt_tile_cols():
    """(T, halo): the columns of the tile one workgroup of `tmssq_cwt`'s walk kernel owns, and the columns it stages in
    LDS on either side of it; a step of a chain that lands outside them is read from device memory (no GPU needed)."""
    halo = C.c_int(0)
    T = _lib.load().ssq_tmssq_cwt_tile_cols(C.byref(halo))
    return int(T), int(halo.value)


def mssq_cwt_row_of_bin(wavelet, scales, ssq_freqs_asc, fs=None):
    """rho, int32 [na]: for every bin of the ascending `ssq_freqs_asc` the row of `scales` whose frequency
    nu_i = `tssq_cwt_row_freqs(wavelet, scales)[i]` fs is nearest in log2 (rows are constant-Q, so log distance is used for
    'linear' grids too); on a tie the lowest row; a bin with a frequency <= 0 takes the row of the lowest nu.  float64,
    numpy, no GPU.  On a 'peak' log grid over log scales it is the reversal na - 1 - bin."""
    nu = tssq_cwt_row_freqs(wavelet, scales) * (1.0 if fs is None else float(fs))
    f = np.ascontiguousarray(ssq_freqs_asc, dtype=np.float64).reshape(-1)
    if f.size != nu.size:
        raise ValueError("`ssq_freqs_asc` must have one frequency per scale (%s != %s)" % (f.size, nu.size))
    if not (np.isfinite(f).all() and np.isfinite(nu).all() and (nu > 0).all()):
        raise ValueError("`ssq_freqs_asc` and the rows' frequencies must be finite (and the rows' positive)")
    pos = f > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        dist = np.abs(np.log2(nu)[None, :] - np.log2(np.where(pos, f, 1.0))[:, None])
    return np.where(pos, dist.argmin(axis=1), int(nu.argmin())).astype(np.int32)


def _mssq_cwt_rows(na):
    if not 2 <= na <= MSST_MAX_ROWS:
        raise ValueError(f"na = {na} scales: mssq_cwt builds 2 .. {MSST_MAX_ROWS} (the walk holds every row of a tile of "
                         "columns in LDS)")


def mssq_cwt(x, wavelet="gmw", scales="log-piecewise", nv=None, fs=None, t=None, ssq_freqs=None, padtype="reflect",
             squeezing="sum", maprange="peak", gamma=None, flipud=True, order=2, n_iter=4, get_w=False, get_rows=False,
             get_bins=False):
    """Multisynchrosqueezed CWT -> (Tx, Wx, ssq_freqs, scales[, w][, rows][, bins]); not in upstream (the CWT counterpart of
    `mssq_stft`; Yu, Wang and Zhao 2019), conventions of `ssq_cwt2`.  Where `ssq_cwt2` applies its frequency map once, this
    asks the map again at the row nearest to the bin a coefficient landed on, `n_iter` steps in all: on a signal whose
    modulation is not linear inside the wavelet the one-step estimate taken off the ridge is biased, and the estimate
    taken where it points is closer.

    Per column, with na rows (scales ascending) and f_asc [na] the ascending bin frequencies the call squeezes onto:
        w[i]    the one-step frequency of row i, in the call's dtype, as reported (get_w=True): `order=2` the w2 of
                `ssq_cwt2`, including its fallback to the first-order frequency where |D| <= gamma^2; `order=1`
                |Im om1| / (2 pi dt) on every element (it runs the same five transforms and costs the same); +inf where
                |W| < gamma
        b[i]    the one-step bin: `ssqueeze`'s bin rule on w[i], in the call's dtype, before any `flipud`; -1 where w is
                infinite; NaN lands in bin 0, as `ssqueeze` has it
        rho[k]  the row of bin k: `mssq_cwt_row_of_bin(wavelet, scales, f_asc, fs)`, the row nearest in log frequency
                (the rows and the bins are different index sets; on a 'peak' log grid rho is the reversal na - 1 - k)
    The walk, in row space:
        r1[k] = k  (kept k)
        r(i+1)[k] = rho[b[ri[k]]]  if b[rho[b[ri[k]]]] >= 0,  else ri[k]             (i = 1 .. n_iter - 1)
    A chain stops on a row that has no map of its own and on a fixed point; a cycle keeps turning until `n_iter` runs
    out.  Then w_n[k] = w[r_n[k]] (+inf where k is not kept) and `Tx` = `ssqueeze(Wx, w_n, ...)`: rows ascending inside a
    column, no atomics, `flipud` applied there and nowhere else.  A coefficient lands on bin b[r_n[k]] with its OWN
    row weight and keeps its phase, so every column keeps its weighted sum: `issq_cwt`, `extract_ridges` and the
    component inversion take `Tx` unchanged.  `n_iter=1`, `order=2` is `ssq_cwt2` bit for bit.

    `Wx` equals `ssq_cwt2`'s; `w` is the ONE-step map; `rows` (get_rows=True) is int32 r_n, -1 where an element is not
    kept; `bins` (get_bins=True) is int32 b, the one-step bins the kernel computed.  `mssq_cwt_walk` runs the walk alone
    on a frequency map the caller holds.

    Built: what `ssq_cwt2` builds, with `order` 1 or 2, `n_iter` an int from 1 to 64 (the bound of `mssq_stft`), 2 .. 2049
    scales and `squeezing` 'sum' or 'lebesgue'.  Anything else raises ValueError before any GPU work.  The walk runs out
    of LDS, a tile of columns at a time (csrc/cwt_msst.hip); its kernel is built without register spills or scratch
    (profiles/msst_cwt_resources.txt)."""
    lib = _lib.load()
    order = _order12(order, "mssq_cwt builds orders 1 and 2")
    n_iter = _n_iter(n_iter)
    squeeze = _squeeze_code(squeezing)
    f = _cwt_front(x, wavelet, scales, fs, t, gamma, padtype)
    s, row_const, f_asc, scaletype, f_idx = _finite_freq_grid(f, scales, nv, ssq_freqs, maprange)
    _mssq_cwt_rows(len(s))
    rho = mssq_cwt_row_of_bin(wavelet, s, f_asc, 1.0 / f.dt)
    _lib.require_gpu()
    shape = (f.batch, len(s), f.N)
    Tx, Wx = _lib.pinned_empty(shape, f.cdt), _lib.pinned_empty(shape, f.cdt)
    w = _lib.pinned_empty(shape, f.rdt) if get_w else None
    rows = _lib.pinned_empty(shape, np.int32) if get_rows else None
    bins = _lib.pinned_empty(shape, np.int32) if get_bins else None
    _call(lib.ssq_mssq_cwt_host(f.code, _ptr(f.xa), f.batch, f.N, f.wcode, f.p0, f.p1, _ptr(s), len(s), f.dt,
                                _ptr(row_const), _ptr(f_asc), FREQS[scaletype], f_idx or 0, f.pad, squeeze, f.gamma,
                                VARIANT_FLIPUD if flipud else 0, 0, order, n_iter, _ptr(rho), _ptr(Tx), _ptr(Wx), _ptr(w),
                                _ptr(rows), _ptr(bins)))
    return (*_unbatch(f.batched, Tx, Wx), f_asc[::-1].astype(f.rdt), s.astype(f.rdt), *_unbatch(f.batched, w, rows, bins))


def mssq_cwt_walk(w, ssq_freqs_asc, row_of_bin, n_iter):
    """The walk of `mssq_cwt` alone, on a frequency map the caller holds -> (rows, bins, w_n).  `w`: float32 / float64
    [na, n] or [B, na, n] (2 <= na <= 2049), +inf where an element is not kept; `ssq_freqs_asc` [na]: the ascending bin
    frequencies, their type ('log', 'linear', 'log-piecewise') inferred as `ssqueeze` infers it; `row_of_bin` [na]: the
    row of every bin.  `bins` is int32 b, the bin of every element by `ssqueeze`'s rule in w's dtype (-1 where w is
    infinite); `rows` int32 r_n of the walk in `mssq_cwt`'s docstring (-1 where not kept); `w_n` = w[r_n], +inf where not
    kept.  Runs the kernel of `mssq_cwt` (csrc/cwt_msst.hip); every refusal is a ValueError before any GPU work."""
    lib = _lib.load()
    n_iter = _n_iter(n_iter)
    if not isinstance(w, np.ndarray) or w.dtype not in (np.float32, np.float64) or w.ndim not in (2, 3):
        raise ValueError("`w` must be a float32 or float64 ndarray [na, n] or [B, na, n]")
    w3 = np.ascontiguousarray(w if w.ndim == 3 else w[None])
    B, na, n = w3.shape
    if not 2 <= na <= MSST_MAX_ROWS or B < 1 or n < 1:
        raise ValueError(f"`w` of shape {w.shape}: 2 .. {MSST_MAX_ROWS} rows, and no empty axis")
    if not isinstance(ssq_freqs_asc, np.ndarray) or ssq_freqs_asc.shape != (na,) or ssq_freqs_asc.dtype.kind != "f":
        raise ValueError("`ssq_freqs_asc` must be a float ndarray with one frequency per row of `w`")
    if not (np.isfinite(ssq_freqs_asc).all() and (np.diff(ssq_freqs_asc) > 0).all()):
        raise ValueError("`ssq_freqs_asc` must be finite and ascending")
    if na == 2:                                            # (two frequencies have no second difference to infer from)
        f_asc, scaletype, f_idx = np.ascontiguousarray(ssq_freqs_asc, dtype=np.float64), "linear", None
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            f_asc, scaletype, f_idx = _freq_type(ssq_freqs_asc, None, None, None)
    rho = np.asarray(row_of_bin)
    if rho.shape != (na,) or rho.dtype.kind not in "iu" or rho.min() < 0 or rho.max() >= na:
        raise ValueError(f"`row_of_bin` must hold one integer row from 0 to na - 1 = {na - 1} per bin")
    rho = np.ascontiguousarray(rho, dtype=np.int32)
    _lib.require_gpu()
    rows, bins, w_n = np.empty(w3.shape, np.int32), np.empty(w3.shape, np.int32), np.empty_like(w3)
    _call(lib.ssq_mssq_cwt_walk_host(SSQ_F32 if w3.dtype == np.float32 else SSQ_F64, _ptr(w3), B, na, n, _ptr(f_asc),
                                     FREQS[scaletype], f_idx or 0, _ptr(rho), n_iter, _ptr(rows), _ptr(bins), _ptr(w_n)))
    return tuple(_unbatch(w.ndim == 3, rows, bins, w_n))


def mssq_cwt_tile_cols(na):
    """Columns of the LDS tile one workgroup of `mssq_cwt`'s walk kernel owns for `na` scales (no GPU needed)."""
    c = _lib.load().ssq_mssq_cwt_tile_cols(int(na))
    if c < 0:
        raise ValueError(f"na {na!r}: 2 .. {MSST_MAX_ROWS}")
    return int(c)


def lmssq_cwt_default_delta(wavelet, scales):
    """The default `delta` of `lmssq_cwt`: the half-width in rows of the wavelet's response across the scales.  With the
    wavelet evaluated by the library (`ssq_upstream_psih`, as `upstream_scales` does), wc its peak frequency, i0 = na // 2
    and R[i] = psih(scales[i] wc / scales[i0]) the response of the rows to a tone on the peak frequency of row i0, the
    smallest d >= 1 at which both neighbours i0 - d and i0 + d that exist are <= 1e-3 R[i0]; at most min(na - 1, 256).  The
    1e-3 is part of the definition, not a measurement.  numpy on the host, no GPU."""
    from .upstream_scales import _psih_fn
    wcode, p0, p1 = _wavelet(wavelet)
    s = np.ascontiguousarray(scales, dtype=np.float64).reshape(-1)
    na = len(s)
    if na < 2 or not (np.isfinite(s).all() and (s > 0).all()):
        raise ValueError("`scales` must hold at least 2 positive, finite scales")
    wc = (p1 / p0) ** (1 / p0) if wcode == WAVELET["gmw"] else p0
    i0 = na // 2
    R = _psih_fn(wavelet)(s * (wc / s[i0]))
    d = 1
    while d < na - 1:
        near = [R[i] for i in (i0 - d, i0 + d) if 0 <= i < na]
        if all(r <= LMSST_LOBE_LEVEL * R[i0] for r in near):
            break
        d += 1
    return int(max(1, min(d, na - 1, LMSST_MAX_DELTA)))


def lmssq_cwt(x, wavelet="gmw", scales="log-piecewise", nv=None, fs=None, t=None, ssq_freqs=None, padtype="reflect",
              squeezing="sum", maprange="peak", gamma=None, flipud=True, delta=None, get_w=False, get_rows=False):
    """Local maximum synchrosqueezed CWT -> (Tx, Wx, ssq_freqs, scales[, w][, rows]); not in upstream (the CWT counterpart
    of `lmssq_stft`; Yu, Wang, Zhao and Liu 2019), conventions of `mssq_cwt`.  A coefficient moves to the frequency of the
    row where |Wx| has its maximum inside a window of +- `delta` rows.  No derivative of the wavelet is formed: ONE
    inverse transform per row against the five of `ssq_cwt2`.

    Per column, with na rows (scales ascending) and an int `delta` >= 1:
        A[i] = re^2 + im^2 of Wx[i] as the call reports it (rounded to the call's dtype), evaluated in fp64 with the two
               products and the sum rounded one by one
        m[i] = the row of the maximum of A over rows max(0, i - delta) .. min(na - 1, i + delta), scanned ascending and
               taken only where strictly greater, so the lowest row wins a tie; rows that are not kept take part
        w[i] = nu_hz[m[i]], nu_hz = `tssq_cwt_row_freqs(wavelet, scales)` fs rounded once to the call's dtype; +inf where
               the cell is not kept: |W| < gamma on the fp64 coefficient (default 10 eps of the dtype; `ssq_cwt2`'s rule)
    and `Tx` = `ssqueeze(Wx, w, ...)`: rows ascending inside a column, no atomics, `flipud` applied there.  A coefficient
    keeps its OWN row weight and phase, so every column keeps its weighted sum: `issq_cwt`, `extract_ridges` and the
    component inversion take `Tx` unchanged.  On a 'peak' log grid over log scales a coefficient lands on bin
    na - 1 - m[i].

    `Wx` is `ssq_cwt2`'s bit for bit; `w` (get_w=True) is real; `rows` (get_rows=True) is int32 m, -1 where a cell is not
    kept.  `lmsst_rows` runs the window maximum alone on a map the caller holds.

    `delta=None` asks for `lmssq_cwt_default_delta(wavelet, scales)`, the half-width of the wavelet's response across the
    rows (its 1e-3 level is part of the definition, not a measurement); else an int from 1 to min(na - 1, 256) -- 256 is a
    bound on work, not a measured number.  The limit is `lmssq_stft`'s: the energy goes to the SCALOGRAM's ridge, which on
    a fast FM is not the instantaneous frequency.

    Built: what `ssq_cwt2` builds (order-0 'gmw' and 'morlet', an ndarray `scales` of the three grids), for 2 .. 2049
    scales and `squeezing` 'sum' or 'lebesgue'.  Anything else, a bool, a float or an out-of-range `delta` raises
    ValueError before any GPU work.  The kernels are built without register spills or scratch
    (profiles/lmsst_cwt_resources.txt)."""
    lib = _lib.load()
    squeeze = _squeeze_code(squeezing)
    f = _cwt_front(x, wavelet, scales, fs, t, gamma, padtype)
    s, row_const, f_asc, scaletype, f_idx = _finite_freq_grid(f, scales, nv, ssq_freqs, maprange)
    na = len(s)
    if not 2 <= na <= MSST_MAX_ROWS:
        raise ValueError(f"na = {na} scales: lmssq_cwt builds 2 .. {MSST_MAX_ROWS}")
    delta = _delta(delta, na, lambda: lmssq_cwt_default_delta(wavelet, s))
    nu_hz = np.ascontiguousarray(tssq_cwt_row_freqs(wavelet, s) / f.dt)
    if not (np.isfinite(nu_hz).all() and (nu_hz > 0).all()):
        raise ValueError("`scales` give row frequencies that are not positive and finite")
    _lib.require_gpu()
    shape = (f.batch, na, f.N)
    Tx, Wx = _lib.pinned_empty(shape, f.cdt), _lib.pinned_empty(shape, f.cdt)
    w = _lib.pinned_empty(shape, f.rdt) if get_w else None
    rows = _lib.pinned_empty(shape, np.int32) if get_rows else None
    _call(lib.ssq_lmssq_cwt_host(f.code, _ptr(f.xa), f.batch, f.N, f.wcode, f.p0, f.p1, _ptr(s), na, f.dt,
                                 _ptr(row_const), _ptr(f_asc), FREQS[scaletype], f_idx or 0, f.pad, squeeze, f.gamma,
                                 VARIANT_FLIPUD if flipud else 0, 0, delta, _ptr(nu_hz), _ptr(Tx), _ptr(Wx), _ptr(w),
                                 _ptr(rows)))
    return (*_unbatch(f.batched, Tx, Wx), f_asc[::-1].astype(f.rdt), s.astype(f.rdt), *_unbatch(f.batched, w, rows))


def lmsst_rows(A, delta):
    """The window maximum of `lmssq_cwt` alone, on a map the caller holds -> int32 m, same shape.  `A`: float32 or float64
    [R, n] or [B, R, n] (2 <= R <= 2049; a float32 map is widened, which is exact); per column
        m[k] = the row of the maximum of A over rows max(0, k - delta) .. min(R - 1, k + delta), scanned ascending and
               taken only where strictly greater (the lowest row wins a tie)
    with no keep rule.  Runs the plane kernel of `lmssq_cwt` (csrc/cwt_lmsst.hip); a `delta` that is not an int from 1 to
    min(R - 1, 256) and every other refusal is a ValueError before any GPU work."""
    lib = _lib.load()
    if not isinstance(A, np.ndarray) or A.dtype not in (np.float32, np.float64) or A.ndim not in (2, 3):
        raise ValueError("`A` must be a float32 or float64 ndarray [R, n] or [B, R, n]")
    a3 = np.ascontiguousarray(A if A.ndim == 3 else A[None])
    B, R, n = a3.shape
    if not 2 <= R <= MSST_MAX_ROWS or B < 1 or n < 1:
        raise ValueError(f"`A` of shape {A.shape}: 2 .. {MSST_MAX_ROWS} rows, and no empty axis")
    if delta is None:
        raise ValueError("delta None: `lmsst_rows` has no default")
    delta = _delta(delta, R, None)
    _lib.require_gpu()
    out = np.empty(a3.shape, np.int32)
    _call(lib.ssq_lmsst_rows_host(SSQ_F32 if a3.dtype == np.float32 else SSQ_F64, _ptr(a3), B, R, n, delta, _ptr(out)))
    return _unbatch(A.ndim == 3, out)[0]


CONCEFT_MAX_ORDERS = 8                  # csrc/cwt_conceft.hip: kConceftMaxOrders
CONCEFT_MAX_DRAWS = 256                 # csrc/cwt_conceft.hip: kConceftMaxDraws
CONCEFT_MIN_ADMITTANCE = 1e-6           # a draw's c_m relative to sum_j |r_mj| |C_kj| below which it is refused


def gmw_adm_ssq(gamma, beta, k):
    """The admittance of the order-k GMW (bandpass norm), C_k = int_0^inf psih_k(w) / w dw, in closed form:
    A sum_m kc[m] 2^m Gamma(beta / gamma + m) / gamma with kc = `gmw_k_constants(gamma, beta, k)`, wc = (beta / gamma)^(1 /
    gamma) and A = exp(-beta ln wc + wc^gamma).  C_0 is `adm_ssq(('gmw', ...))`, the constant `issq_cwt` divides by."""
    gamma, beta, k = float(gamma), float(beta), int(k)
    if not (gamma > 0 and beta > 0 and math.isfinite(gamma) and math.isfinite(beta)):
        raise ValueError("gmw_adm_ssq: gamma and beta must be positive and finite")
    if not 0 <= k <= GMW_MAX_ORDER:
        raise ValueError(f"gmw_adm_ssq: order {k!r} outside 0 .. {GMW_MAX_ORDER}")
    kc = gmw_k_constants(gamma, beta, k)
    q = beta / gamma
    ln_a = q - q * math.log(q)                               # -beta ln wc + wc^gamma
    if q + k < 170 and abs(ln_a) < 700:                       # Gamma itself: the alternating sum cancels several digits
        return float(math.exp(ln_a) * sum(kc[m] * 2.0 ** m * math.gamma(q + m) for m in range(k + 1)) / gamma)
    return float(sum(kc[m] * 2.0 ** m * math.exp(math.lgamma(q + m) + ln_a) for m in range(k + 1)) / gamma)


def _conceft_gauge(r, adm):
    """Rows of `r` [M, J] normalised and turned by the unit phase that makes c_m = sum_j r_mj adm[j] real and positive
    -> (r complex128 [M, J], c float64 [M]).  Formed in extended precision and rounded once, so that equivalent inputs
    (a row times any unit phase, or a row that is gauged already) agree to the last place or so."""
    r = np.array(r, dtype=np.complex128)
    adm = np.asarray(adm, dtype=np.float64).reshape(-1)
    if r.ndim != 2 or r.shape[1] != len(adm) or r.shape[0] < 1:
        raise ValueError(f"`vectors` must be [n_draws, {len(adm)}] (one column per order); got shape {r.shape}")
    if not np.isfinite(r.view(np.float64)).all():
        raise ValueError("`vectors` must be finite")
    rl, al = r.astype(np.clongdouble), adm.astype(np.longdouble)
    norm = np.sqrt((rl.real ** 2 + rl.imag ** 2).sum(axis=1))
    if (norm == 0).any():
        raise ValueError("`vectors`: draw %d is the zero vector" % int(np.argmax(norm == 0)))
    rl = rl / norm[:, None]
    c = (rl * al[None, :]).sum(axis=1)
    floor = CONCEFT_MIN_ADMITTANCE * (np.abs(rl) * np.abs(al)[None, :]).sum(axis=1)
    bad = ~(np.abs(c) > floor)
    if bad.any():
        m = int(np.argmax(bad))
        raise ValueError("`vectors`: draw %d is degenerate, its admittance |sum_j r_j C_kj| = %.3g is not above %.3g "
                         "(the draw's wavelet has no usable reconstruction constant)" % (m, float(abs(c[m])), float(floor[m])))
    rl = rl * (np.conj(c) / np.abs(c))[:, None]
    return np.ascontiguousarray(rl.astype(np.complex128)), np.abs(c).astype(np.float64)


def _conceft_draws(n_draws, n_orders, seed):
    """The raw draws: `default_rng(seed)` complex normals [n_draws, n_orders] with unit rows; every refusal of the counts."""
    for name, v in (("n_draws", n_draws), ("n_orders", n_orders)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} {v!r}: must be an int")
    M, J = int(n_draws), int(n_orders)
    if not 1 <= M <= CONCEFT_MAX_DRAWS:
        raise ValueError(f"n_draws {n_draws!r}: 1 .. {CONCEFT_MAX_DRAWS} are built")
    if not 1 <= J <= CONCEFT_MAX_ORDERS:
        raise ValueError(f"n_orders {n_orders!r}: 1 .. {CONCEFT_MAX_ORDERS} are built")
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((M, J)) + 1j * rng.standard_normal((M, J))
    return r / np.linalg.norm(r, axis=1, keepdims=True)


def conceft_vectors(n_draws, n_orders, seed, adm):
    """The random unit vectors of `conceft_cwt`: complex normal draws from `np.random.default_rng(seed)`, normalised, each
    turned by the unit phase that makes c_m = sum_j r_mj adm[j] real and positive (`adm`: the orders' `gmw_adm_ssq`)
    -> complex128 [n_draws, n_orders]."""
    r = _conceft_draws(n_draws, n_orders, seed)
    if len(np.asarray(adm).reshape(-1)) != r.shape[1]:
        raise ValueError(f"`adm` must hold one admittance per order ({r.shape[1]})")
    return _conceft_gauge(r, adm)[0]


def conceft_cwt(x, wavelet="gmw", scales="log-piecewise", orders=3, n_draws=20, seed=0, vectors=None, nv=None, fs=None,
                t=None, ssq_freqs=None, padtype="reflect", maprange="peak", gamma=None, flipud=True, get_Wx=False,
                get_w=False, squeezing="sum"):
    """ConceFT, the multitaper synchrosqueezed CWT (Daubechies, Wang and Wu 2016) -> (Tx, ssq_freqs, scales[, Wx][, w]);
    not in upstream, conventions of `ssq_cwt`.  The answer to noise: the J orthogonal wavelets of a Morse family are the
    GMWs of orders k_0 .. k_{J-1}; M random unit vectors r_m in C^J each give a wavelet sum_j r_mj psi_kj, and the M
    synchrosqueezed transforms are averaged.  The signal's ridge is where every draw agrees, the noise-driven
    reassignments differ from draw to draw and average down; a plain multitaper average widens the ridge, this does not.

    With W_j, dW_j the planes of `cwt_higher_order(x, wavelet, order=orders, average=False, derivative=True)` (one forward
    FFT per signal) and C_k = `gmw_adm_ssq(gamma, beta, k)`:
        gauge      r_m times the unit phase that makes c_m = sum_j r_mj C_kj real and positive (a global phase of the
                   wavelet moves no bin; the draws then add coherently and every column sum of Tx stays a positive
                   multiple of the analytic signal); a draw with c_m <= 1e-6 sum_j |r_mj| |C_kj| is refused
        per draw   W^(m) = sum_j r_mj W_j, dW^(m) = sum_j r_mj dW_j (j ascending, in the call's dtype); the phase
                   transform and the bin by `ssq_cwt`'s rule, kept where |W^(m)| > gamma (default 10 eps of the dtype);
                   Tx[k, n] += W^(m)[i, n] row_const[i]
        scale      Tx *= C_0 / sum_m c_m, so `issq_cwt(Tx, wavelet)` inverts it as it inverts `ssq_cwt`'s; with
                   vectors = [[1, 0, ...]] the scale is exactly 1 and Tx is `ssq_cwt`'s
    The combinations are linear, so the 2 J planes are computed once and every draw is formed from them on the device in
    one fused kernel (csrc/cwt_conceft.hip): one thread owns a column of Tx, no atomics, the additions into a cell in a
    fixed order, so the result is bitwise the same run to run and whatever the batch.

    `orders`: an int J (the orders 0 .. J-1) or a tuple of distinct orders within 0 .. 16, at most 8.  `vectors`
    [M, J] complex overrides `n_draws` (1 .. 256) and `seed` (`conceft_vectors`); its rows are normalised and gauged here.
    `ssq_freqs` are the order-0 wavelet's, as for `ssq_cwt(order=)`.  `Wx` (get_Wx=True): the J planes [J, na, N]; `w`
    (get_w=True): every draw's phase transform [M, na, N], real, +inf where not kept.  A batch [B, N] gives a leading B.

    Built: wavelet 'gmw' with bandpass norm; an ndarray `scales` of any of the three grids; `ssq_freqs` None, a string or
    an array; maprange 'peak' / 'maximal'; squeezing 'sum'; the five padtypes; `flipud`; J na <= 32767.  Anything else
    raises ValueError before any GPU work."""
    lib = _lib.load()
    if squeezing != "sum":
        raise ValueError(f"squeezing {squeezing!r}: conceft_cwt builds 'sum' only")
    if _wavelet_name(wavelet) != "gmw":
        raise ValueError("conceft_cwt: the wavelet must be GMW, whose higher orders are the orthogonal tapers (got %r)"
                         % (wavelet,))
    f = _cwt_front(x, wavelet, scales, fs, t, gamma, padtype)
    p0, p1 = f.p0, f.p1
    if not (math.isfinite(p0) and math.isfinite(p1)):                       # (the front end: positive; here finite too)
        raise ValueError(f"wavelet {wavelet!r}: the parameters must be positive")
    if isinstance(orders, (bool, np.bool_)):
        raise ValueError(f"`orders` must be an int or a tuple / list / range of ints (got {orders!r})")
    if isinstance(orders, (int, np.integer)):
        if not 1 <= orders <= CONCEFT_MAX_ORDERS:
            raise ValueError(f"`orders` {orders!r}: 1 .. {CONCEFT_MAX_ORDERS} orders are built")
        orders = tuple(range(int(orders)))
    elif isinstance(orders, (tuple, list, range)):
        orders = tuple(orders)
    else:
        raise ValueError(f"`orders` must be an int or a tuple / list / range of ints (got {orders!r})")
    for k in orders:
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"`orders` must hold ints (got {orders!r})")
        if not 0 <= k <= GMW_MAX_ORDER:
            raise ValueError(f"`orders` must lie within 0 .. {GMW_MAX_ORDER} (got {orders!r})")
    if not 1 <= len(orders) <= CONCEFT_MAX_ORDERS:
        raise ValueError(f"`orders`: 1 .. {CONCEFT_MAX_ORDERS} orders are built (got {len(orders)})")
    if len(set(orders)) != len(orders):
        raise ValueError(f"`orders` must be distinct (got {orders!r})")
    orders = tuple(int(k) for k in orders)
    J = len(orders)
    adm = np.array([gmw_adm_ssq(p0, p1, k) for k in orders])
    if vectors is None:
        r, c = _conceft_gauge(_conceft_draws(n_draws, J, seed), adm)
    else:
        vectors = np.asarray(vectors)
        if vectors.ndim != 2 or vectors.shape[1] != J or vectors.dtype.kind not in "fiuc":
            raise ValueError(f"`vectors` must be a numeric array [n_draws, {J}] (one column per order); got shape "
                             f"{vectors.shape}")
        if not 1 <= vectors.shape[0] <= CONCEFT_MAX_DRAWS:
            raise ValueError(f"`vectors`: 1 .. {CONCEFT_MAX_DRAWS} draws are built (got {vectors.shape[0]})")
        r, c = _conceft_gauge(vectors, adm)
    M = r.shape[0]
    scale = float(gmw_adm_ssq(p0, p1, 0) / c.sum())         # (vectors = e_0 of order 0: C_0 / C_0, exactly 1)
    s, row_const, f_asc, scaletype, f_idx = _finite_freq_grid(f, scales, nv, ssq_freqs, maprange)
    na = len(s)
    _shape_checked(lib, lib.ssq_conceft_cwt_workspace_bytes(f.code, f.batch, f.N, na, J, None))
    polys = np.ascontiguousarray(gmw_order_coefficients(p0, p1, orders, average=False))
    _lib.require_gpu()
    Tx = _lib.pinned_empty((f.batch, na, f.N), f.cdt)
    Wx = _lib.pinned_empty((f.batch, J, na, f.N), f.cdt) if get_Wx else None
    w = _lib.pinned_empty((f.batch, M, na, f.N), f.rdt) if get_w else None
    _call(lib.ssq_conceft_cwt_host(f.code, _ptr(f.xa), f.batch, f.N, p0, p1, _ptr(polys), polys.shape[1], J, _ptr(r), M,
                                   scale, _ptr(s), na, f.dt, _ptr(row_const), _ptr(f_asc), FREQS[scaletype], f_idx or 0,
                                   f.pad, f.gamma, VARIANT_FLIPUD if flipud else 0, 0, _ptr(Tx), _ptr(Wx), _ptr(w)))
    return (*_unbatch(f.batched, Tx), f_asc[::-1].astype(f.rdt), s.astype(f.rdt), *_unbatch(f.batched, Wx, w))


def hermite_windows(n_fft, n_tapers, sigma=None):
    """The first `n_tapers` orthonormal Hermite functions as windows of `n_fft` samples -> float64 [n_tapers, n_fft]: the
    tapers of `conceft_stft` (Daubechies, Wang and Wu 2016, section 3).  psi_0(u) = pi^(-1/4) exp(-u^2 / 2) and the
    three-term recurrence psi_{k+1} = sqrt(2 / (k + 1)) u psi_k - sqrt(k / (k + 1)) psi_{k-1}, sampled at
    u = (i - n_fft // 2) / sigma and divided by sqrt(sigma), so that the rows are orthonormal in l2 once the window holds
    them: with the default sigma = n_fft / 16 the Gram matrix of 8 tapers is within 1e-15 of the identity for n_fft >= 64
    and within 3e-8 at n_fft = 32; at n_fft = 16 the higher tapers are cut off by the window and are NOT orthogonal (the
    transform does not need orthogonality, only the gauge).  1 <= n_tapers <= 8."""
    for name, v in (("n_fft", n_fft), ("n_tapers", n_tapers)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} {v!r}: must be an int")
    if n_fft < 1:
        raise ValueError(f"n_fft {n_fft!r}: must be positive")
    if not 1 <= n_tapers <= CONCEFT_MAX_ORDERS:
        raise ValueError(f"n_tapers {n_tapers!r}: 1 .. {CONCEFT_MAX_ORDERS} are built")
    if sigma is None:
        sigma = n_fft / 16
    if (isinstance(sigma, (bool, np.bool_)) or not isinstance(sigma, (int, float, np.integer, np.floating))
            or not math.isfinite(sigma) or not sigma > 0):
        raise ValueError(f"sigma {sigma!r}: must be positive and finite")
    sigma = float(sigma)
    u = (np.arange(int(n_fft), dtype=np.float64) - int(n_fft) // 2) / sigma
    h = np.empty((int(n_tapers), int(n_fft)), dtype=np.float64)
    h[0] = math.pi ** -0.25 * np.exp(-0.5 * u * u)
    for k in range(int(n_tapers) - 1):
        h[k + 1] = math.sqrt(2.0 / (k + 1)) * u * h[k] - (math.sqrt(k / (k + 1.0)) * h[k - 1] if k else 0.0)
    return h / math.sqrt(sigma)


def conceft_stft(x, tapers=None, n_fft=None, win_len=None, hop_len=1, fs=None, t=None, modulated=True, padtype="reflect",
                 n_tapers=3, n_draws=20, seed=0, vectors=None, gamma=None, flipud=False, get_planes=False, get_w=False):
    """ConceFT on the STFT, the multitaper synchrosqueezed STFT (Daubechies, Wang and Wu 2016)
    -> (Tx, ssq_freqs, Sfs[, Sx, dSx][, w]); not in upstream, conventions of `ssq_stft2`.  The form of ConceFT for noisy
    band-limited data on a linear frequency grid: J orthonormal tapers h_j (default: `hermite_windows(n_fft, n_tapers)`),
    M random unit vectors r_m in C^J that each give a window sum_j r_mj h_j, and the M first-order synchrosqueezed STFTs
    averaged.  The signal's ridge is where every draw agrees; the noise-driven reassignments differ from draw to draw and
    average down.

    With c = n_fft // 2, V_j the STFT of `x` with h_j and V1_j the one with its spectral derivative (Nyquist term zeroed),
    both run in fp64 for either dtype and rounded once to the call's dtype (padding, hop and `modulated` of `ssq_stft2`):
        gauge      r_m normalised and turned by the unit phase that makes c_m = sum_j r_mj h_j[c] real and positive; a draw
                   with c_m <= 1e-6 sum_j |r_mj| |h_j[c]| is refused
        per draw   S = sum_j r_mj V_j, dS = sum_j r_mj V1_j (j ascending, in the call's dtype);
                   w = fs |k / n_fft - Im(dS / S) / (2 pi)|, kept where |S| > gamma (default 10 eps of the dtype); the bin
                   of w by `ssq_stft2`'s rule on np.linspace(0, fs / 2, F);  Tx[bin, t] += S dw h_0[c] / sum_m c_m
    so `issq_stft(Tx, window=tapers[0])` inverts it at hop_len = 1; with vectors = [[1, 0, ...]] the factor is exactly dw
    and Tx is the first-order squeeze with taper 0.  The 2 J planes are computed once per slice of frames and every draw
    is formed, binned and summed from them in one kernel (csrc/stft_conceft.hip): one thread owns a column of Tx, no
    atomics, the additions into a cell in a fixed order, so the result is bitwise the same run to run, whatever the batch
    and the workspace.

    `tapers`: an ndarray [J, win_len] of real windows (1 <= J <= 8), each sized to `n_fft` as `get_window` sizes one;
    tapers[0][c] must be finite and non-zero.  `vectors` [M, J] complex overrides `n_draws` (1 .. 256) and `seed`; its rows
    are normalised and gauged here.  `Sx`, `dSx` (get_planes=True): the planes V_j, V1_j [J, F, n_frames]; `w`
    (get_w=True): every draw's frequency [M, F, n_frames], real, +inf where a bin is not kept.  A batch [B, N] gives a
    leading B.  `n_fft` must be a power of two from 16 to 4096; the five padtypes.  Anything else raises ValueError
    before any GPU work."""
    lib = _lib.load()
    if isinstance(hop_len, (bool, np.bool_)) or not isinstance(hop_len, (int, np.integer)) or hop_len < 1:
        raise ValueError(f"hop_len {hop_len!r}: must be a positive int")
    hop_len = int(hop_len)
    if tapers is not None:
        if (not isinstance(tapers, np.ndarray) or tapers.ndim != 2 or tapers.dtype.kind not in "fiu"
                or not 1 <= tapers.shape[0] <= CONCEFT_MAX_ORDERS or tapers.shape[1] < 1):
            raise ValueError(f"`tapers` must be a real ndarray [n_tapers, win_len] of 1 .. {CONCEFT_MAX_ORDERS} windows")
        tapers = np.asarray(tapers, dtype=np.float64)
        if not np.isfinite(tapers).all():
            raise ValueError("`tapers` must be finite")
        win0 = tapers[0]
    else:
        if isinstance(n_tapers, (bool, np.bool_)) or not isinstance(n_tapers, (int, np.integer)):
            raise ValueError(f"n_tapers {n_tapers!r}: must be an int")
        if not 1 <= n_tapers <= CONCEFT_MAX_ORDERS:
            raise ValueError(f"n_tapers {n_tapers!r}: 1 .. {CONCEFT_MAX_ORDERS} are built")
        win0 = np.zeros(win_len or 0)                        # (sized below, once n_fft is known)
    f = _stft_front(x, win0, n_fft, win_len, hop_len, fs, t, "conceft_stft")
    if not (math.isfinite(f.fs) and f.fs > 0):
        raise ValueError(f"conceft_stft: fs must be positive and finite (got {f.fs!r})")
    pad = _pad_code(padtype)
    if tapers is None:
        tapers = hermite_windows(win_len or f.n_fft, int(n_tapers))
    wins = np.ascontiguousarray(np.stack([get_window(h, tapers.shape[1], f.n_fft) for h in tapers]))
    J = wins.shape[0]
    adm = wins[:, f.n_fft // 2].copy()
    if not (math.isfinite(adm[0]) and adm[0] != 0):
        raise ValueError("conceft_stft: tapers[0] at the window's centre (index n_fft // 2 once sized) must be finite and "
                         f"non-zero (got {adm[0]!r}): it is the constant `issq_stft` divides by")
    if vectors is None:
        r, c = _conceft_gauge(_conceft_draws(n_draws, J, seed), adm)
    else:
        vectors = np.asarray(vectors)
        if vectors.ndim != 2 or vectors.shape[1] != J or vectors.dtype.kind not in "fiuc":
            raise ValueError(f"`vectors` must be a numeric array [n_draws, {J}] (one column per taper); got shape "
                             f"{vectors.shape}")
        if not 1 <= vectors.shape[0] <= CONCEFT_MAX_DRAWS:
            raise ValueError(f"`vectors`: 1 .. {CONCEFT_MAX_DRAWS} draws are built (got {vectors.shape[0]})")
        r, c = _conceft_gauge(vectors, adm)
    M = r.shape[0]
    scale = float(adm[0] / c.sum())                          # (vectors = e_0: h_0[c] / h_0[c], exactly 1)
    if not (math.isfinite(scale) and scale > 0):
        raise ValueError("conceft_stft: tapers[0] at the window's centre must be positive under the gauge "
                         f"(h_0[c] / sum_m c_m = {scale!r})")
    g = _gamma_arg(gamma)
    if g != g:
        raise ValueError("conceft_stft: gamma is NaN")
    _shape_checked(lib, lib.ssq_conceft_stft_workspace_bytes(f.code, f.batch, f.N, f.n_fft, hop_len, J, None))
    _lib.require_gpu()
    B, F, nfr = _stft_shape(f, hop_len)
    Tx = _lib.pinned_empty((B, F, nfr), f.cdt)
    Sx = _lib.pinned_empty((B, J, F, nfr), f.cdt) if get_planes else None
    dSx = _lib.pinned_empty((B, J, F, nfr), f.cdt) if get_planes else None
    w = _lib.pinned_empty((B, M, F, nfr), f.rdt) if get_w else None
    freqs = np.empty(F, dtype=np.float64)
    _call(lib.ssq_conceft_stft_host(f.code, _ptr(f.xa), f.batch, f.N, _ptr(wins), J, f.n_fft, hop_len, f.fs, pad, _ptr(r),
                                    M, scale, g, _variant(modulated, flipud), 0, _ptr(Tx), _ptr(freqs), _ptr(Sx),
                                    _ptr(dSx), _ptr(w)))
    return (*_unbatch(f.batched, Tx), freqs.astype(f.rdt), _Sfs(f), *_unbatch(f.batched, Sx, dSx, w))


def issq_cwt(Tx, wavelet="gmw", cc=None, cw=None):
    """ssqueezepy.issq_cwt (old/ssqueezepy/_ssq_cwt.py:313-417).  `cc`, `cw` None: the full inverse
    (2 / Css) sum_rows Re Tx, [N] in Tx's real dtype ([B, N] for a batched `Tx` [B, F, N]).  Otherwise curve centres and half-widths (rows of Tx, one per
    column; 1-D: one curve, 2-D [N, K]: K curves, as `extract_ridges` returns them) -> float64 [K + 1, N]: row k < K the
    sum of Re Tx over the rows clip(cc - cw, 0, F) .. clip(cc + cw, 0, F) of each column (none where cc == -1), row K
    the sum over the rows no curve covers, all times 2 / Css.  Extension: a batched Tx [B, F, N] with cc, cw [B, N] or
    [B, N, K] (batched `extract_ridges` output) -> [B, K + 1, N]."""
    comp = _component_args(Tx, cc, cw)
    if comp is not None:
        return _issq_components(*comp, 2.0 / adm_ssq(wavelet))
    return _issq(Tx, 2.0 / adm_ssq(wavelet))


def icwt(Wx, wavelet="gmw", scales="log-piecewise", nv=None, one_int=True, x_len=None, x_mean=0, padtype="reflect",
         rpadded=False, l1_norm=True):
    """ssqueezepy.icwt (old/ssqueezepy/_cwt.py:321-452), one-integral form:
    'log' scales:    (2 / Cpsi) ln(2^(1/nv)) sum_a Re Wx[a] / (1 or sqrt(a)) + x_mean;
    'linear':        (2 / Cpsi) (pi / 4) sum_a Re Wx[a] / (a or a^1.5) + x_mean (:438-448, :477-492);
    'log-piecewise': the 'log' inverses of the two segments either side of the transition, summed (:418-427; each
                     adds x_mean, as upstream's do).
    Extension: a batch `Wx` [B, na, N] -> [B, N]; `x_mean` a scalar or one value per signal."""
    if not one_int:
        raise ValueError("only the one-integral inverse (one_int=True) is built")
    s, scaletype, _nv, s_own = _scales(scales)
    _full_map(Wx, "Wx")
    if Wx.shape[-2] != len(s):
        raise _RowCountError("%s != %s" % (len(s), Wx.shape[-2]))
    if Wx.ndim == 3:                                        # one mean per signal, or one for all
        xm = np.asarray(x_mean)
        if xm.ndim > 1 or (xm.ndim == 1 and xm.shape[0] != Wx.shape[0]):
            raise ValueError(f"`x_mean` must be a scalar or one value per signal ({Wx.shape[0]}); got shape {xm.shape}")
    if scaletype == "log-piecewise":                        # the segments in the caller's dtype, as upstream splits them
        idx = logscale_transition_idx(s_own)
        kw = dict(wavelet=wavelet, one_int=one_int, x_len=x_len, x_mean=x_mean, padtype=padtype, rpadded=rpadded,
                  l1_norm=l1_norm)
        return icwt(Wx[..., :idx, :], scales=s_own[:idx], **kw) + icwt(Wx[..., idx:, :], scales=s_own[idx:], **kw)
    if scaletype == "linear":
        x = _issq(Wx, (2.0 / adm_ssq(wavelet)) * np.pi / 4, 1.0 / (s if l1_norm else s ** 1.5))
    else:
        x = _issq(Wx, (2.0 / adm_ssq(wavelet)) * np.log(2 ** (1 / _nv)), None if l1_norm else 1.0 / np.sqrt(s))
    if Wx.ndim == 3 and np.ndim(x_mean) == 1:               # a column in x's dtype: what a Python float per 2-D call adds
        return x + np.asarray(x_mean).reshape(-1, 1).astype(x.dtype)
    return x + x_mean


# --------------------------------------------------------------------------------- synchrosqueezing a transform ----
SSQUEEZE_MODES = {"sum": 0, "lebesgue": 1, "abs": 2}   # include/ssq_hip.h: SSQ_SQUEEZE_SUM, _LEBESGUE, _ABS


def _cmap(A, name):
    """A 2-D [F, N] or batched 3-D [B, F, N] complex64 / complex128 map -> (A [B, F, N] contiguous, batched, code)."""
    if not isinstance(A, np.ndarray) or A.ndim not in (2, 3) or A.dtype not in (np.complex64, np.complex128):
        raise TypeError(f"`{name}` must be a 2D [F, N] (or batched 3D [B, F, N]) complex64 / complex128 ndarray")
    batched = A.ndim == 3
    return np.ascontiguousarray(A if batched else A[None]), batched, _ccode(A.dtype)


def _like(B, A, name):
    """`B` as a complex array of `A`'s shape and dtype ([B, F, N] contiguous)."""
    if not isinstance(B, np.ndarray) or B.shape != A.shape or B.dtype.kind != "c":
        raise ValueError(f"`{name}` must be a complex ndarray of the shape of `Wx` {A.shape}")
    return np.ascontiguousarray(B if B.ndim == 3 else B[None], dtype=A.dtype)


def _sfs_rows(Sfs, F, rdt):
    sfs = np.ascontiguousarray(np.asarray(Sfs).reshape(-1), dtype=rdt)
    if len(sfs) != F:
        raise ValueError(f"`Sfs` must have one frequency per row of `Sx` ({len(sfs)} != {F})")
    return sfs


def _phase(Wx, dWx, Sfs, gamma):
    Wb, batched, code = _cmap(Wx, "Wx")
    dWb = _like(dWx, Wx, "dWx")
    B, F, N = Wb.shape
    rdt = _rdtype(code)
    sfs = None if Sfs is None else _sfs_rows(Sfs, F, rdt)
    lib = _lib.load()
    _lib.require_gpu()
    w = np.empty((B, F, N), dtype=rdt)
    _call(lib.ssq_phase_host(code, _ptr(Wb), _ptr(dWb), _ptr(sfs), B, F, N, float(gamma), _ptr(w)))
    return _unbatch(batched, w)[0]


def phase_cwt(Wx, dWx, difftype="trig", gamma=None, parallel=None):
    """ssqueezepy.phase_cwt (old/ssqueezepy/_ssq_cwt.py:420-509, algos.py:706-741): w = |Im(dWx / Wx)| / (2 pi), real in
    Wx's real dtype, +inf where |Wx| < gamma.  `gamma=None` is upstream's default here, sqrt(eps) of the dtype (:488-489;
    ssq_cwt passes 10 eps).  `parallel` is accepted and unused."""
    if difftype != "trig":
        raise ValueError(f"difftype {difftype!r}: only 'trig' is built")
    _, _, code = _cmap(Wx, "Wx")
    if gamma is None:
        gamma = math.sqrt(_eps(code))
    return _phase(Wx, dWx, None, gamma)


def phase_stft(Sx, dSx, Sfs, gamma=None, parallel=None):
    """ssqueezepy.phase_stft (old/ssqueezepy/_ssq_stft.py:200-246, algos.py:784-816): w = |Sfs[row] - Im(dSx / Sx) /
    (2 pi)|, +inf where |Sx| < gamma; `gamma=None` is 10 eps of the dtype.  `parallel` is accepted and unused."""
    _, _, code = _cmap(Sx, "Sx")
    if gamma is None:
        gamma = 10 * _eps(code)
    if Sfs is None:
        raise ValueError("`Sfs` must be given")
    return _phase(Sx, dSx, Sfs, gamma)


def ssqueeze(Wx, w=None, ssq_freqs=None, scales=None, Sfs=None, fs=None, t=None, squeezing="sum", maprange="maximal",
             wavelet=None, gamma=None, was_padded=True, flipud=False, dWx=None, transform="cwt"):
    """ssqueezepy.ssqueeze (old/ssqueezepy/ssqueezing.py:13-245) -> (Tx, ssq_freqs) on a transform the caller holds:
    `Wx` [F, N] (or a batch [B, F, N], one launch) complex64 / complex128 with `w` (its phase transform) or `dWx`.
    From `w`, a value counts where w is finite (algos.py:173-252); from `dWx`, where |Wx| > gamma (:860-968), with the
    kernels of ssq_cwt / ssq_stft.  `gamma=None` (upstream requires it with `dWx`) is 10 eps of the dtype, what ssq_cwt
    and ssq_stft pass.  squeezing 'sum', 'lebesgue' (1 / F per row: a batch squeezes as its signals one by one),
    'abs' (real Tx) or a function applied to `Wx` here (its complex result is cast to Wx's dtype; a real one gives a
    real Tx); with `dWx` only 'sum' (upstream would take the phase from the replaced `Wx` too).  Not built, raising
    ValueError: maprange 'energy' or a tuple; transform 'stft' without an array `ssq_freqs` or, from `dWx`, without
    `Sfs` or with ssq_freqs[0] != Sfs[0] (pass `w = phase_stft(...)` instead)."""
    # ---- every refusal before any GPU work
    if transform not in ("cwt", "stft"):
        raise ValueError("`transform` must be one of: cwt, stft (got %s)" % transform)
    Wb, batched, code = _cmap(Wx, "Wx")
    B, F, N = Wb.shape
    rdt = _rdtype(code)
    if w is None and dWx is None:
        raise ValueError("if `w` is None, `dWx` must not be")
    if w is not None:
        w = np.asarray(w)
        if w.shape != Wx.shape or w.dtype.kind not in "fiu":
            raise ValueError(f"`w` must be a real ndarray of the shape of `Wx` {Wx.shape}")
        if w.min() < 0:
            raise ValueError("found negatives in `w`")
    if callable(squeezing) and not isinstance(squeezing, str):
        mode = None
    elif isinstance(squeezing, str) and squeezing in SSQUEEZE_MODES:
        mode = squeezing
    else:
        raise ValueError(f"squeezing {squeezing!r}: 'sum', 'lebesgue', 'abs' or a function")
    if w is None and squeezing != "sum":
        raise ValueError(f"squeezing {squeezing!r} with `w=None`: only 'sum' is built from `dWx` (upstream takes the "
                         "phase from the replaced `Wx` too); compute `w = phase_cwt(Wx, dWx)` / `phase_stft` first")
    if isinstance(maprange, (tuple, list)) or maprange == "energy":
        raise ValueError(f"maprange {maprange!r}: 'peak' and 'maximal' are built")
    if maprange not in ("peak", "maximal"):
        raise ValueError(f"maprange {maprange!r}: must be one of 'maximal', 'peak'")
    dt = _dt(fs, t, N)
    f_idx = Sfs_t = None
    if transform == "cwt":
        if scales is None:
            raise ValueError("`scales` can't be None if `transform == 'cwt'`")
        s, cwt_scaletype, _nv, s_own = _scales(scales)
        if len(s) != F:
            raise ValueError("`scales` must have one scale per row of `Wx` (%s != %s)" % (len(s), F))
        row_const = _row_const(s, cwt_scaletype, _nv)                                   # ssqueezing.py:122-127

        def generate(scaletype):
            if maprange == "peak" and wavelet is None:
                raise ValueError("`wavelet` must be given with maprange 'peak'")
            wcode, p0, p1 = _wavelet(wavelet) if wavelet is not None else (0, 0.0, 0.0)
            return _ssq_freqs(s, N, wcode, p0, p1, dt, maprange, scaletype, s_own, was_padded)
        f_asc, scaletype, f_idx = _freq_type(ssq_freqs, cwt_scaletype, maprange, generate)
        if not isinstance(ssq_freqs, np.ndarray):
            ssq_freqs = f_asc
    else:
        if not isinstance(ssq_freqs, np.ndarray):
            raise ValueError("transform 'stft': `ssq_freqs` must be an array (ssq_stft passes Sfs)")
        f_own = _own_dtype(ssq_freqs)
        f_asc, scaletype = np.ascontiguousarray(f_own, dtype=np.float64), "linear"       # :189-191
        row_const = np.full(F, float(f_own[1] - f_own[0]))                               # :129-130
        if w is None:
            if Sfs is None:
                raise ValueError("transform 'stft' with `w=None`: `Sfs` must be given")
            Sfs_t = _sfs_rows(Sfs, F, rdt)
            if Sfs_t[0] != rdt(f_own[0]):
                raise ValueError("transform 'stft' with `w=None` bins from Sfs[0]: ssq_freqs[0] != Sfs[0] is not "
                                 "built; pass `w = phase_stft(Sx, dSx, Sfs)` instead")
    if len(f_asc) != F:
        raise ValueError("`ssq_freqs` must have one frequency per row of `Wx` (%s != %s)" % (len(f_asc), F))
    kind, trans = FREQS[scaletype], f_idx or 0
    # ---- `Wx` replaced as ssqueezing.py:183-188 does
    real_out = mode == "abs"
    if mode is None:
        Wv = np.asarray(squeezing(Wx))
        if Wv.shape != Wx.shape:
            raise ValueError(f"`squeezing` must return an array of the shape of `Wx` {Wx.shape} (got {Wv.shape})")
        real_out = Wv.dtype.kind != "c"
        Wb = np.ascontiguousarray(Wv if batched else Wv[None], dtype=Wb.dtype)
        mode = "sum"
    lib = _lib.load()
    _lib.require_gpu()
    if w is not None:
        wb = np.ascontiguousarray(w if batched else w[None], dtype=rdt)
        Tx = np.empty((B, F, N), dtype=rdt if mode == "abs" else Wb.dtype)
        _call(lib.ssq_ssqueeze_w_host(code, None if mode == "lebesgue" else _ptr(Wb), _ptr(wb), B, F, N,
                                      _ptr(row_const), _ptr(f_asc), kind, trans, SSQUEEZE_MODES[mode], int(bool(flipud)),
                                      _ptr(Tx)))
    else:
        dWb = _like(dWx, Wx, "dWx")
        g = 10 * _eps(code) if gamma is None else float(gamma)
        Tx = np.empty((B, F, N), dtype=Wb.dtype)
        _call(lib.ssq_ssqueeze_dwx_host(code, _ptr(Wb), _ptr(dWb), _ptr(Sfs_t), B, F, N, _ptr(row_const), _ptr(f_asc),
                                        kind, trans, SSQUEEZE_MODES[mode], int(bool(flipud)), g, _ptr(Tx)))
    if real_out and Tx.dtype.kind == "c":
        Tx = np.ascontiguousarray(Tx.real)
    if transform == "cwt" or flipud:                                                     # :199-205
        ssq_freqs = ssq_freqs[::-1]
    return _unbatch(batched, Tx)[0], ssq_freqs


# ---------------------------------------------------------------------------------------------- ridge extraction ----
def extract_ridges(Tf, scales, penalty=2., n_ridges=1, bw=15, transform='cwt', get_params=False, parallel=True):
    """ssqueezepy.extract_ridges (old/ssqueezepy/ridge_extraction.py:11-146) -> ridge_idxs [N, n_ridges] int64, or
    (ridge_idxs, ridge_f, ridge_e) with get_params.  Extension: a 3-D `Tf` [B, F, N] is a batch (outputs get a leading
    B).  dtypes as upstream (:113-121): the parameter dtype (scales, eps, penalty, ridge_f, ridge_e) is float64 only
    for complex128 `Tf`; the cost and DP run in the dtype of |Tf|**2 (fp64 for float64 or integer `Tf`).  The metric
    log(scales) / scales (:118-120) is formed here in NumPy; everything per element runs in HIP kernels.  The backward
    trace is upstream's serial one (:206-215): `parallel` is accepted and ignored (its prange kernel, :217-232, races
    when two rows match)."""
    lib = _lib.load()
    Tf = np.asarray(Tf)
    if Tf.ndim not in (2, 3):
        raise ValueError("`Tf` must be 2D [F, N] or 3D [B, F, N]")
    batched = Tf.ndim == 3
    Tb = Tf if batched else Tf[None]
    B, F, N = Tb.shape
    if Tf.dtype == np.complex128:
        code, pcode, cplx, src = SSQ_F64, SSQ_F64, 1, Tb
    elif Tf.dtype == np.complex64:
        code, pcode, cplx, src = SSQ_F32, SSQ_F32, 1, Tb
    elif Tf.dtype == np.float32:
        code, pcode, cplx, src = SSQ_F32, SSQ_F32, 0, Tb
    elif Tf.dtype == np.float64 or Tf.dtype.kind in "biu":    # integers: |x|**2 is exact in fp64 for |x| < 2**26
        code, pcode, cplx, src = SSQ_F64, SSQ_F32, 0, Tb.astype(np.float64, copy=False)
    else:
        raise TypeError(f"`Tf` dtype {Tf.dtype}: complex64/128, float32/64 or integer are supported")
    pdt = _rdtype(pcode)
    s = np.asarray(scales, dtype=pdt)
    if s.ndim > 2 or (s.ndim == 2 and s.shape[1] != 1) or s.size != F:
        raise ValueError(f"`scales` must have shape ({F},) or ({F}, 1) to match `Tf`, got {s.shape}")
    if int(n_ridges) != n_ridges or n_ridges < 1:
        raise ValueError("`n_ridges` must be an integer >= 1")
    if not np.isfinite(bw) or bw < 0:
        raise ValueError("`bw` must be finite and >= 0")
    scales_orig = np.ascontiguousarray(s.reshape(-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        metric = np.ascontiguousarray((np.log(scales_orig) if transform == 'cwt' else scales_orig).reshape(-1))
    pen = float(np.asarray(penalty, dtype=pdt))
    n_ridges = int(n_ridges)
    _lib.require_gpu()
    src = np.ascontiguousarray(src)
    ridge_idxs = np.empty((B, N, n_ridges), dtype=np.int64)
    ridge_f = np.empty((B, N, n_ridges), dtype=pdt) if get_params else None
    ridge_e = np.empty((B, N, n_ridges), dtype=pdt) if get_params else None
    _call(lib.ssq_extract_ridges_host(code, pcode, cplx, _ptr(src), B, F, N, _ptr(metric), _ptr(scales_orig), pen,
                                      n_ridges, float(bw), _ptr(ridge_idxs), _ptr(ridge_f), _ptr(ridge_e), None))
    out = _unbatch(batched, ridge_idxs, ridge_f, ridge_e)
    return tuple(out) if get_params else out[0]
