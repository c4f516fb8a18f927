"""NumPy model of the fused STFT kernels' per-column fixed-point scatter (csrc/stft_fused_kernel.h, the epilogue of
`stft_fused_kernel` and of `stft_tx1024_kernel`), the inputs that stress it, and the bound the tests hold it to.

The scheme, per column (frame) j, for weights c = Sx (sum mode) or 1/n_freqs (Lebesgue) of the kept bins:
  tot   = fl(fl(sum |Re c| + |Im c|) * dw)                       the column's L1 mass, in T
  e     = frexp exponent of tot (tot < 2^e), clamped below at EMIN (-90 fp32, -960 fp64)
  scale = dw * 2^(FRAC - e), inv = 2^(e - FRAC)                  FRAC = 30 (fp32), 50 (fp64); powers of two: exact
  i     = round(fl(c * scale))                                   fp32: floor(v + 1/2); fp64: nearest-even
  cell  = integer sum of i over the bins that land on the row    exact, order independent
  Tx    = fl(T(cell)) * inv                                      the conversion rounds in fp32 (|cell| can pass 2^24)
  tot not finite (NaN/Inf in the frame): the whole column comes out NaN.

Bound (a) of tests/test_gpu_stft_scatter.py, for every column j, against the float64 re-accumulation Tx_re of the same
weights and bins:        max_k |Tx[k, j] - Tx_re[k, j]| <= B * tot_j,   tot_j = dw * sum_kept (|Re c| + |Im c|).
Derivation (per cell, in units of tot_j):
  1. one contribution's integer rounding is at most one unit (1/2 in fp64, 1/2 + 1 ulp in fp32's floor(v + 1/2));
  2. the unit is 2^(e - FRAC) <= 4 * tot_j * 2^-FRAC: 2^(e-1) <= tot, and one more factor of two for e landing one
     high because tot is a rounded sum (or, in a test, because Sx comes from another instantiation of the kernel);
  3. a cell receives at most n_freqs contributions                      -> 4 * n_freqs * 2^-FRAC;
  4. the products fl(c * scale) are off by 2^-p |c * scale| each (p = 24 or 53), over the whole column at most
     2^-p * 2^FRAC units = 2^-p * 2^FRAC * 4 * 2^-FRAC * tot_j: 4 * 2^-24 = 64 * 4 * 2^-30 (fp32), 2^-51 = 2 * 2^-50 (fp64);
  5. the read-out conversion T(cell) adds one ulp of the cell's value (<= tot_j): 2^-24 in fp32, exact in fp64
     (|cell| < 2^51); the Sx the test re-accumulates comes from the debug instantiation and may differ by an ulp per
     bin from the Tx instantiation's: another 2^-24 resp. 2^-53 of tot_j; the fp32 weight dw itself is exact (the
     re-accumulation uses fl32(dw)).
Sum:  B32 = (4 n_freqs + 256) 2^-30 + 2^-21      (2^-21 = 8 ulp(fp32): the issue's allowance for step 5)
      B64 = (4 n_freqs + 8) 2^-50
"""
import math

import numpy as np

from oracle import ssq_oracle as o

FRAC = {4: 30, 8: 50}
EMIN = {4: -90, 8: -960}


def bound(n_freqs: int, dtype) -> float:
    """B of the module docstring."""
    if np.dtype(dtype).itemsize == 4:
        return (4 * n_freqs + 256) * 2.0 ** -30 + 2.0 ** -21
    return (4 * n_freqs + 8) * 2.0 ** -50


def weights(Sx, keep, lebesgue: bool):
    """The scattered weight c of every bin (0 where the bin is skipped), complex128."""
    n = Sx.shape[0]
    c = np.full(Sx.shape, 1.0 / float(n), dtype=np.complex128) if lebesgue else Sx.astype(np.complex128)
    return np.where(keep, c, 0.0)


def column_mass(c, dw: float):
    """tot_j = dw * sum over the kept bins of |Re c| + |Im c| (float64)."""
    return dw * (np.abs(c.real) + np.abs(c.imag)).sum(0)


def scatter_model(Sx, k, keep, dw: float, n_out: int, dtype, lebesgue: bool = False):
    """The kernels' fixed-point scatter of weights(Sx) into rows k, in `dtype` arithmetic.  Returns (Tx, e)."""
    T = np.dtype(dtype).type
    sz = np.dtype(dtype).itemsize
    frac, emin = FRAC[sz], EMIN[sz]
    c = weights(Sx, keep, lebesgue)
    cr, ci = c.real.astype(T), c.imag.astype(T)
    dwT = T(dw)
    with np.errstate(all="ignore"):
        l1 = (np.abs(cr).astype(np.float64) + np.abs(ci).astype(np.float64)).sum(0).astype(T)
        tot = (l1 * dwT).astype(T)
    bad = ~np.isfinite(tot)
    _, e = np.frexp(np.where(bad, 0, tot).astype(np.float64))
    if sz == 4:
        e = np.where(tot < T(2.0 ** -126), -126, e)     # exponent field 0 (zero, subnormal) reads as 2^-126
    e = np.maximum(e, emin).astype(np.int64)
    scale = (np.ldexp(np.float64(dwT), frac - e)).astype(T)        # dw * 2^(FRAC - e): exact
    inv = np.ldexp(1.0, e - frac)
    with np.errstate(all="ignore"):
        pr, pi = (cr * scale[None, :]).astype(T), (ci * scale[None, :]).astype(T)
    if sz == 4:
        ir, ii = np.floor(pr.astype(np.float64) + 0.5), np.floor(pi.astype(np.float64) + 0.5)
    else:
        ir, ii = np.rint(pr), np.rint(pi)
    ir = np.where(keep & ~bad[None, :], ir, 0).astype(np.int64)
    ii = np.where(keep & ~bad[None, :], ii, 0).astype(np.int64)
    cols = np.broadcast_to(np.arange(Sx.shape[1]), Sx.shape)
    rows = np.where(keep, k, 0)
    acc_r = np.zeros((n_out, Sx.shape[1]), dtype=np.int64)
    acc_i = np.zeros_like(acc_r)
    np.add.at(acc_r, (rows, cols), ir)
    np.add.at(acc_i, (rows, cols), ii)
    lim = 2 ** 31 if sz == 4 else 2 ** 51
    assert np.abs(acc_r).max(initial=0) < lim and np.abs(acc_i).max(initial=0) < lim, "a partial sum left the cell"
    Tx = (acc_r.astype(T).astype(np.float64) * inv[None, :]) + 1j * (acc_i.astype(T).astype(np.float64) * inv[None, :])
    Tx[:, bad] = np.nan
    return Tx.astype(np.complex64 if sz == 4 else np.complex128), e


def worst_ratio(Tx, Sx, k, keep, dw: float, dtype, lebesgue: bool = False):
    """max over the columns of  max_k |Tx - Tx_re| / (B * tot_j)  (columns of zero mass must be exactly zero: they
    count as 0 when they are and as inf when they are not).  Tx_re: float64 re-accumulation of the same weights."""
    n_out = Tx.shape[0]
    c = weights(Sx, keep, lebesgue)
    Tx_re = o.accumulate_tx(Sx.astype(np.complex128), np.where(keep, k, 0), keep, dw, n_out, lebesgue=lebesgue)
    tot = column_mass(c, dw)
    err = np.abs(Tx.astype(np.complex128) - Tx_re).max(0)
    B = bound(Sx.shape[0], dtype)
    with np.errstate(all="ignore"):
        r = np.where(tot > 0, err / (B * tot), np.where(err == 0, 0.0, np.inf))
    return float(np.nan_to_num(r, nan=np.inf).max(initial=0.0)), r


# ------------------------------------------------------------------ configurations and inputs of the scatter tests ----
# (dtype, n_fft, hop, frames per tile F of the kernel that serves Tx)
CONFIGS = [
    (np.float32, 1024, 256, 16),     # stft_tx1024_kernel
    (np.float32, 256, 64, 32),
    (np.float32, 1000, 250, 16),     # mixed radix inside the 1024-point kernel
    (np.float64, 1024, 256, 8),      # SPLIT
    (np.float64, 256, 64, 16),
]
PADS = ("reflect", "zero")
INPUTS = ("geometric_tone", "plus_one", "minus_one", "nyquist", "impulse_train", "bursts")
M_LIST = {np.float32: (-30, -7, 13, 40), np.float64: (-30, -7, 13, 40, 200, 400)}
# synth_signal seeds of 3(c), per configuration: chosen (by search on the float64 oracle, both paddings) so that the
# weakest bin stays clear of 2^6 * gamma * 2^30 = 1.5e-4, i.e. m = -30 meets its precondition with the default gamma
EQUIV_SEEDS = {"float32-1024-256": 32, "float32-256-64": 66, "float32-1000-250": 11, "float64-1024-256": 70,
               "float64-256-64": 11}


def config_id(cfg):
    return f"{np.dtype(cfg[0]).name}-{cfg[1]}-{cfg[2]}"


def equivariance_signal(cfg):
    dtype, n_fft, hop, F = cfg
    return o.synth_signal(3 * F * hop + 77, EQUIV_SEEDS[config_id(cfg)], dtype)


def make_input(name: str, n_fft: int, hop: int, F: int, dtype):
    """The inputs of 3(b).  About three tiles (3 F hop samples, odd remainder), except the tone, which needs the
    281 hops its amplitude takes to climb from 2^-20 to 2^20 by 2^(1/7) per hop."""
    N = 3 * F * hop + hop // 2 + 3
    n = np.arange(N, dtype=np.float64)
    if name == "geometric_tone":
        N = 281 * hop
        n = np.arange(N, dtype=np.float64)
        assert n_fft % 8 == 0                                      # frequency 1/8: the centre of bin n_fft / 8
        x = np.exp2(-20.0 + n / (7.0 * hop)) * np.cos(2.0 * math.pi * (n % 8) / 8.0)
    elif name == "plus_one":
        x = np.ones(N)
    elif name == "minus_one":
        x = -np.ones(N)
    elif name == "nyquist":
        x = 1.0 - 2.0 * (n % 2)
    elif name == "impulse_train":
        x = (n % hop == 0).astype(np.float64)
    elif name == "bursts":
        gap = n_fft + F * hop + hop + 1                            # longer than a frame plus a whole tile of hops
        burst = F * hop + 37
        x = np.concatenate([o.synth_signal(burst, 3, np.float64), np.zeros(gap), o.synth_signal(burst, 4, np.float64),
                            np.zeros(gap)])
    else:
        raise ValueError(name)
    return x.astype(dtype)


def silent_columns(x, n_fft: int, hop: int, pad: str):
    """Columns whose frame (padding included) holds only zeros."""
    padded = o.stft_pad(np.asarray(x, dtype=np.float64), n_fft, pad)
    n_frames = o.stft_frames(padded.shape[0], n_fft, hop)
    nz = np.concatenate([[0], np.cumsum(padded != 0)])
    start = np.arange(n_frames) * hop
    return (nz[start + n_fft] - nz[start]) == 0


def frames_covering(sample: int, n_frames: int, n_fft: int, hop: int):
    """Columns whose frame reads original sample `sample` (reflect or zero padding of a signal much longer than
    n_fft: the mirror of a sample within n_fft of an end is not considered -- keep `sample` in the interior)."""
    start = np.arange(n_frames) * hop - (n_fft - 1) // 2
    return (start <= sample) & (sample < start + n_fft)


def equivariance_preconditions(Sx, m: int, gamma: float, two_pi_eff: float, dtype):
    """3(c): from the float64 oracle's Sx.  Returns the list of violated preconditions (empty: the case runs)."""
    a = np.abs(Sx)
    s = math.ldexp(1.0, m)
    bad = []
    for scale in (1.0, s):
        near = (a * scale >= gamma / 64.0) & (a * scale <= gamma * 64.0)
        if near.any():
            bad.append(f"{int(near.sum())} bins within 2^6 of gamma at scale {scale:g}")
    if ((a >= gamma) != (a * s >= gamma)).any():
        bad.append("bins cross gamma")
    top = 120 if np.dtype(dtype).itemsize == 4 else 1000
    mx = a.max()
    if 2.0 * math.log2(mx) + 2 * m + math.log2(two_pi_eff) >= top:
        bad.append("|Sx|^2 leaves the range")
    return bad


def two_pi_eff(win, fs: float = 1.0) -> float:
    """2 pi alpha of the fused kernels: alpha = the power of two that balances the window and its derivative channel
    (api_stft.hip: frexp(max|g| / max|g' fs|) -> 2^(e-1))."""
    g = np.asarray(win, dtype=np.float64)
    gd = o.diff_window(g) * fs
    _, e = math.frexp(np.abs(g).max() / np.abs(gd).max())
    return 2.0 * math.pi * math.ldexp(1.0, e - 1)
