"""GPU tests of the fused STFT kernels' fixed-point scatter at the edges of its number range.

The existing parity tests compare Tx relative to the GLOBAL maximum on O(1) signals; the scatter works per COLUMN
(`column_scale`: 2^e > tot_j, contributions rounded to 30 resp. 50 fractional bits; `stft_tx1024_kernel` packs
IM * 2^32 + RE + 2^31 into one 64-bit LDS atomic).  Here, for fp32 1024/256 (tx1024), 256/64, 1000/250 and fp64 1024/256
(SPLIT), 256/64, each with both paddings:

 (a) per column j:  max_k |Tx[k, j] - Tx_re[k, j]| <= B * tot_j,  Tx_re the float64 re-accumulation of the kernel's own
     Sx and k,  tot_j = dw * sum over the kept bins of |Re c| + |Im c|,
         B32 = (4 n_freqs + 256) 2^-30 + 2^-21,   B64 = (4 n_freqs + 8) 2^-50,
     derived from the code, not measured: tests/helpers/scatter_model.py states the derivation step by step, and
     tests/test_scatter_model.py shows on the CPU that a NumPy model of the scheme meets it on these very inputs;
 (b) on inputs that stress the scheme: a bin-centre tone growing by 2^(1/7) per hop from 2^-20 to 2^20 (all the mass in
     one cell, every mantissa of tot, quiet columns next to loud ones), x = +1 and x = -1 (single-signed pile-up in row
     0; the negative one exercises the packed cell's borrow), the Nyquist tone (the q == 8, t == 0 lane), an impulse
     train of period hop (flat spectrum, every bin kept), bursts separated by exact silence longer than a frame plus a
     tile (silent columns: exactly 0, no NaN);
 (c) power-of-two equivariance: Tx(2^m x) == 2^m Tx(x) BITWISE with identical k and keep mask, m in {-30, -7, 13, 40}
     (fp64 also 200, 400; -200 cannot meet the precondition with the default gamma: every bin falls below it).  The
     kernels' scales are powers of two and v_rcp is exponent-invariant, so nothing but the exponents may change.
     Preconditions, checked here from the float64 oracle: no bin within 2^6 of gamma before or after scaling, none
     crosses gamma, max|Sx|^2 2^(2m) two_pi_eff < 2^120 (fp32) / 2^1000 (fp64).  m = -70: every bin is below gamma,
     Tx is exactly zero;
 (d) NaN locality through Tx: one NaN sample -> columns whose frame does not read it are bitwise those of the clean
     run, the others carry NaN in row 0 (where the reference's scan puts a NaN bin); in Lebesgue mode, where the weight
     is the constant 1/n_freqs, row 0 of those columns holds dw and the other rows 0, as in the reference.
k and the keep mask follow the existing rules on the kernel's own w and Sx (tests/helpers/binrule.py, the fp32 bin
model, the first-minimum scan).  Every case prints its worst err / (B tot_j): DESIGN.md §4.1.1 quotes them.
"""
import math

import numpy as np
import pytest

from oracle import ssq_oracle as o
from ssqueeze_rs_amd import _rs
from tests.helpers import scatter_model as sm
from tests.helpers.binrule import stft_bins_follow_reference_rule

pytestmark = pytest.mark.gpu

GAMMA = o.DEFAULT_GAMMA


def _run(x, n_fft, hop, pad, squeezing="sum"):
    return _rs.ssq_stft(x, np.hanning(n_fft), n_fft=n_fft, hop_len=hop, fs=1.0, padtype=pad, squeezing=squeezing,
                        _debug=True)


def _check_bins_and_keep(dtype, Sx, w, k, f):
    """The existing rules, on the kernel's own Sx and w."""
    keep = k >= 0
    a = np.abs(Sx.astype(np.complex128))
    fin = np.isfinite(w)
    assert keep[(a > 2 * GAMMA) & fin].all(), "a bin above gamma was skipped"
    assert not keep[a < GAMMA / 2].any(), "a bin below gamma was kept"
    dw = f[1] - f[0]
    if dtype == np.float32:
        assert np.isfinite(w[keep]).all()
        stft_bins_follow_reference_rule(k, w, f, keep)
        assert np.array_equal(k[keep], o.stft_bins_f32_model(w[keep], dw, f.shape[0]))
    else:
        kk, ww = k[keep], w[keep]
        diff = kk != o.nearest_bin_first_min(ww, f)
        if diff.any():                                       # only next to a half-bin tie
            tq = ww[diff] / dw
            assert (np.abs(tq - np.floor(tq) - 0.5) < 1e-9 * np.maximum(1.0, np.abs(tq))).all()
    return keep


def _check_columns(tag, dtype, Tx, Sx, k, keep, f, lebesgue=False):
    """(a): every column within B * tot_j of the float64 re-accumulation of the kernel's own Sx and k."""
    dw = float(dtype(f[1] - f[0]))
    worst, r = sm.worst_ratio(Tx, Sx, k, keep, dw, dtype, lebesgue=lebesgue)
    print(f"SCATTER {tag}: worst err/(B*tot_j) = {worst:.4f} at column {int(np.argmax(r))} of {r.shape[0]}")
    assert np.isfinite(Tx.view(dtype)).all(), tag
    assert worst <= 1.0, (tag, worst, int(np.argmax(r)))
    return worst


@pytest.mark.parametrize("cfg", sm.CONFIGS, ids=sm.config_id)
@pytest.mark.parametrize("pad", sm.PADS)
@pytest.mark.parametrize("name", sm.INPUTS)
def test_per_column_bound_on_stress_inputs(cfg, pad, name):
    dtype, n_fft, hop, F = cfg
    x = sm.make_input(name, n_fft, hop, F, dtype)
    Tx, f, dbg = _run(x, n_fft, hop, pad)
    keep = _check_bins_and_keep(dtype, dbg["Sx"], dbg["w"], dbg["k"], f)
    _check_columns(f"{sm.config_id(cfg)} {pad} {name}", dtype, Tx, dbg["Sx"], dbg["k"], keep, f)
    if name == "bursts":
        silent = sm.silent_columns(x, n_fft, hop, pad)
        assert silent.sum() >= F
        assert not keep[:, silent].any()
        assert not Tx[:, silent].any()                        # exactly 0 (and so no NaN)
        assert (np.abs(Tx[:, ~silent]).max(0) > 0).all()
    if name in ("bursts", "impulse_train"):
        TxL, fL, dL = _run(x, n_fft, hop, pad, "lebesgue")
        keepL = _check_bins_and_keep(dtype, dL["Sx"], dL["w"], dL["k"], fL)
        _check_columns(f"{sm.config_id(cfg)} {pad} {name} lebesgue", dtype, TxL, dL["Sx"], dL["k"], keepL, fL, True)
    if name in ("plus_one", "minus_one"):
        # interior columns: single-signed real contributions pile into row 0
        j = Tx.shape[1] // 2
        assert (Tx[0, j].real > 0) == (name == "plus_one") and np.abs(Tx[:, j]).argmax() == 0


@pytest.mark.parametrize("cfg", sm.CONFIGS, ids=sm.config_id)
@pytest.mark.parametrize("pad", sm.PADS)
def test_power_of_two_equivariance(cfg, pad):
    dtype, n_fft, hop, F = cfg
    x = sm.equivariance_signal(cfg)
    _, _, im = o.ssq_stft(x.astype(np.float64), np.hanning(n_fft), n_fft=n_fft, hop_len=hop, fs=1.0, padtype=pad,
                          return_intermediates=True)
    tpe = sm.two_pi_eff(np.hanning(n_fft))
    Tx, f, dbg = _run(x, n_fft, hop, pad)
    skipped = []
    for m in sm.M_LIST[dtype]:
        why = sm.equivariance_preconditions(im["Sx"], m, GAMMA, tpe, dtype)
        if why:
            skipped.append((m, why))
            continue
        s = dtype(math.ldexp(1.0, m))
        Tm, _, dm = _run(x * s, n_fft, hop, pad)
        assert np.array_equal(dm["k"], dbg["k"]), (m, int((dm["k"] != dbg["k"]).sum()))
        assert np.array_equal(dm["Sx"], dbg["Sx"] * s), m
        assert np.array_equal(dm["w"], dbg["w"], equal_nan=True), m
        bad = Tm != Tx * s
        assert not bad.any(), (m, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert len(skipped) <= 1, skipped
    T0, _, d0 = _run(x * dtype(2.0 ** -70), n_fft, hop, pad)      # far below the default gamma: nothing is kept
    assert (np.abs(im["Sx"]) * 2.0 ** -70 < GAMMA / 64).all()
    assert not (d0["k"] >= 0).any() and not T0.any()


@pytest.mark.parametrize("cfg", [sm.CONFIGS[0], sm.CONFIGS[1], sm.CONFIGS[4]], ids=sm.config_id)
@pytest.mark.parametrize("pad", sm.PADS)
@pytest.mark.parametrize("squeezing", ["sum", "lebesgue"])
def test_nan_stays_in_the_columns_that_read_it(cfg, pad, squeezing):
    dtype, n_fft, hop, F = cfg
    x = o.synth_signal(3 * F * hop + 77, 17, dtype)
    clean, f, _ = _run(x, n_fft, hop, pad, squeezing)
    xp = x.copy()
    sample = x.shape[0] // 2 + 5
    xp[sample] = np.nan
    Tx, _, _ = _run(xp, n_fft, hop, pad, squeezing)
    hit = sm.frames_covering(sample, Tx.shape[1], n_fft, hop)
    assert 2 <= hit.sum() <= n_fft // hop + 1
    assert np.array_equal(Tx[:, ~hit], clean[:, ~hit])
    if squeezing == "sum":
        assert np.isnan(Tx[0, hit].real).all()
    else:
        # every bin of such a frame is NaN; the reference keeps a NaN bin (only |Sx| < gamma and infinite w are
        # skipped, ssq_stft.rs:23, :278) and its scan leaves k = 0: n_freqs times 1/n_freqs * dw in row 0, nothing else
        dw = f[1] - f[0]
        col = Tx[:, hit].astype(np.complex128)
        assert not col[1:].any()
        assert (np.abs(col[0] - dw) <= sm.bound(f.shape[0], dtype) * dw).all(), col[0]
