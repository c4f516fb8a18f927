"""CPU tests of the fixed-point scatter scheme, independent of the kernels: the NumPy model of
tests/helpers/scatter_model.py, fed the float64 oracle's Sx and k for every input of tests/test_gpu_stft_scatter.py,
meets the per-column bound those GPU tests hold the kernels to, and the power-of-two equivariance cases listed there
satisfy their preconditions.  So inputs and bounds are satisfiable whatever the kernels do."""
import numpy as np
import pytest

from oracle import ssq_oracle as o
from tests.helpers import scatter_model as sm


def _oracle(x, n_fft, hop, pad, squeezing="sum"):
    win = np.hanning(n_fft)
    _, _, im = o.ssq_stft(np.asarray(x, dtype=np.float64), win, n_fft=n_fft, hop_len=hop, fs=1.0, padtype=pad,
                          squeezing=squeezing, return_intermediates=True)
    return im


@pytest.mark.parametrize("cfg", sm.CONFIGS, ids=sm.config_id)
@pytest.mark.parametrize("pad", sm.PADS)
@pytest.mark.parametrize("name", sm.INPUTS)
def test_model_meets_the_per_column_bound(cfg, pad, name):
    dtype, n_fft, hop, F = cfg
    x = sm.make_input(name, n_fft, hop, F, dtype)
    im = _oracle(x, n_fft, hop, pad)
    cd = np.complex64 if dtype == np.float32 else np.complex128
    Sx = im["Sx"].astype(cd)                                  # the weights as the kernel holds them
    keep = ~np.isinf(im["w"])
    dw = float(dtype(im["dw"]))
    n_freqs = Sx.shape[0]
    for leb in (True, False):
        Tx, e = sm.scatter_model(Sx, im["k"], keep, dw, n_freqs, dtype, lebesgue=leb)
        assert np.isfinite(Tx.view(dtype)).all()
        worst, r = sm.worst_ratio(Tx, Sx, im["k"], keep, dw, dtype, lebesgue=leb)
        assert worst <= 1.0, (name, pad, leb, worst, int(np.argmax(r)))
    # (Tx, e: sum mode from here on)
    if name == "bursts":
        silent = sm.silent_columns(x, n_fft, hop, pad)
        assert silent.sum() >= F                              # a whole tile of silence
        assert not keep[:, silent].any() and not Tx[:, silent].any()
    if name == "geometric_tone":
        # quiet next to loud, and every exponent of the column scale across 40 octaves
        assert e.max() - e.min() >= 38
        c = sm.weights(Sx, keep, False)
        a = np.abs(c.real) + np.abs(c.imag)
        inner = slice(8, -8)
        on_ridge = np.where(im["k"] == n_freqs // 4, a, 0).sum(0)
        assert (on_ridge[inner] >= 0.9 * a.sum(0)[inner]).all()      # the column's mass lands in one cell


def test_model_handles_the_clamps_and_nan():
    """EMIN clamp (a column far below 2^EMIN), an empty column, and a NaN column."""
    rng = np.random.default_rng(5)
    for dtype, tiny in ((np.float32, 2.0 ** -100), (np.float64, 2.0 ** -1000)):
        Sx = (rng.standard_normal((33, 6)) + 1j * rng.standard_normal((33, 6)))
        Sx[:, 1] *= tiny
        Sx[:, 2] = 0
        Sx[5, 3] = np.nan
        k = rng.integers(0, 33, size=Sx.shape)
        keep = np.ones(Sx.shape, dtype=bool)
        keep[:, 2] = False
        Tx, e = sm.scatter_model(Sx, k, keep, 2.0 ** -5, 33, dtype)
        emin = sm.EMIN[np.dtype(dtype).itemsize]
        assert e[1] == emin and e[2] == (emin if dtype == np.float32 else 0)     # frexp(0) = 0 in the fp64 branch
        assert not Tx[:, 2].any() and np.isnan(Tx[:, 3]).all()
        ok = [0, 4, 5]
        worst, _ = sm.worst_ratio(Tx[:, ok], Sx[:, ok], k[:, ok], keep[:, ok], 2.0 ** -5, dtype)
        assert worst <= 1.0


@pytest.mark.parametrize("cfg", sm.CONFIGS, ids=sm.config_id)
def test_equivariance_cases_satisfy_their_preconditions(cfg):
    """Every listed m of 3(c) runs (none is skipped) for the seed the GPU test uses; m = -70 puts every bin below
    the default gamma."""
    dtype, n_fft, hop, F = cfg
    x = sm.equivariance_signal(cfg)
    tpe = sm.two_pi_eff(np.hanning(n_fft))
    for pad in sm.PADS:
        im = _oracle(x, n_fft, hop, pad)
        for m in sm.M_LIST[dtype]:
            assert sm.equivariance_preconditions(im["Sx"], m, o.DEFAULT_GAMMA, tpe, dtype) == [], (pad, m)
        assert (np.abs(im["Sx"]) * 2.0 ** -70 < o.DEFAULT_GAMMA / 64).all()
