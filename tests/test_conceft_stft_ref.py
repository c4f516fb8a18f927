"""The facts of the numpy model of ConceFT on the STFT (tests/helpers/conceft_stft_ref.py) that the
definition of `upstream.conceft_stft` rests on, and `upstream.hermite_windows`.  No GPU, no library."""
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import upstream as up
from tests.helpers import conceft_ref as cr
from tests.helpers import conceft_stft_ref as cs
from tests.helpers import sst2_ref as s2

N, NFFT, SIGMA, J, M = 2048, 256, 16.0, 3, 16
EPS = float(np.finfo(np.float64).eps)


@functools.lru_cache(maxsize=None)
def tapers():
    h = up.hermite_windows(NFFT, J, SIGMA)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def planes(nseed):
    x, f1, f2 = cr.noisy_pair(N, nseed)
    V, V1 = cs.planes(x, tapers(), NFFT)
    for a in (V, V1):
        a.setflags(write=False)
    return x, f1, f2, V, V1


def squeeze(nseed, r):
    """Tx of the model for raw vectors r on the planes of noise seed `nseed` (None: no noise)."""
    x, f1, f2, V, V1 = planes(nseed)
    adm = tapers()[:, NFFT // 2]
    rg, c = cr.gauge(r, adm)
    return cs.squeeze_planes(V, V1, rg, c, adm[0], NFFT)


def e0(n):
    r = np.zeros((1, n))
    r[0, 0] = 1
    return r


@pytest.mark.parametrize("n_fft", [64, 128, 256, 512, 1024, 2048, 4096])
def test_hermite_gram(n_fft):
    """The default tapers are orthonormal once the window holds them: 8 tapers at sigma = n_fft / 16 reach |u| = 8, where
    psi_7^2 is below 1e-20.  A Gram entry is a sum of n_fft products of O(1 / sigma) values whose absolute sum is at most
    1 (Cauchy-Schwarz), each value carrying the recurrence's rounding, a few eps per step over 7 steps: 64 eps bounds it
    (the model measured 9e-16 = 4 eps)."""
    h = up.hermite_windows(n_fft, 8)
    assert h.shape == (8, n_fft) and h.dtype == np.float64
    err = np.abs(h @ h.T - np.eye(8)).max()
    print("n_fft %d: max |Gram - I| = %.3g" % (n_fft, err))
    assert err <= 64 * EPS


def test_hermite_gram_short_windows():
    """n_fft = 32 cuts psi_7 off at |u| = 8 with sigma = 2, where samples are so sparse (one per 0.5) that the Riemann
    sum of the products is no longer exact: the model measured 2.8e-8; the bound 1e-6 is what aliasing of a product of
    bandwidth 2 sqrt(2 * 7 + 1) = 7.7 rad sampled at 2 pi / 0.5 = 12.6 rad allows (exp(-(12.6 - 7.7)^2 / 2) = 6e-6 times
    the O(0.1) amplitude of the spectrum's tail).  At n_fft = 16 the tapers are not orthogonal at all (documented)."""
    h = up.hermite_windows(32, 8)
    err = np.abs(h @ h.T - np.eye(8)).max()
    print("n_fft 32: max |Gram - I| = %.3g" % err)
    assert err <= 1e-6
    h = up.hermite_windows(16, 8)
    assert np.abs(h @ h.T - np.eye(8)).max() > 1e-3


@pytest.mark.parametrize("n_fft,n_tapers,sigma", [(256, 8, None), (64, 3, 5.5), (4096, 8, 100.0), (16, 2, None)])
def test_hermite_against_the_polynomial_form(n_fft, n_tapers, sigma):
    """The recurrence against numpy's Hermite polynomials: both forms are accurate to a few eps of the taper's maximum
    per order (the polynomial form cancels more at high orders: 1e-12 of the maximum covers order 7)."""
    h = up.hermite_windows(n_fft, n_tapers, sigma)
    ref = cs.hermite(n_fft, n_tapers, sigma)
    assert np.abs(h - ref).max() <= 1e-12 * np.abs(ref).max()


def test_e0_vector_is_the_first_order_squeeze():
    """vectors = e_0 against `sst2_ref` restricted to first order (its re_w1 and keep, scattered rows ascending): the same
    V, the same bins outside ties (the two write Im(V1 / V) differently: the last place of w) and the same cells
    where no tie is near."""
    x, f1, f2, V, V1 = planes(0)
    Tx, S, w = cs.squeeze_planes(V, V1, e0(J), np.array([tapers()[0, NFFT // 2]]), tapers()[0, NFFT // 2], NFFT,
                                 details=True)
    Vr, _, _, _, d = s2.sst2_ref(x, tapers()[0], NFFT, details=True)
    assert np.array_equal(Vr, V[0]) and np.array_equal(S[0], V[0])
    F = NFFT // 2 + 1
    w1 = np.where(d["keep"], np.abs(d["re_w1"]), np.inf)
    assert np.array_equal(np.isinf(w1), np.isinf(w[0]))
    k1, v1 = cs.bin_positions(w1, F, 1.0)
    k0, _ = cs.bin_positions(w[0], F, 1.0)
    tie = np.abs(v1 - np.floor(v1) - 0.5) < 1e-9
    keep = d["keep"]
    assert not ((k1 != k0) & keep & ~tie).any()
    ref = np.zeros_like(Tx)
    cols = np.arange(Tx.shape[1])
    for i in range(F):
        q = keep[i]
        np.add.at(ref, (k1[i, q], cols[q]), V[0][i, q] * d["dw"])
    clean = ~(tie & keep).any(axis=0)
    assert clean.sum() >= 0.99 * len(clean)
    assert np.array_equal(Tx[:, clean], ref[:, clean])


def test_inversion():
    """2 / h_0[c] sum_k Re Tx recovers the noise-free signal on the columns N/8 .. 7N/8: the model measured a relative L2
    error of 6.2e-10 for ConceFT and 3.3e-11 for the first-order squeeze with taper 0 (the tapers' tails beyond the
    window: psi_2 at |u| = 8 is 1e-12 of its peak, its spectral derivative's wrap-around the rest); 1e-8 holds both with
    room and a wrong gauge, scale or admittance misses it by orders of magnitude (a 1 % error in the scale is 1e-2)."""
    x, _, _, _, _ = planes(None)
    cols = slice(N // 8, 7 * N // 8)
    rel = lambda T: float(np.linalg.norm((2 / tapers()[0, NFFT // 2] * T.real.sum(0) - x)[cols])      # noqa: E731
                          / np.linalg.norm(x[cols]))
    ec, e1 = rel(squeeze(None, cs.draws(M, J, 3))), rel(squeeze(None, e0(J)))
    print("relative L2 error: ConceFT %.3g, first order %.3g" % (ec, e1))
    assert ec <= 1e-8 and e1 <= 1e-8


@pytest.mark.parametrize("vseed", [3, 11])
@pytest.mark.parametrize("nseed", range(4))
def test_concentration(nseed, vseed):
    """Unit white noise on the two components: the share of |Tx|^2 within +-2 rows of the two true ridges is at least
    the first-order squeeze's plus 0.02 (the model's gaps: 0.039 .. 0.052; shares 0.723 .. 0.758 against 0.684 ..
    0.713)."""
    x, f1, f2, V, V1 = planes(nseed)
    sc = cs.ridge_share(squeeze(nseed, cs.draws(M, J, vseed)), f1, f2)
    s0 = cs.ridge_share(squeeze(nseed, e0(J)), f1, f2)
    print("ridge share: ConceFT %.4f, first order %.4f" % (sc, s0))
    assert sc >= s0 + 0.02
