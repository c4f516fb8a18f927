"""CPU tests of the ConceFT model tests/helpers/conceft_ref.py and of the host-side pieces of `upstream.conceft_cwt`
(`gmw_adm_ssq`, `conceft_vectors`): the closed-form admittances against quadrature, the gauge, the model's invariance
under the vectors' phases, the degenerate draw, the ties of the model on the inputs the GPU tests use, and the
concentration facts of DESIGN 4.18 (no GPU)."""
import functools

import numpy as np
import pytest

from ssqueeze_rs_amd import upstream as up
from tests.helpers import conceft_ref as cr
from tests.helpers import cwt_sst2_ref as m2
from tests.helpers import ssqueeze_ref as sq
from tests import test_gpu_conceft as gt

EPS = float(np.finfo(np.float64).eps)
GMW = ("gmw", {"gamma": 3.0, "beta": 60.0})
ADM_3_60 = [0.375226141043, 0.0196942648671, 0.262817748396, 0.0236630080736, 0.22556439662]


@pytest.mark.parametrize("k", range(5))
def test_admittance_closed_form_against_quadrature(k):
    a, q = cr.adm(3.0, 60.0, k), cr.adm_quadrature(3.0, 60.0, k)
    assert abs(a - q) <= 1e-9 * abs(a)
    assert abs(a - ADM_3_60[k]) <= 2e-12 * abs(a) + 5e-13
    assert abs(up.gmw_adm_ssq(3.0, 60.0, k) - a) <= 1e-12 * abs(a)
    a2, q2 = cr.adm(2.0, 7.5, k), cr.adm_quadrature(2.0, 7.5, k)                  # another member of the family
    assert abs(a2 - q2) <= 1e-9 * abs(a2) and abs(up.gmw_adm_ssq(2.0, 7.5, k) - a2) <= 1e-12 * abs(a2)


def test_order_zero_admittance_is_adm_ssq():
    for g, b in ((3.0, 60.0), (3.0, 20.0)):
        want = up.adm_ssq(("gmw", {"gamma": g, "beta": b}))
        assert abs(up.gmw_adm_ssq(g, b, 0) - want) <= 1e-10 * want


def test_vectors_are_unit_gauged_and_reproducible():
    adm = np.array([up.gmw_adm_ssq(3.0, 60.0, k) for k in range(4)])
    r = up.conceft_vectors(20, 4, 5, adm)
    assert r.shape == (20, 4) and r.dtype == np.complex128
    assert np.abs(np.linalg.norm(r, axis=1) - 1).max() <= 4 * EPS
    c = r @ adm
    assert (c.real > 0).all() and np.abs(c.imag).max() <= 4 * EPS * np.abs(adm).sum()
    assert np.array_equal(r, up.conceft_vectors(20, 4, 5, adm))
    assert not np.array_equal(r, up.conceft_vectors(20, 4, 6, adm))
    assert np.abs(r - cr.vectors(20, 4, 5, adm)).max() <= 8 * EPS                  # the model's own generator
    # the draws themselves are the issue's: default_rng(seed) normals, normalised
    rng = np.random.default_rng(5)
    raw = rng.standard_normal((20, 4)) + 1j * rng.standard_normal((20, 4))
    raw /= np.linalg.norm(raw, axis=1, keepdims=True)
    assert np.abs(np.abs(r) - np.abs(raw)).max() <= 8 * EPS


@functools.lru_cache(maxsize=None)
def _small():
    """A small noisy case: (W, dW, adm, f_asc, row_const)."""
    N = 256
    x = gt.two_chirps(N, 2) + 0.3 * np.random.default_rng(9).standard_normal(N)
    sc = gt.S0 * 2.0 ** (np.arange(30) / 6)
    wcode, p0, p1 = up._wavelet(GMW)
    s, rc, f, kind, f_idx = up._cwt_freq_grid(sc, None, None, "peak", N, wcode, p0, p1, 1.0)
    W, dW = cr.planes(x, s, 3.0, 60.0, (0, 1, 2))
    return W, dW, np.array([cr.adm(3.0, 60.0, k) for k in range(3)]), f, rc


def test_model_is_invariant_under_the_vectors_phases():
    W, dW, adm, f, rc = _small()
    r = cr.vectors(6, 3, 1, adm)
    ph = np.exp(2j * np.pi * np.random.default_rng(3).random(6))
    out = []
    for v in (r, r * ph[:, None]):
        v, c = cr.gauge(v, adm)
        out.append(cr.squeeze_planes(W, dW, v, c, adm[0], f, rc, True, True, 10 * EPS))
    err = np.abs(out[0] - out[1]).max() / np.abs(out[0]).max()
    print("phase invariance: %.3g of the maximum" % err)
    assert err <= 1e-13


def test_unit_vector_is_ssqueeze_of_order_zero():
    W, dW, adm, f, rc = _small()
    e0 = np.array([[1.0, 0, 0]])
    r, c = cr.gauge(e0, adm)
    assert np.array_equal(r, e0) and c[0] == adm[0]
    Tx = cr.squeeze_planes(W, dW, r, c, adm[0], f, rc, True, True, 10 * EPS)
    assert np.array_equal(Tx, sq.ssqueeze_fast(W[0], dW[0], f, rc, True, True, 10 * EPS))


def test_degenerate_draws_are_refused():
    adm = np.array([cr.adm(3.0, 60.0, k) for k in range(2)])
    bad = np.array([[adm[1], -adm[0]]])                                            # c = 0
    with pytest.raises(ValueError):
        cr.gauge(bad, adm)
    with pytest.raises(ValueError):
        cr.gauge(np.zeros((1, 2)), adm)


@pytest.mark.parametrize("i", range(len(gt.CASES)), ids=gt.IDS)
def test_model_ties_on_the_gpu_cases_are_rare(i):
    """The model alone, on its own planes of the inputs tests/test_gpu_conceft.py uses: strong coefficients with a
    fractional bin within 1e-9 of a half are at most 1e-3 of the strong ones (the project's cap)."""
    N, scf, J, M, pad, kw = gt.CASES[i]
    s, rc, f, kind, f_idx = gt.grids(i)
    W, dW = cr.planes(gt.two_chirps(N, i), s, 3.0, 60.0, range(J), fs=gt.FS, padtype=pad)
    r, c = gt.case_vectors(i)
    ntie = nstrong = 0
    for m in range(M):
        Wm, dWm = cr.combine(W, r[m]), cr.combine(dW, r[m])
        w = cr.phase(Wm, dWm, 10 * EPS)
        strong = (np.abs(Wm) >= 1e-2 * np.abs(Wm).max()) & np.isfinite(w)
        with np.errstate(all="ignore"):
            _, v = m2.bin_positions(w, f, kind, f_idx)
        ntie += int((strong & (np.abs(v - np.floor(v) - 0.5) < 1e-9)).sum())
        nstrong += int(strong.sum())
    print("ties %d of %d strong" % (ntie, nstrong))
    assert ntie <= 1e-3 * nstrong


@functools.lru_cache(maxsize=None)
def _noisy_planes(nseed):
    x, f1, f2 = cr.noisy_pair(gt.NC, nseed)
    wcode, p0, p1 = up._wavelet(GMW)
    s, rc, f, kind, f_idx = up._cwt_freq_grid(gt.SCALES_C, None, None, "peak", gt.NC, wcode, p0, p1, 1.0)
    assert kind == "log"
    W, dW = cr.planes(x, s, 3.0, 60.0, (0, 1, 2))
    return W, dW, f, rc, f1, f2


@pytest.mark.parametrize("nseed", range(4))
def test_concentration_of_the_model(nseed):
    """Unit white noise on the two components (N = 2048, 96 log scales at nv 16, J = 3, M = 16): ConceFT's share of
    |Tx|^2 within +-2 rows of the true ridges exceeds the single-wavelet transform's by at least 0.02 for both vector
    seeds.  The fp64 model gives 0.717 .. 0.730 for ssq_cwt and 0.756 .. 0.780 for ConceFT; the gaps 0.039 .. 0.060."""
    W, dW, f, rc, f1, f2 = _noisy_planes(nseed)
    adm = np.array([cr.adm(3.0, 60.0, k) for k in range(3)])
    r0, c0 = cr.gauge(np.array([[1.0, 0, 0]]), adm)
    s0 = cr.ridge_share(cr.squeeze_planes(W, dW, r0, c0, adm[0], f, rc, True, True, 10 * EPS), f1, f2, f)
    assert 0.70 <= s0 <= 0.75
    for vseed in (3, 11):
        r, c = cr.gauge(cr.vectors(16, 3, vseed, adm), adm)
        sc = cr.ridge_share(cr.squeeze_planes(W, dW, r, c, adm[0], f, rc, True, True, 10 * EPS), f1, f2, f)
        print("noise %d vectors %d: ssq_cwt %.4f ConceFT %.4f" % (nseed, vseed, s0, sc))
        assert sc >= s0 + 0.02
        assert 0.039 - 5e-4 <= sc - s0 <= 0.060 + 5e-4
