"""GPU parity of the higher-order GMW transforms of the upstream-parity mode (`upstream.cwt(order=<set>, average=)`,
`upstream.ssq_cwt(order=)`, `upstream.cwt_higher_order`; `cwt` rejects a bare int order) against the NumPy restatement tests/helpers/gmw_order_ref.py,
which runs upstream's way: one transform per order, then the mean of the outputs; dWx of ssq_cwt by `trigdiff`.
The library runs an averaged order set as ONE transform with the averaged wavelet table, and `average=False` as one
plan with a row group per order.  Tolerances as tests/test_gpu_upstream.py: fp64 1e-11 of each output's maximum, fp32
5e-6; Tx re-accumulated from the kernel's own w, bins index-exact except at half-bin ties."""
import numpy as np
import pytest

from oracle import upstream_oracle as u
from ssqueeze_rs_amd import upstream as up
from tests.helpers import gmw_order_ref as g

pytestmark = pytest.mark.gpu

PAIRS = [(3.0, 60.0), (3.0, 20.0)]


def echirp(N):                                   # reconstruction_test.py:33-35
    t = np.linspace(0, 10, N, endpoint=False)
    return np.cos(2 * np.pi * 3 * np.exp(t / 3)), t


def _scales(gamma, beta, nv=8, octaves=9):
    j0 = int(np.ceil(np.log2(u.morsefreq(gamma, beta) / np.pi) * nv))
    return 2 ** (np.arange(j0, j0 + octaves * nv) / nv)


def _close(a, b, tol):
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= tol * np.abs(b).max()


def _as_list(a):
    return a if isinstance(a, list) else [a]


def _order_cwt(x, wavelet, order, average=None, **kw):
    """an order set through `cwt`, a single int order through `cwt_higher_order` (`cwt` rejects a bare int order)"""
    if isinstance(order, int):
        return up.cwt_higher_order(x, wavelet, order=order, average=average, **kw)
    return up.cwt(x, wavelet, order=order, average=average, **kw)


@pytest.mark.parametrize("gb", PAIRS)
@pytest.mark.parametrize("order,average", [(1, None), (2, None), ((0, 1, 2), None), (range(3), None), ((0, 1, 2), True),
                                           ((0, 1, 2), False), (range(3), False)])
def test_cwt_orders_match_the_per_order_restatement(gb, order, average):
    gamma, beta = gb
    wav = ("gmw", {"gamma": gamma, "beta": beta})
    sc = _scales(gamma, beta)
    for N in (1000, 1001):
        x, ts = echirp(N)
        fs = 1 / (ts[1] - ts[0])
        Wx, s, dWx = _order_cwt(x, wav, order, average, scales=sc, fs=fs, derivative=True)
        Wo, dWo = g.cwt_higher_order(x, sc, gamma, beta, order, average, fs=fs, derivative=True)
        assert isinstance(Wx, list) == isinstance(Wo, list) and isinstance(dWx, list) == isinstance(dWo, list)
        assert len(_as_list(Wx)) == len(_as_list(Wo))
        for a, b in zip(_as_list(Wx), _as_list(Wo)):
            assert a.dtype == np.complex128 and a.shape == (len(sc), N)
            _close(a, b, 1e-11)
        for a, b in zip(_as_list(dWx), _as_list(dWo)):
            _close(a, b, 1e-11)
        assert np.array_equal(s, sc)


def test_cwt_order_structure():
    gamma, beta = PAIRS[0]
    sc = _scales(gamma, beta)
    x, ts = echirp(1000)
    lst, _ = up.cwt(x, "gmw", scales=sc, order=(0, 1, 2), average=False)
    assert isinstance(lst, list) and len(lst) == 3 and all(a.shape == (len(sc), 1000) for a in lst)
    avg, _ = up.cwt(x, "gmw", scales=sc, order=(0, 1, 2))
    _close(avg, np.mean(lst, axis=0), 1e-13)
    # a single order in a tuple with average=False is the array itself; order (0,) is the order-0 transform bit for bit
    W0, _ = up.cwt(x, "gmw", scales=sc)
    Wt, _ = up.cwt(x, "gmw", scales=sc, order=(0,), average=False)
    assert not isinstance(Wt, list) and np.array_equal(Wt, W0)
    with pytest.warns(UserWarning):
        W2, _ = up.cwt(x, "gmw", scales=sc, order=(2,), average=True)
    assert np.array_equal(W2, up.cwt_higher_order(x, "gmw", order=2, scales=sc)[0])
    assert np.array_equal(up.cwt(x, "gmw", scales=sc, order=(1,))[0], up.cwt_higher_order(x, "gmw", order=1, scales=sc)[0])
    # each group of the one-plan average=False run equals that order alone
    for k in range(3):
        Wk = up.cwt_higher_order(x, "gmw", order=k, scales=sc)[0]
        assert np.abs(lst[k] - Wk).max() <= 1e-14 * np.abs(lst[k]).max()
    # cwt_higher_order is cwt with `order`; rpadded keeps the padded columns
    Wh, sh, dWh = up.cwt_higher_order(x, "gmw", order=(1, 2), scales=sc, derivative=True, rpadded=True)
    Wo, dWo = g.cwt_higher_order(x, sc, gamma, beta, (1, 2), derivative=True, rpadded=True)
    assert Wh.shape == (len(sc), 2048)
    _close(Wh, Wo, 1e-11)
    _close(dWh, dWo, 1e-11)
    Wz, _ = up.cwt_higher_order(x, "gmw", order=3, scales=sc, padtype="zero")
    _close(Wz, g.cwt_higher_order(x, sc, gamma, beta, 3, padtype="zero"), 1e-11)


@pytest.mark.parametrize("order", [2, range(3)])
@pytest.mark.parametrize("kw", [dict(), dict(flipud=False, squeezing="lebesgue"), dict(flipud=True, squeezing="lebesgue"),
                                dict(flipud=False)])
def test_ssq_cwt_orders_match_the_restatement(order, kw):
    gamma, beta = PAIRS[0]
    x, ts = echirp(1024)
    fs = 1 / (ts[1] - ts[0])
    sc = _scales(gamma, beta, nv=16)
    Tx, Wx, f, s, w, dWx = up.ssq_cwt(x, "gmw", scales=sc, fs=fs, order=order, get_w=True, get_dWx=True, **kw)
    To, Wo, fo, so, im = g.ssq_cwt_order(x, sc, gamma, beta, order, fs=fs, **kw)
    assert Tx.shape == To.shape and np.allclose(f, fo, rtol=1e-14, atol=0)
    assert np.array_equal(f, up.ssq_cwt(x, "gmw", scales=sc, fs=fs, **kw)[2])          # the order-0 ssq_freqs
    wmax = np.abs(Wo).max()
    assert np.abs(Wx - Wo).max() <= 1e-11 * wmax and np.abs(dWx - im["dWx"]).max() <= 1e-11 * np.abs(im["dWx"]).max()
    keep_g, keep_o = np.isfinite(w), im["k"] >= 0
    assert np.abs(Wo[keep_g != keep_o]).max(initial=0.0) <= 1e-6 * wmax + 1e-12
    na = len(sc)
    fa = im["freqs_ascending"]
    with np.errstate(all="ignore"):
        v = (np.log2(w) - np.log2(fa[0])) / (np.log2(fa[1]) - np.log2(fa[0]))
        k_own = np.minimum(np.rint(np.maximum(np.where(keep_g, v, 0.0), 0)), na - 1).astype(np.int64)
    if kw.get("flipud", True):
        k_own = na - 1 - k_own
    Wv = (np.ones(Wo.shape) / na) if kw.get("squeezing") == "lebesgue" else Wo
    Tre = np.zeros_like(To)
    cols = np.arange(Tx.shape[1])
    for i in range(na):
        m = keep_g[i]
        np.add.at(Tre, (k_own[i, m], cols[m]), Wv[i, m] * im["const"])
    assert np.abs(Tx - Tre).max() <= 1e-10 * max(np.abs(Tre).max(), 1e-300)
    both = keep_o & keep_g & (np.abs(Wo) > 1e-6 * wmax)
    mism = both & (k_own != im["k"])
    if mism.any():
        vv = v[mism]
        assert (np.abs(np.abs(vv - np.floor(vv)) - 0.5) < 1e-6).all()
    assert mism.mean() <= 1e-3


def test_float32_orders_and_batches():
    rng = np.random.default_rng(3)
    xb = rng.standard_normal((3, 400)).astype(np.float32)
    sc = _scales(3.0, 60.0, nv=8, octaves=6)
    Wx, s = up.cwt(xb, "gmw", scales=sc, order=(0, 1, 2))
    assert Wx.shape == (3, len(sc), 400) and Wx.dtype == np.complex64 and s.dtype == np.float32
    lst, _, dl = up.cwt(xb, "gmw", scales=sc, order=range(3), average=False, derivative=True)
    assert len(lst) == 3 and all(a.shape == (3, len(sc), 400) and a.dtype == np.complex64 for a in lst + dl)
    W1, _ = up.cwt_higher_order(xb[1], "gmw", order=2, scales=sc)
    assert W1.shape == (len(sc), 400) and W1.dtype == np.complex64
    for b in range(3):
        xd = xb[b].astype(np.float64)
        Wo = g.cwt_higher_order(xd, sc, 3.0, 60.0, (0, 1, 2))
        assert np.abs(Wx[b] - Wo).max() <= 5e-6 * np.abs(Wo).max()
        for k in range(3):
            Wk, dWk = g.cwt_higher_order(xd, sc, 3.0, 60.0, k, derivative=True)
            assert np.abs(lst[k][b] - Wk).max() <= 5e-6 * np.abs(Wk).max()
            assert np.abs(dl[k][b] - dWk).max() <= 5e-6 * np.abs(dWk).max()
    assert np.abs(W1 - g.cwt_higher_order(xb[1].astype(np.float64), sc, 3.0, 60.0, 2)).max() <= 5e-6 * np.abs(W1).max()
    Tc, Wc, fc, sc2 = up.ssq_cwt(xb, "gmw", scales=sc, order=range(3))
    assert Tc.shape == (3, len(sc), 400) and Tc.dtype == np.complex64 and Wc.dtype == np.complex64
    assert fc.dtype == np.float32 and sc2.dtype == np.float32
    To, Wo, *_ = g.ssq_cwt_order(xb[1].astype(np.float64), sc, 3.0, 60.0, range(3))
    assert np.abs(Wc[1] - Wo).max() <= 5e-6 * np.abs(Wo).max()


def test_order_options_outside_the_subset_raise_value_error():
    x = np.zeros(256)
    sc = _scales(3.0, 60.0, nv=8, octaves=3)
    for kw in (dict(wavelet="morlet", order=1), dict(wavelet=("morlet", {"mu": 13.4}), order=(0, 1)),
               dict(wavelet="gmw", order=1, l1_norm=False), dict(wavelet="gmw", order=-1),
               dict(wavelet="gmw", order=(0, -1)), dict(wavelet=("gmw", {"order": 1})),
               dict(wavelet="gmw", order=up.GMW_MAX_ORDER + 1), dict(wavelet="gmw", order=1)):
        with pytest.raises(ValueError):
            up.cwt(x, scales=sc, **kw)
    with pytest.raises(ValueError):
        up.cwt_higher_order(x, "morlet", order=0, scales=sc)
    for kw in (dict(wavelet="morlet", order=2), dict(wavelet="gmw", order=-2), dict(wavelet=("gmw", {"order": 2}))):
        with pytest.raises(ValueError):
            up.ssq_cwt(x, scales=sc, **kw)
