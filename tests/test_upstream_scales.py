"""Upstream's scale utilities (`ssqueeze_rs_amd.upstream_scales`, re-exported by `upstream`) against the NumPy
restatement tests/helpers/scales_ref.py, and the facts upstream's own tests state (old/tests/misc_test.py:12-19).
CPU only: the wavelet is evaluated by the library's host entry point ssq_upstream_psih."""
import numpy as np
import pytest

from ssqueeze_rs_amd import upstream as up
from ssqueeze_rs_amd.upstream_scales import _psih_fn
from tests.helpers import scales_ref as ref

WAVELETS = ["gmw", ("gmw", {"beta": 8}), ("morlet", {"mu": 6}), ("morlet", {"mu": 13.4})]
SIZES = [2 ** p for p in range(6, 13)] + [2 ** 16, 2 ** 20]
SPECS = ["log", "log-piecewise", "linear", "log:maximal", "log:minimal", "log:naive", "linear:maximal",
         "log-piecewise:minimal"]


def _ids(w):
    return w if isinstance(w, str) else "%s-%s" % (w[0], "-".join("%s%s" % kv for kv in w[1].items()))


def test_psih_is_the_oracle_wavelet():
    w = np.linspace(-3, 40, 4001)
    for wav in WAVELETS:
        fn = ref._fn(wav)
        got = _psih_fn(wav)(w)
        want = fn(w)
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), wav


@pytest.mark.parametrize("wavelet", WAVELETS, ids=_ids)
@pytest.mark.parametrize("spec", SPECS)
def test_process_scales_matches_restatement(wavelet, spec):
    for N in SIZES:
        try:
            want = ref.process_scales(spec, N, wavelet)
        except Exception as e:                             # upstream raises here too: so must the mirror
            with pytest.raises(type(e)):
                up.process_scales(spec, N, wavelet)
            continue
        got, kind, na, nv = up.process_scales(spec, N, wavelet, get_params=True)
        assert got.shape == want.shape and got.dtype == np.float64, (N, spec)
        np.testing.assert_allclose(got, want, rtol=1e-13, err_msg=f"N={N} {spec}")
        assert kind == spec.split(":")[0] and na == len(want) and nv == 32


@pytest.mark.parametrize("wavelet", WAVELETS, ids=_ids)
def test_scalebounds_and_make_scales_match_restatement(wavelet):
    for N in (128, 2048, 2 ** 16):
        for preset in ("maximal", "minimal", "naive", None):
            try:
                want = ref.scalebounds(wavelet, N, preset)
            except Exception as e:
                with pytest.raises(type(e)):
                    up.cwt_scalebounds(wavelet, N, preset=preset)
                continue
            got = up.cwt_scalebounds(wavelet, N, preset=preset)
            np.testing.assert_allclose(got, want, rtol=1e-13)
        mn, mx = ref.scalebounds(wavelet, N, "maximal")
        for kind in ("log", "log-piecewise", "linear"):
            for nv in (16, 32):
                np.testing.assert_allclose(up.make_scales(N, mn, mx, nv=nv, scaletype=kind, wavelet=wavelet),
                                           ref.make_scales(N, mn, mx, nv, kind, wavelet), rtol=1e-13)
        np.testing.assert_allclose(up.make_scales(N, mn, mx, nv=32, scaletype="log-piecewise", wavelet=wavelet,
                                                  downsample=2),
                                   ref.make_scales(N, mn, mx, 32, "log-piecewise", wavelet, downsample=2), rtol=1e-13)


@pytest.mark.parametrize("wavelet", WAVELETS, ids=_ids)
def test_generated_grids_are_classified(wavelet):
    for N in (2048, 2 ** 16):
        for spec in ("log", "log-piecewise", "linear", "log:naive"):
            s = up.process_scales(spec, N, wavelet)
            kind = spec.split(":")[0]
            if kind == "log-piecewise" and ref.transition_idx(s) is None:
                kind = "log"                               # no downsampling scale found: one segment
            got, nv = up.infer_scaletype(s)
            assert got == kind == ref.scaletype(s), (N, spec)
            if N == 2048:                                  # (long float32 linear grids fail upstream's threshold)
                assert up.infer_scaletype(s.astype(np.float32))[0] == kind
            if kind == "log":
                assert nv == 32 and up.logscale_transition_idx(s) is None
            elif kind == "linear":
                assert nv is None
            else:
                idx = up.logscale_transition_idx(s)
                assert idx == ref.transition_idx(s) and 0 < idx < len(s)
                assert nv.shape == (len(s), 1)
                np.testing.assert_allclose(nv[:idx], 32, rtol=1e-9)      # first segment: 32 voices
                np.testing.assert_allclose(nv[idx:], 8, rtol=1e-9)       # downsampled by 4
                np.testing.assert_allclose(up.nv_from_scales(s), nv)


def test_classification_rejects_other_arrays():
    s = 2 ** (np.arange(40) / 8)
    two = np.hstack([s[:10], s[11:25:2], s[26::4]])        # two transitions
    assert ref.transition_idx(two) is None and up.logscale_transition_idx(two) is None
    for bad in (two, np.array([1.0, 3.0, 4.0, 9.0, 10.0])):
        with pytest.raises(ValueError):
            up.infer_scaletype(bad)
        with pytest.raises(ValueError):
            up.process_scales(bad, 64)
    with pytest.raises(TypeError):
        up.infer_scaletype(np.arange(1, 9))
    # upstream classifies [1, 2, 5] as 'log-piecewise' (one scale after the jump) and fails later (_exp_fm of one point);
    # the mirror's transforms refuse it up front
    assert up.infer_scaletype(np.array([1.0, 2.0, 5.0]))[0] == "log-piecewise"
    with pytest.raises(ValueError):
        up._scales(np.array([1.0, 2.0, 5.0]))
    with pytest.raises(Exception, match="differs"):
        up.process_scales(s, 64, nv=16)
    assert up.process_scales(s, 64, get_params=True)[1:] == ("log", 40, 8)
    assert up.process_scales(np.linspace(1, 9, 17), 64, get_params=True)[1:] == ("linear", 17, None)


def test_bounds():
    """old/tests/misc_test.py:12-19: cwt_scalebounds on Morlet mu=6 succeeds for N = 4096 down to 64."""
    for N in (4096, 2048, 1024, 512, 256, 128, 64):
        mn, mx = up.cwt_scalebounds(("morlet", {"mu": 6}), N=N)
        assert 0 < mn < mx


def test_find_helpers_match_restatement():
    for wav in WAVELETS:
        fn = ref._fn(wav)
        wp, peak = up.find_maximum(fn)
        assert (wp, peak) == ref.find_maximum(fn)
        assert up.find_first_occurrence(fn, .5 * peak, step_start=0, step_limit=wp)[0] == \
            ref.find_first_occurrence(fn, .5 * peak, 0, wp)
        assert up.find_min_scale(wav, cutoff=-.5) == pytest.approx(ref.min_scale(wav), rel=1e-13)
        s = 2 ** (np.arange(0, 320) / 32)
        assert up.find_downsampling_scale(wav, s) == ref.downsampling_idx(wav, s)


def test_mirror_accepts_every_upstream_grid_kind():
    """`upstream._scales` classifies arrays as upstream does; today's exponential arrays keep their nv."""
    s = 2 ** (np.arange(1, 60) / 12)
    assert up._scales(s)[1:3] == ("log", 12)
    lp = up.process_scales("log-piecewise", 4096, "gmw")
    got = up._scales(lp)
    assert got[1] == "log-piecewise" and got[2].shape == (len(lp), 1)
    assert up._scales(np.linspace(1, 40, 100))[1:3] == ("linear", None)
    with pytest.raises(ValueError):
        up._scales(np.array([1.0, 2.0, 5.0]))


@pytest.mark.parametrize("N", [1024, 2048, 2 ** 16])
def test_float32_piecewise_grids_are_accepted(N):
    """A float32 copy of a log-piecewise grid (what `ssq_cwt` returns for float32 input) is 'log-piecewise' with the
    same transition, found with float32's thresholds as upstream finds it; the float64 test would not see it."""
    s = up.process_scales("log-piecewise", N, "gmw").reshape(-1)
    s32 = s.astype(np.float32)
    idx = up.logscale_transition_idx(s)
    assert idx is not None and up.logscale_transition_idx(s32) == idx
    s64, kind, nv, own = up._scales(s32)
    assert kind == "log-piecewise" and own.dtype == np.float32 and s64.dtype == np.float64
    assert nv.shape == (len(s), 1) and np.allclose(nv[idx:], 8, rtol=1e-4)
    assert up.logscale_transition_idx(own) == idx
