"""The record of `ssqueeze_rs_amd.upstream`'s Python (CPU only): what every public callable hands to the library's
`*_host*` entry points, what it makes of their results, and what it refuses, case by case against
tests/golden/upstream_frontend.json.

The fixture holds one outcome line per case (`outcome`): a refusal's exception type and full message in words (refusals
with the same outcome share a line); for a case that makes a call, the entry's name, the digest of the arguments
recorded for it and the digest of what the callable returned, described below.  The whole records would be seven times
the size.  It was recorded by tests/golden/make_upstream_frontend.py at the commit it names (`commit`), before the
mirror's front ends were shared, and is not regenerated for a refactor: every case's record must equal it exactly.

The harness.  `require_gpu` is patched (a no-op for the accepted cases, a sentinel for the refusals), `up._ptr` is the
identity, and `up._lib.load` returns a proxy over the real library.  The proxy forwards everything (`ssq_upstream_p2up`,
`ssq_upstream_center_frequency`, `ssq_upstream_adm`, the `*_workspace_bytes` checks, `ssq_last_error` run for real on
the host) but the `*_host*` entry points: for those it records the entry's name and every argument -- a scalar as
`<type>:<repr>`, an array as `<dtype>[<shape>]#<sha1 of its bytes, 16 hex digits>`, None as None, an output array as
`<dtype>[<shape>]#out` (np.empty's bytes mean nothing) -- fills every OUTPUT array with a deterministic pattern, and
returns 0.  The outputs are the pointer parameters include/ssq_hip.h does not declare `const`; inputs are never written
(several are views of the caller's).  What the callable returns is recorded the same way, so the mirror's own
post-processing (`.real.copy()`, `[::-1].astype`, `_cwt`'s split, the unbatching, `icwt`'s `x_mean` column) is pinned
too, and so are the warnings.

The table.  Accepted cases: every public callable on a float64 [300] and a float32 [2, 300] signal (600 samples for the
default n_fft = 512), each option moved off its default on its own.  Refusals: one case at least for every `raise` of
upstream.py that can be reached (the generator counts them), and by name the faults on which the copied front ends had
drifted: an `nv` that differs from the scales', gamma = inf and beta = inf for the wavelet, a NaN `gamma`, a bad
`padtype` and a one-sample signal, on every callable that takes them.  An input with two faults is not in the table:
which of the two refusals wins is not pinned.

A refusal is run with the sentinel: its record is the exception's type name and full message, or that it reached
`require_gpu`; a case that reaches it is run again without the sentinel and the call it makes is recorded as well
("passes through to the recorded call" is an outcome like any other).
"""
import functools
import hashlib
import json
import os
import re
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "upstream_frontend.json")
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------------------- harness ----
class _Reached(Exception):
    pass


def _refuse():
    raise _Reached("require_gpu")


@functools.lru_cache(maxsize=None)
def host_outputs():
    """name -> (number of parameters, positions of the output parameters) of every `*_host*` entry point of the header:
    an output is a pointer parameter not declared `const`."""
    with open(_lib.HEADER_PATH) as f:
        src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S))
    out = {}
    for name, params in re.findall(r"\b(ssq_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        if re.match(r"ssq_(?!host_).*_host(_|$)", name):
            params = params.split(",")
            out[name] = (len(params), [i for i, p in enumerate(params) if "*" in p and "const" not in p])
    return out


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def rec(v):
    """The record of one argument or returned value (JSON data only)."""
    if v is None:
        return None
    if isinstance(v, np.ndarray):
        tail = "" if v.flags.c_contiguous else "!strided"
        return "%s[%s]#%s%s" % (v.dtype, ",".join(str(n) for n in v.shape), digest(v), tail)
    if isinstance(v, (tuple, list)):
        return {type(v).__name__: [rec(e) for e in v]}
    if isinstance(v, np.generic):
        return "%s:%r" % (type(v).__name__, v.item())
    return "%s:%r" % (type(v).__name__, v)


def fill(a, k):
    """The pattern an output array in parameter position k comes back with."""
    assert isinstance(a, np.ndarray) and a.flags.c_contiguous and a.flags.writeable
    flat = a.reshape(-1)
    v = (np.arange(flat.size, dtype=np.int64) * 7 + 3 * k) % 251 - 100
    flat[:] = v + 1j * ((v * 5) % 13 - 6) if a.dtype.kind == "c" else v


class _Proxy:
    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in host_outputs():
            return fn
        n_params, outputs = host_outputs()[name]

        def record(*args):
            assert len(args) == n_params == len(_lib._SIGNATURES[name][1]), name
            # an output's bytes on entry are whatever np.empty left there: its dtype and shape alone are recorded
            self._calls.append({"entry": name, "args": [
                rec(a) if k not in outputs or a is None else rec(a).split("#")[0] + "#out" for k, a in enumerate(args)]})
            for k in outputs:
                if args[k] is not None:
                    fill(args[k], k)
            return 0
        return record


def run(case, sentinel, lines=None):
    """One case -> its record.  `lines`: a list that gets the line of upstream.py a refusal was raised from."""
    fn, a, k = case
    calls = []
    real = _lib.load()
    with pytest.MonkeyPatch.context() as mp, warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        mp.setattr(up._lib, "require_gpu", _refuse if sentinel else lambda: None)
        mp.setattr(up, "_ptr", lambda arr: arr)
        mp.setattr(up._lib, "load", lambda: _Proxy(real, calls))
        try:
            out = {"returns": rec(getattr(up, fn)(*a, **k))}
        except _Reached:
            out = {"reaches": "require_gpu"}
        except Exception as e:
            out = {"raises": type(e).__name__, "message": str(e)}
            if lines is not None:
                tb, line = e.__traceback__, None
                while tb is not None:
                    if tb.tb_frame.f_code.co_filename == up.__file__:
                        line = tb.tb_lineno
                    tb = tb.tb_next
                lines.append(line)
    if calls:
        out["calls"] = calls
    if caught:
        out["warnings"] = [str(w.message) for w in caught]
    return out


def record_of(cid, lines=None):
    """The record of case `cid`, as the fixture holds it."""
    t = tables()
    if cid in t.accepted:
        out = run(t.accepted[cid], False, lines)
    else:
        out = run(t.refusals[cid], True, lines)
        if "reaches" in out:
            out["then"] = run(t.refusals[cid], False, lines)
    return json.loads(json.dumps(out))


def outcome(r):
    """What the fixture holds of a record, one line: every call as `entry(<digest of its recorded arguments>)`, then
    `-> <digest of the recorded return value>` or the exception's type and full message in words, then the warnings.
    A line that differs says which part moved; the failing test prints the record itself."""
    def h(v):
        return hashlib.sha1(json.dumps(v, sort_keys=True).encode()).hexdigest()[:10]
    if "reaches" in r:
        return "reaches require_gpu, then " + outcome(r["then"])
    calls = "".join("%s(%s) " % (c["entry"], h(c["args"])) for c in r.get("calls", ()))
    end = "%s: %s" % (r["raises"], r["message"]) if "raises" in r else "-> " + h(r["returns"])
    return calls + end + (" [warnings: %s]" % "; ".join(r["warnings"]) if "warnings" in r else "")


# -------------------------------------------------------------------------------------------------------- inputs ----
def _sig(n):
    k = np.arange(n, dtype=np.int64)
    return ((k * 37 + 11) % 101 - 50) / 64.0 + ((k * k) % 17 - 8) / 32.0


def _cplx(shape, dtype):
    k = np.arange(int(np.prod(shape)), dtype=np.int64)
    return (((k * 29 + 5) % 97 - 48) / 16.0 + 1j * (((k * 13 + 7) % 89 - 44) / 32.0)).reshape(shape).astype(dtype)


def _real(shape, dtype):
    k = np.arange(int(np.prod(shape)), dtype=np.int64)
    return (((k * 31 + 3) % 127) / 256.0).reshape(shape).astype(dtype)


@functools.lru_cache(maxsize=None)
def inputs():
    z = SimpleNamespace()
    z.x = _sig(300)                                                       # float64 [300]
    z.xb = np.stack([_sig(300), 0.5 * _sig(300)[::-1]]).astype(np.float32)  # float32 [2, 300]
    z.x600 = _sig(600)
    z.x1 = np.array([1.0])                                                # the one-sample signal
    z.xi = np.arange(300)                                                 # an integer signal (cast to float64)
    z.win = 1.1 - np.abs(2.0 * np.arange(48) / 47.0 - 1.0)                # float64 [48]
    z.win16 = z.win[16:32].copy()                                         # 16 taps, for n_fft = 16
    z.t = 0.25 * np.arange(300)
    z.sc = 2.0 * 2.0 ** (np.arange(20) / 4)                               # 'log', nv = 4
    z.sc32 = z.sc.astype(np.float32)
    z.slin = np.linspace(2.0, 60.0, 20)
    z.slp = np.ascontiguousarray(up.process_scales("log-piecewise", 300, "gmw")).reshape(-1)
    z.slp_col = up.process_scales("log-piecewise", 300, "gmw")             # [na, 1], as upstream returns it
    z.flin = np.linspace(0.01, 0.5, 20)
    z.flog = 0.01 * 2.0 ** (np.arange(20) / 4)
    z.flin32 = z.flin.astype(np.float32)
    for name, dt in (("c128", np.complex128), ("c64", np.complex64)):
        setattr(z, "S_" + name, _cplx((33, 300), dt))                      # STFT maps, n_fft = 64
        setattr(z, "Sb_" + name, _cplx((2, 33, 300), dt))
        setattr(z, "W_" + name, _cplx((20, 300), dt))                      # CWT maps on `sc`
        setattr(z, "Wb_" + name, _cplx((2, 20, 300), dt))
    z.W_lp = _cplx((len(z.slp), 300), np.complex128)
    z.Wb_lp = _cplx((2, len(z.slp), 300), np.complex64)
    z.w = _real((20, 300), np.float64)
    z.wb = _real((2, 20, 300), np.float32)
    z.ws = _real((33, 300), np.float64)
    z.sfs = np.linspace(0, 0.5, 33)
    n = np.arange(300)
    z.cc = (5 + n % 7).astype(np.int64)                                    # [N]
    z.cc2 = np.stack([5 + n % 7, 12 + n % 5], axis=1)                      # [N, 2]
    z.cw = np.full(300, 2)
    z.cw2 = np.full((300, 2), 2.5)                                         # floats: truncated
    z.ccb = np.stack([z.cc2, z.cc2 + 1])                                   # [2, N, 2]
    z.cwb = np.full((2, 300, 2), 1)
    z.bins = ((np.arange(33 * 40).reshape(33, 40) * 5) % 34 - 1).astype(np.int32)
    z.binsb = np.stack([z.bins, z.bins[::-1] * 0 + 3]).astype(np.int32)
    z.vec = np.array([[1.0, 0.5j, 0.25], [0.5, 1.0, -1.0j]])
    return z


STFT_FAMILY = ("stft", "ssq_stft", "ssq_stft2", "mssq_stft", "tssq_stft", "reassign_stft")
POW2_N_FFT = ("ssq_stft2", "mssq_stft", "tssq_stft", "reassign_stft")
CWT_FAMILY = ("cwt", "cwt_higher_order", "ssq_cwt", "ssq_cwt2", "reassign_cwt", "tssq_cwt", "conceft_cwt")
PADTYPES = ("reflect", "zero", "symmetric", "replicate", "wrap")
GMW20 = ("gmw", {"gamma": 3, "beta": 20})
MORLET6 = ("morlet", {"mu": 6.0})

# the options of each forward transform, each moved off its default on its own (beside the family's common ones)
STFT_OPTIONS = {
    "stft": [dict(derivative=True), dict(dtype="float32")],
    "ssq_stft": [dict(get_w=True), dict(get_dWx=True), dict(get_w=True, get_dWx=True), dict(flipud=True),
                 dict(squeezing="lebesgue"), dict(gamma=1e-6), dict(gamma=None), dict(preserve_transform=True)],
    "ssq_stft2": [dict(get_w=True), dict(flipud=True), dict(squeezing="lebesgue"), dict(gamma=1e-6)],
    "mssq_stft": [dict(get_w=True), dict(get_bins=True), dict(get_w=True, get_bins=True), dict(flipud=True),
                  dict(squeezing="lebesgue"), dict(gamma=1e-6), dict(order=1), dict(order=2), dict(n_iter=1),
                  dict(n_iter=4), dict(n_iter=np.int64(7))],
    "tssq_stft": [dict(get_tau=True), dict(order=1), dict(order=2), dict(gamma=1e-6)],
    "reassign_stft": [dict(get_w=True), dict(get_tau=True), dict(get_w=True, get_tau=True), dict(gamma=1e-6)],
}
STFT_ALL_FLAGS = {
    "stft": dict(derivative=True), "ssq_stft": dict(get_w=True, get_dWx=True), "ssq_stft2": dict(get_w=True),
    "mssq_stft": dict(get_w=True, get_bins=True), "tssq_stft": dict(get_tau=True),
    "reassign_stft": dict(get_w=True, get_tau=True),
}
CWT_OPTIONS = {
    "cwt": [dict(derivative=True), dict(rpadded=True), dict(rpadded=True, derivative=True), dict(l1_norm=False),
            dict(order=(1,)), dict(order=(0, 1, 2)), dict(order=(0, 1, 2), average=False),
            dict(order=(1, 2), average=False, derivative=True), dict(order=range(3), average=True),
            dict(order=[2], average=True), dict(order=(0,)), dict(order=(0, 0), average=False), dict(order=0),
            dict(vectorized=False, astensor=False, cache_wavelet=True, nan_checks=True, patience=1)],
    "cwt_higher_order": [dict(order=2), dict(order=0), dict(order=(1, 3)), dict(order=(1, 3), average=False),
                         dict(order=(1, 3), average=False, derivative=True), dict(order=1, average=True),
                         dict(derivative=True), dict(rpadded=True), dict(l1_norm=True),
                         dict(vectorized=False, cache_wavelet=None, nan_checks=False, patience=0)],
    "ssq_cwt": [dict(get_w=True), dict(get_dWx=True), dict(get_w=True, get_dWx=True), dict(flipud=False),
                dict(squeezing="lebesgue"), dict(gamma=1e-6), dict(gamma=None), dict(order=1), dict(order=(0, 2)),
                dict(order=(0,)), dict(order=[1, 2], get_dWx=True), dict(difforder=4, preserve_transform=False)],
    "ssq_cwt2": [dict(get_w=True), dict(flipud=False), dict(squeezing="lebesgue"), dict(gamma=1e-6)],
    "reassign_cwt": [dict(get_w=True), dict(get_tau=True), dict(get_targets=True),
                     dict(get_w=True, get_tau=True, get_targets=True), dict(flipud=False), dict(gamma=1e-6)],
    "tssq_cwt": [dict(get_tau=True), dict(get_targets=True), dict(get_tau=True, get_targets=True), dict(order=1),
                 dict(order=2), dict(gamma=1e-6), dict(work_limit_bytes=1 << 30)],
    "conceft_cwt": [dict(get_Wx=True), dict(get_w=True), dict(get_Wx=True, get_w=True), dict(flipud=False),
                    dict(gamma=1e-6), dict(orders=2), dict(orders=(0, 2, 5)), dict(orders=[3]), dict(orders=range(1, 3)),
                    dict(n_draws=3, seed=7), dict(squeezing="sum")],
}
CWT_ALL_FLAGS = {
    "cwt": dict(derivative=True), "cwt_higher_order": dict(derivative=True, order=(1, 2), average=False),
    "ssq_cwt": dict(get_w=True, get_dWx=True), "ssq_cwt2": dict(get_w=True),
    "reassign_cwt": dict(get_w=True, get_tau=True, get_targets=True), "tssq_cwt": dict(get_tau=True, get_targets=True),
    "conceft_cwt": dict(get_Wx=True, get_w=True, n_draws=3),
}
HAS_FREQS = ("ssq_cwt", "ssq_cwt2", "reassign_cwt", "conceft_cwt")       # take ssq_freqs and maprange
TAKES_GAMMA = ("ssq_stft", "ssq_stft2", "mssq_stft", "tssq_stft", "reassign_stft", "ssq_cwt", "ssq_cwt2", "reassign_cwt",
               "tssq_cwt", "conceft_cwt")


def _r(v):
    """repr for a case id, spelled the same under every numpy."""
    return _tag({"": v})[1:]


def _tag(kw):
    def word(v):
        if isinstance(v, np.ndarray):
            named = [n for n, a in vars(inputs()).items() if a is v]
            return named[0] if named else "%s%s" % (v.dtype, list(v.shape))
        if isinstance(v, dict):
            return _tag(v)
        if isinstance(v, (tuple, list)):
            return "(" + ",".join(word(e) for e in v) + ")" if len(v) < 8 else "%s[%d]" % (type(v).__name__, len(v))
        if isinstance(v, np.generic):
            return "%s(%r)" % (type(v).__name__, v.item())
        return getattr(v, "__name__", None) or repr(v)
    return ",".join("%s=%s" % (k, word(v)) for k, v in kw.items()) or "defaults"


def _accepted(z):
    cases = {}

    def add(cid, fn, *a, **k):
        assert cid not in cases, cid
        cases[cid] = (fn, a, k)

    # ---- STFT family: n_fft = 64 on 300 samples, each option on its own; the default n_fft = 512 on 600 samples
    for fn in STFT_FAMILY:
        base = dict(window=z.win, n_fft=64)
        add(f"{fn}/600,default n_fft", fn, z.x600, window=z.win)
        add(f"{fn}/int signal", fn, z.xi, **base)
        for xname in ("x", "xb"):
            add(f"{fn}/{xname}", fn, getattr(z, xname), **base)
            add(f"{fn}/{xname},all flags", fn, getattr(z, xname), **base, **STFT_ALL_FLAGS[fn])
        common = [dict(padtype=p) for p in (PADTYPES if fn == "stft" else ("wrap",))] + [
            dict(modulated=False), dict(fs=4.0), dict(t=z.t), dict(hop_len=3), dict(n_fft=16, window=z.win16), dict(win_len=32)]
        for kw in common + STFT_OPTIONS[fn]:
            add(f"{fn}/x,{_tag(kw)}", fn, z.x, **{**base, **kw})
    add("stft/any-length n_fft", "stft", z.x, window=z.win, n_fft=60)
    add("ssq_stft/any-length n_fft", "ssq_stft", z.xb, window=z.win, n_fft=50, hop_len=3, get_w=True)

    # ---- CWT family on the 20-row log grid, each option on its own
    for fn in CWT_FAMILY:
        base = dict(scales=z.sc)
        for xname in ("x", "xb"):
            add(f"{fn}/{xname}", fn, getattr(z, xname), **base)
            add(f"{fn}/{xname},all flags", fn, getattr(z, xname), **base, **CWT_ALL_FLAGS[fn])
        add(f"{fn}/int signal", fn, z.xi, **base)
        common = [dict(padtype=p) for p in (PADTYPES if fn == "ssq_cwt" else ("wrap",))] + [
            dict(fs=4.0), dict(t=z.t), dict(nv=4), dict(scales=z.sc32), dict(scales=z.slin), dict(scales=z.slp),
            dict(scales=z.slp.astype(np.float32)), dict(wavelet=GMW20)]
        if fn != "conceft_cwt":
            common += [dict(wavelet="morlet"), dict(wavelet=MORLET6)]
        if fn in HAS_FREQS:
            common += [dict(ssq_freqs="linear"), dict(ssq_freqs=z.flin), dict(ssq_freqs=z.flog), dict(ssq_freqs=z.flin32),
                       dict(maprange="maximal"), dict(scales=z.slp, ssq_freqs="log-piecewise"),
                       dict(scales=z.slp, maprange="maximal", ssq_freqs="log"), dict(ssq_freqs="log-piecewise")]
        for kw in common + CWT_OPTIONS[fn]:
            add(f"{fn}/x,{_tag(kw)}", fn, z.x, **{**base, **kw})
    add("conceft_cwt/vectors", "conceft_cwt", z.x, scales=z.sc, vectors=z.vec)
    add("conceft_cwt/vectors,xb,flags", "conceft_cwt", z.xb, scales=z.sc, vectors=z.vec, get_Wx=True, get_w=True)
    add("conceft_cwt/vectors e0", "conceft_cwt", z.x, scales=z.sc, orders=2, vectors=[[1, 0]])
    add("conceft_cwt/vectors,orders tuple", "conceft_cwt", z.x, scales=z.slp, orders=(1, 4), vectors=z.vec[:, :2].real)

    # ---- the inverses, on 2-D and batched 3-D maps
    for S, Sb, tag in ((z.S_c128, z.Sb_c64, "c128"),):
        for m, mt in ((S, "2d"), (Sb, "c64,3d")):
            add(f"istft/{tag},{mt}", "istft", m, window=z.win)
            add(f"istft/{tag},{mt},options", "istft", m, window=z.win, n_fft=64, win_len=48, hop_len=3, N=700,
                modulated=False, win_exp=2)
            add(f"issq_stft/{tag},{mt}", "issq_stft", m, window=z.win)
            add(f"issq_stft/{tag},{mt},n_fft,win_len", "issq_stft", m, window=z.win, n_fft=64, win_len=40)
    for W, Wb, tag in ((z.W_c128, z.Wb_c64, "c128"),):
        for m, mt in ((W, "2d"), (Wb, "c64,3d")):
            for wv in ("gmw", "morlet", GMW20):
                add(f"issq_cwt/{tag},{mt},{_tag(dict(wavelet=wv))}", "issq_cwt", m, wv)
            add(f"icwt/{tag},{mt},log", "icwt", m, scales=z.sc)
            add(f"icwt/{tag},{mt},log,float32 scales,nv", "icwt", m, scales=z.sc32, nv=4)
            add(f"icwt/{tag},{mt},linear", "icwt", m, scales=z.slin)
            add(f"icwt/{tag},{mt},linear,l1_norm=False", "icwt", m, "morlet", scales=z.slin, l1_norm=False)
            add(f"icwt/{tag},{mt},log,l1_norm=False", "icwt", m, scales=z.sc, l1_norm=False)
            add(f"icwt/{tag},{mt},x_mean scalar", "icwt", m, scales=z.sc, x_mean=1.5)
            add(f"icwt/{tag},{mt},unused options", "icwt", m, scales=z.sc, x_len=300, padtype="bogus", rpadded=True)
        add(f"icwt/{tag},3d,x_mean per signal", "icwt", Wb, scales=z.sc, x_mean=np.array([1.5, -2.0]))
        add(f"icwt/{tag},3d,x_mean list", "icwt", Wb, scales=z.slin, x_mean=[1, 2])
        add(f"icwt/{tag},3d,x_mean 0-d", "icwt", Wb, scales=z.sc, x_mean=np.float32(0.5))
    add("icwt/log-piecewise,2d", "icwt", z.W_lp, scales=z.slp)
    add("icwt/log-piecewise,2d,x_mean", "icwt", z.W_lp, scales=z.slp_col, x_mean=0.75, l1_norm=False)
    add("icwt/log-piecewise,3d", "icwt", z.Wb_lp, scales=z.slp)
    add("icwt/log-piecewise,3d,x_mean per signal", "icwt", z.Wb_lp, scales=z.slp.astype(np.float32),
        x_mean=np.array([1.5, -2.0]))
    # the component inversions by curves
    for fn, extra in (("issq_cwt", dict(wavelet="gmw")), ("issq_stft", dict(window=z.win))):
        W, Wb = (z.W_c128, z.Wb_c64) if fn == "issq_cwt" else (z.S_c64, z.Sb_c128)
        add(f"{fn}/cc 1-D", fn, W, cc=z.cc, cw=z.cw, **extra)
        add(f"{fn}/cc 2-D", fn, W, cc=z.cc2, cw=z.cw2, **extra)
        add(f"{fn}/cc 2-D,cw 1 column broadcast", fn, W, cc=z.cc2[:, :1], cw=z.cw2, **extra)
        add(f"{fn}/cc 2-D,cw wider", fn, W, cc=z.cc2.astype(np.float64) + 0.75, cw=np.full((300, 3), 1), **extra)
        add(f"{fn}/batched,cc 3-D", fn, Wb, cc=z.ccb, cw=z.cwb, **extra)
        add(f"{fn}/batched,cc 2-D", fn, Wb, cc=z.ccb[:, :, 0], cw=z.cwb[:, :, 0], **extra)
    add("issq_stft/cc,n_fft,win_len", "issq_stft", z.S_c128, window=z.win, cc=z.cc, cw=z.cw, n_fft=64, win_len=40)

    # ---- ssqueeze on a held transform
    for W, w, tag in ((z.W_c128, z.w, "2d"), (z.Wb_c64, z.wb, "3d")):
        base = dict(w=w, scales=z.sc)
        kws = [dict(), dict(wavelet="gmw", maprange="peak"), dict(squeezing="abs"), dict(squeezing=np.abs),
               dict(w=None, dWx=W[..., ::-1, :]), dict(w=None, dWx=W, flipud=True, wavelet="morlet", maprange="peak")]
        if tag == "2d":
            kws += [dict(wavelet=MORLET6, maprange="peak", was_padded=False), dict(was_padded=False),
                    dict(ssq_freqs="linear"), dict(ssq_freqs=z.flin), dict(ssq_freqs=z.flog), dict(ssq_freqs=z.flin32),
                    dict(squeezing="lebesgue"), dict(squeezing=np.conj), dict(flipud=True), dict(fs=4.0), dict(t=z.t),
                    dict(scales=z.slin), dict(scales=z.sc32), dict(w=(w * 8).astype(np.int32)),
                    dict(w=None, dWx=W[..., ::-1, :], gamma=1e-6), dict(w=None, dWx=W.astype(np.complex64))]
        for kw in kws:
            add(f"ssqueeze/cwt,{tag},{_tag(kw)}", "ssqueeze", W, **{**base, **kw})
    for kw in (dict(ssq_freqs="log-piecewise", maprange="peak", wavelet="gmw"), dict(maprange="peak", wavelet="gmw"),
               dict(maprange="peak", wavelet="gmw", was_padded=False), dict(ssq_freqs="log")):
        add(f"ssqueeze/cwt,log-piecewise scales,{_tag(kw)}", "ssqueeze", z.W_lp, w=_real(z.W_lp.shape, np.float64),
            scales=z.slp, **kw)
    for S, w, tag in ((z.S_c128, z.ws, "2d"), (z.Sb_c64, np.stack([z.ws, z.ws]), "3d")):
        base = dict(w=w, ssq_freqs=z.sfs, transform="stft")
        for kw in (dict(), dict(flipud=True), dict(squeezing="lebesgue"), dict(squeezing="abs"), dict(squeezing=np.abs),
                   dict(scales=z.sc, fs=2.0), dict(ssq_freqs=z.sfs.astype(np.float32)),
                   dict(w=None, dWx=S, Sfs=z.sfs), dict(w=None, dWx=S, Sfs=list(z.sfs), gamma=1e-6, flipud=True)):
            add(f"ssqueeze/stft,{tag},{_tag(kw)}", "ssqueeze", S, **{**base, **kw})

    # ---- the phase transforms, the walk, the ridges
    for W, tag in ((z.W_c128, "c128,2d"), (z.Wb_c64, "c64,3d")):
        add(f"phase_cwt/{tag}", "phase_cwt", W, W[..., ::-1, :])
        add(f"phase_cwt/{tag},gamma", "phase_cwt", W, W[..., ::-1, :], gamma=1e-6, parallel=True)
    for S, tag in ((z.S_c64, "c64,2d"), (z.Sb_c128, "c128,3d")):
        add(f"phase_stft/{tag}", "phase_stft", S, S[..., ::-1, :], z.sfs)
        add(f"phase_stft/{tag},gamma", "phase_stft", S, S[..., ::-1, :], list(z.sfs), gamma=1e-6)
    add("msst_walk/2d", "msst_walk", z.bins, 4)
    add("msst_walk/3d", "msst_walk", z.binsb, 1)
    add("msst_walk/strided", "msst_walk", z.binsb[:, :, ::2], np.int32(64))
    add("msst_tile_cols/33", "msst_tile_cols", 33)
    add("msst_tile_cols/2049", "msst_tile_cols", 2049)
    maps = (("c64", z.W_c64, z.Wb_c64), ("c128", z.W_c128, z.Wb_c128), ("f64", z.w, z.wb.astype(np.float64)),
            ("f32", z.w.astype(np.float32), z.wb), ("int", (z.w * 100).astype(np.int32), (z.wb * 100).astype(np.int64)))
    for tag, m, mb in maps:
        add(f"extract_ridges/{tag},2d", "extract_ridges", m, z.sc)
        add(f"extract_ridges/{tag},2d,get_params", "extract_ridges", m, z.sc, get_params=True)
        add(f"extract_ridges/{tag},3d", "extract_ridges", mb, z.sc.reshape(-1, 1), penalty=0.5, n_ridges=3, bw=4)
        add(f"extract_ridges/{tag},3d,get_params,stft", "extract_ridges", mb, z.slin, n_ridges=np.int64(2), bw=2.5,
            transform="stft", get_params=True, parallel=False)
    add("extract_ridges/list map", "extract_ridges", z.w.tolist(), list(z.sc))

    # ---- the small public helpers
    for wv in ("gmw", "morlet", GMW20, MORLET6):
        add(f"adm_ssq/{_tag(dict(wavelet=wv))}", "adm_ssq", wv)
        add(f"adm_cwt/{_tag(dict(wavelet=wv))}", "adm_cwt", wv)
        add(f"tssq_cwt_row_freqs/{_tag(dict(wavelet=wv))}", "tssq_cwt_row_freqs", wv, z.sc32)
    for n in (1, 300, 512, 513):
        add(f"p2up/{n}", "p2up", n)
    add("get_window/no n_fft", "get_window", z.win.astype(np.float32), 48)
    add("get_window/padded", "get_window", z.win, 48, 64)
    add("get_window/win_len below len", "get_window", z.win, 40, 64)
    add("get_window/exact", "get_window", z.win, 48, 48)
    add("gmw_k_constants/3,60,2", "gmw_k_constants", 3, 60, 2)
    add("gmw_order_coefficients/average", "gmw_order_coefficients", 3.0, 60.0, (0, 1, 3))
    add("gmw_order_coefficients/each", "gmw_order_coefficients", 3.0, 60.0, [2, 0], average=False)
    add("gmw_adm_ssq/order 0", "gmw_adm_ssq", 3, 60, 0)
    add("gmw_adm_ssq/order 5", "gmw_adm_ssq", 3.0, 60.0, 5)
    add("gmw_adm_ssq/lgamma branch", "gmw_adm_ssq", 1.0, 200.0, 3)
    add("conceft_vectors/4,3", "conceft_vectors", 4, 3, 0, [1.0, 0.5, 0.25])
    add("reassign_cwt_quantum_log2/20,300", "reassign_cwt_quantum_log2", 20, 300)
    add("reassign_cwt_quantum_log2/large", "reassign_cwt_quantum_log2", 1 << 10, 1 << 26)
    add("tssq_cwt_quantum_log2/300", "tssq_cwt_quantum_log2", 300)
    add("tssq_cwt_quantum_log2/large", "tssq_cwt_quantum_log2", 1 << 26)
    return cases


def _refusals(z):
    cases = {}

    def add(cid, fn, *a, **k):
        assert cid not in cases, cid
        cases[cid] = (fn, a, k)

    # ---- every forward transform: the faults they share, and the drifted ones by name
    for fn in STFT_FAMILY:
        base = dict(window=z.win, n_fft=64)
        add(f"{fn}/x a list", fn, list(z.x), **base)
        add(f"{fn}/one sample", fn, z.x1, **base)
        add(f"{fn}/one sample,default n_fft", fn, z.x1, window=z.win)
        add(f"{fn}/bad padtype", fn, z.x, **base, padtype="constant")
        add(f"{fn}/t of another length", fn, z.x, **base, t=np.arange(10))
        add(f"{fn}/no window", fn, z.x, n_fft=64)
        add(f"{fn}/win_len > n_fft", fn, z.x, window=z.win, n_fft=32)
        for n_fft in (60, 8, True):
            add(f"{fn}/n_fft={_r(n_fft)}", fn, z.x, window=np.ones(8), n_fft=n_fft)
        add(f"{fn}/default n_fft 300", fn, z.x, window=z.win)
        add(f"{fn}/hop_len=0", fn, z.x, **base, hop_len=0)                  # divides by zero after the GPU is asked for
        if fn in TAKES_GAMMA:
            add(f"{fn}/gamma NaN", fn, z.x, **base, gamma=NAN)
        if "squeezing" in STFT_KW[fn]:
            add(f"{fn}/squeezing abs", fn, z.x, **base, squeezing="abs")
        if "order" in STFT_KW[fn]:
            for order in (0, True, "2"):
                add(f"{fn}/order={_r(order)}", fn, z.x, **base, order=order)
    add("ssq_stft/ssq_freqs given", "ssq_stft", z.x, window=z.win, n_fft=64, ssq_freqs="linear")
    for n_iter in (0, 65, True):
        add(f"mssq_stft/n_iter={_r(n_iter)}", "mssq_stft", z.x, window=z.win, n_fft=64, n_iter=n_iter)
        add(f"msst_walk/n_iter={_r(n_iter)}", "msst_walk", z.bins, n_iter)

    for fn in CWT_FAMILY:
        base = dict(scales=z.sc)
        add(f"{fn}/x a list", fn, list(z.x), **base)
        add(f"{fn}/one sample", fn, z.x1, **base)
        add(f"{fn}/bad padtype", fn, z.x, **base, padtype="constant")
        add(f"{fn}/nv mismatch", fn, z.x, **base, nv=8)
        add(f"{fn}/wavelet gamma=inf", fn, z.x, ("gmw", {"gamma": INF}), **base)
        add(f"{fn}/wavelet beta=inf", fn, z.x, ("gmw", {"beta": INF}), **base)
        add(f"{fn}/wavelet beta=-1", fn, z.x, ("gmw", {"beta": -1.0}), **base)
        add(f"{fn}/wavelet mu=0", fn, z.x, ("morlet", {"mu": 0.0}), **base)
        add(f"{fn}/wavelet bump", fn, z.x, "bump", **base)
        add(f"{fn}/wavelet gmw order 1", fn, z.x, ("gmw", {"order": 1}), **base)
        add(f"{fn}/scales default string", fn, z.x)
        add(f"{fn}/scales one", fn, z.x, scales=np.array([4.0]))
        add(f"{fn}/scales negative", fn, z.x, scales=-z.sc)
        add(f"{fn}/scales with inf", fn, z.x, scales=np.concatenate([z.sc, [INF]]))
        add(f"{fn}/scales log-piecewise short segment", fn, z.x,
            scales=np.concatenate([z.sc[:1], z.sc[1] * 2.0 ** (np.arange(19) / 8)]))
        add(f"{fn}/fs=-1", fn, z.x, **base, fs=-1.0)
        add(f"{fn}/fs=nan", fn, z.x, **base, fs=NAN)
        add(f"{fn}/t of another length", fn, z.x, **base, t=np.arange(10))
        if fn in TAKES_GAMMA:
            add(f"{fn}/gamma NaN", fn, z.x, **base, gamma=NAN)
        if fn in HAS_FREQS:
            add(f"{fn}/ssq_freqs of another length", fn, z.x, **base, ssq_freqs=z.flin[:10])
            add(f"{fn}/ssq_freqs a number", fn, z.x, **base, ssq_freqs=5)
            add(f"{fn}/ssq_freqs bogus", fn, z.x, **base, ssq_freqs="bogus")
            add(f"{fn}/ssq_freqs with inf", fn, z.x, **base, ssq_freqs=np.concatenate([z.flin[:-1], [INF]]))
            add(f"{fn}/log-piecewise with maximal", fn, z.x, scales=z.slp, maprange="maximal")
            add(f"{fn}/maprange bogus", fn, z.x, **base, maprange="bogus")
        if "squeezing" in CWT_KW[fn]:
            add(f"{fn}/squeezing abs", fn, z.x, **base, squeezing="abs")
        if fn in ("reassign_cwt", "tssq_cwt", "conceft_cwt"):               # the C entries' shape checks, on the host
            add(f"{fn}/too many rows", fn, z.x, scales=2.0 * 2.0 ** (np.arange(40000) / 4096),
                **({} if fn == "tssq_cwt" else {"maprange": "maximal"}))
        if fn in ("ssq_cwt2", "reassign_cwt", "conceft_cwt"):               # 'peak' frequencies that overflow
            add(f"{fn}/generated ssq_freqs not finite", fn, z.x, scales=2.0 * 2.0 ** (np.arange(40000) / 4096))
    for order in (0, True, "2"):
        add(f"tssq_cwt/order={_r(order)}", "tssq_cwt", z.x, scales=z.sc, order=order)
    add("tssq_cwt/work_limit_bytes small", "tssq_cwt", z.x, scales=z.sc, work_limit_bytes=1024)
    add("tssq_cwt/work_limit_bytes 0", "tssq_cwt", z.x, scales=z.sc, work_limit_bytes=0)
    add("tssq_cwt/row_freqs underflow", "tssq_cwt", z.x, ("morlet", {"mu": 1e-300}), scales=1e300 * z.sc)
    add("tssq_cwt/ssq_freqs gone", "tssq_cwt", z.x, scales=z.sc, ssq_freqs=None)
    add("ssq_cwt/difftype", "ssq_cwt", z.x, scales=z.sc, difftype="phase")
    add("ssq_cwt/scales with zero", "ssq_cwt", z.x, scales=np.concatenate([[0.0], z.sc]))     # (no positivity check there)
    # the orders of cwt, cwt_higher_order, ssq_cwt
    for fn, key in (("cwt", "order"), ("cwt_higher_order", "order"), ("ssq_cwt", "order")):
        for order in (1, -1, 17, (0, 17), (), 1.5, True, (1, 2.0)):
            add(f"{fn}/order={_r(order)}", fn, z.x, scales=z.sc, order=order)
        add(f"{fn}/order with morlet", fn, z.x, "morlet", scales=z.sc, order=(1, 2))
        add(f"{fn}/order 0 set with morlet", fn, z.x, "morlet", scales=z.sc, order=(0,))
    add("cwt/order with l1_norm=False", "cwt", z.x, scales=z.sc, order=(1,), l1_norm=False)
    add("cwt/order 0 set with l1_norm=False", "cwt", z.x, scales=z.sc, order=(0,), l1_norm=False)
    add("cwt_higher_order/order with l1_norm=False", "cwt_higher_order", z.x, scales=z.sc, order=1, l1_norm=False)
    add("cwt_higher_order/order 0 with morlet", "cwt_higher_order", z.x, "morlet", scales=z.sc, order=0)
    add("cwt_higher_order/unexpected keyword", "cwt_higher_order", z.x, scales=z.sc, bogus=1, gamma=2)
    add("cwt/single order averaged", "cwt", z.x, scales=z.sc, order=(2,), average=True)
    # conceft_cwt's own
    cb = dict(scales=z.sc)
    add("conceft_cwt/morlet", "conceft_cwt", z.x, "morlet", **cb)
    add("conceft_cwt/morlet tuple", "conceft_cwt", z.x, MORLET6, **cb)
    for orders in (True, 0, 9, 2.0, "3", None, (1, True), (1, 2.0), (0, 17), (-1, 2), (), tuple(range(9)), (1, 1),
                   np.int64(3)):
        add(f"conceft_cwt/orders={_r(orders)}", "conceft_cwt", z.x, **cb, orders=orders)
    for n_draws in (0, 257, True, 2.0, None):
        add(f"conceft_cwt/n_draws={_r(n_draws)}", "conceft_cwt", z.x, **cb, n_draws=n_draws)
    add("conceft_cwt/vectors 1-D", "conceft_cwt", z.x, **cb, vectors=[1, 0, 0])
    add("conceft_cwt/vectors columns", "conceft_cwt", z.x, **cb, vectors=np.ones((2, 2)))
    add("conceft_cwt/vectors strings", "conceft_cwt", z.x, **cb, vectors=np.array([["a", "b", "c"]]))
    add("conceft_cwt/vectors no draw", "conceft_cwt", z.x, **cb, vectors=np.ones((0, 3)))
    add("conceft_cwt/vectors 257 draws", "conceft_cwt", z.x, **cb, vectors=np.ones((257, 3)))
    add("conceft_cwt/vectors nan", "conceft_cwt", z.x, **cb, vectors=[[1, NAN, 0]])
    add("conceft_cwt/vectors zero row", "conceft_cwt", z.x, **cb, vectors=[[1, 0, 0], [0, 0, 0]])
    add("conceft_cwt/vectors degenerate", "conceft_cwt", z.x, **cb, orders=2, vectors=_degenerate())
    add("conceft_cwt/J na too large", "conceft_cwt", z.x, scales=2.0 * 2.0 ** (np.arange(20000) / 4096), orders=2)
    add("conceft_vectors/n_draws bool", "conceft_vectors", True, 3, 0, [1, 1, 1])
    add("conceft_vectors/n_orders float", "conceft_vectors", 2, 3.0, 0, [1, 1, 1])
    add("conceft_vectors/n_draws 0", "conceft_vectors", 0, 3, 0, [1, 1, 1])
    add("conceft_vectors/n_orders 9", "conceft_vectors", 2, 9, 0, [1] * 9)
    add("conceft_vectors/adm length", "conceft_vectors", 2, 3, 0, [1, 1])
    add("_conceft_gauge/shape", "_conceft_gauge", np.ones((2, 3)), [1, 1])
    for a, tag in (((0.0, 60.0, 0), "gamma 0"), ((3.0, INF, 0), "beta inf"), ((3.0, 60.0, 17), "order 17"),
                   ((3.0, 60.0, -1), "order -1")):
        add(f"gmw_adm_ssq/{tag}", "gmw_adm_ssq", *a)
    add("reassign_cwt_quantum_log2/0", "reassign_cwt_quantum_log2", 0, 300)
    add("tssq_cwt_quantum_log2/0", "tssq_cwt_quantum_log2", 0)
    add("tssq_cwt_row_freqs/gamma inf", "tssq_cwt_row_freqs", ("gmw", {"gamma": INF}), z.sc)
    add("tssq_cwt_row_freqs/scales negative", "tssq_cwt_row_freqs", "gmw", -z.sc)
    add("tssq_cwt_row_freqs/bump", "tssq_cwt_row_freqs", "bump", z.sc)
    add("msst_tile_cols/0", "msst_tile_cols", 0)
    add("msst_tile_cols/2050", "msst_tile_cols", 2050)
    add("adm_ssq/bump", "adm_ssq", "bump")
    add("get_window/list", "get_window", [1.0, 2.0], 2, 4)
    # msst_walk
    add("msst_walk/int64", "msst_walk", z.bins.astype(np.int64), 2)
    add("msst_walk/1-D", "msst_walk", z.bins[0], 2)
    add("msst_walk/a list", "msst_walk", z.bins.tolist(), 2)
    add("msst_walk/too many rows", "msst_walk", np.zeros((2050, 2), dtype=np.int32), 2)
    add("msst_walk/empty axis", "msst_walk", np.zeros((3, 0), dtype=np.int32), 2)
    add("msst_walk/empty batch", "msst_walk", np.zeros((0, 3, 4), dtype=np.int32), 2)
    add("msst_walk/target below -1", "msst_walk", z.bins - 1, 2)
    add("msst_walk/target F", "msst_walk", z.bins + 1, 2)

    # ---- the inverses
    for fn, kw in (("istft", dict(window=z.win)), ("issq_stft", dict(window=z.win)), ("issq_cwt", dict()),
                   ("icwt", dict(scales=z.sc))):
        good = z.S_c128 if "stft" in fn else z.W_c128
        add(f"{fn}/a list", fn, good.tolist(), **kw)
        add(f"{fn}/real map", fn, good.real, **kw)
        add(f"{fn}/1-D", fn, good[0], **kw)
        add(f"{fn}/4-D", fn, good[None, None], **kw)
        add(f"{fn}/B == 0", fn, good[None][:0], **kw)
        add(f"{fn}/well formed", fn, good, **kw)
    add("istft/rows against n_fft", "istft", z.S_c128, window=z.win, n_fft=128)
    add("istft/win_len > n_fft", "istft", z.S_c128, window=np.ones(80))
    add("istft/no window", "istft", z.S_c128)
    add("issq_stft/modulated=False", "issq_stft", z.S_c128, window=z.win, modulated=False)
    add("issq_stft/hop_len", "issq_stft", z.S_c128, window=z.win, hop_len=2)
    add("issq_stft/no window", "issq_stft", z.S_c128)
    add("issq_stft/no window,cc", "issq_stft", z.S_c128, cc=z.cc, cw=z.cw)
    add("issq_stft/win_len > n_fft,cc", "issq_stft", z.S_c128, window=np.ones(80), cc=z.cc, cw=z.cw)
    add("issq_stft/win_len > n_fft", "issq_stft", z.S_c128, window=np.ones(80))
    add("issq_cwt/bump", "issq_cwt", z.W_c128, "bump")
    for fn, extra in (("issq_cwt", dict()), ("issq_stft", dict(window=z.win))):
        W, Wb = (z.W_c128, z.Wb_c64) if fn == "issq_cwt" else (z.S_c64, z.Sb_c128)
        add(f"{fn}/cc alone", fn, W, cc=z.cc, **extra)
        add(f"{fn}/cw alone", fn, W, cw=z.cw, **extra)
        add(f"{fn}/cc,real map", fn, W.real, cc=z.cc, cw=z.cw, **extra)
        add(f"{fn}/cc 3-D for 2-D map", fn, W, cc=z.ccb, cw=z.cwb, **extra)
        add(f"{fn}/cw 0-d", fn, W, cc=z.cc, cw=2, **extra)
        add(f"{fn}/cc 1-D for batched map", fn, Wb, cc=z.cc, cw=z.cw, **extra)
        add(f"{fn}/cc rows", fn, W, cc=z.cc[:100], cw=z.cw[:100], **extra)
        add(f"{fn}/cc rows,batched", fn, Wb, cc=z.ccb[:1], cw=z.cwb[:1], **extra)
        add(f"{fn}/cc no component", fn, W, cc=z.cc2[:, :0], cw=z.cw2, **extra)
        add(f"{fn}/cw narrower", fn, W, cc=z.cc2, cw=z.cw2[:, :1], **extra)
        add(f"{fn}/cw does not broadcast", fn, W, cc=z.cc2, cw=z.cw2[:100], **extra)
    add("icwt/one_int=False", "icwt", z.W_c128, scales=z.sc, one_int=False)
    add("icwt/row count", "icwt", z.W_c128, scales=z.sc[:10])
    add("icwt/scales default string", "icwt", z.W_c128)
    add("icwt/x_mean 2-D", "icwt", z.Wb_c128, scales=z.sc, x_mean=np.zeros((2, 1)))
    add("icwt/x_mean of another length", "icwt", z.Wb_c128, scales=z.sc, x_mean=np.zeros(3))
    add("icwt/bump", "icwt", z.W_c128, "bump", scales=z.sc)

    # ---- ssqueeze and the phase transforms
    sb = dict(w=z.w, scales=z.sc)
    W = z.W_c128
    add("ssqueeze/transform", "ssqueeze", W, **sb, transform="fft")
    add("ssqueeze/Wx a list", "ssqueeze", W.tolist(), **sb)
    add("ssqueeze/Wx real", "ssqueeze", W.real, **sb)
    add("ssqueeze/no w, no dWx", "ssqueeze", W, scales=z.sc)
    add("ssqueeze/w shape", "ssqueeze", W, w=z.w[:10], scales=z.sc)
    add("ssqueeze/w complex", "ssqueeze", W, w=W, scales=z.sc)
    add("ssqueeze/w negative", "ssqueeze", W, w=z.w - 0.25, scales=z.sc)
    add("ssqueeze/squeezing bogus", "ssqueeze", W, **sb, squeezing="max")
    add("ssqueeze/squeezing a number", "ssqueeze", W, **sb, squeezing=3)
    add("ssqueeze/lebesgue from dWx", "ssqueeze", W, dWx=W, scales=z.sc, squeezing="lebesgue")
    add("ssqueeze/function from dWx", "ssqueeze", W, dWx=W, scales=z.sc, squeezing=np.abs)
    add("ssqueeze/maprange energy", "ssqueeze", W, **sb, maprange="energy")
    add("ssqueeze/maprange tuple", "ssqueeze", W, **sb, maprange=(0.1, 0.4))
    add("ssqueeze/maprange bogus", "ssqueeze", W, **sb, maprange="bogus")
    add("ssqueeze/t of another length", "ssqueeze", W, **sb, t=np.arange(10))
    add("ssqueeze/scales None", "ssqueeze", W, w=z.w)
    add("ssqueeze/scales a string", "ssqueeze", W, w=z.w, scales="log")
    add("ssqueeze/scales rows", "ssqueeze", W, w=z.w, scales=z.sc[:10])
    add("ssqueeze/log-piecewise with maximal", "ssqueeze", z.W_lp, w=_real(z.W_lp.shape, np.float64), scales=z.slp)
    add("ssqueeze/peak without wavelet", "ssqueeze", W, **sb, maprange="peak")
    add("ssqueeze/peak with bump", "ssqueeze", W, **sb, maprange="peak", wavelet="bump")
    add("ssqueeze/ssq_freqs a number", "ssqueeze", W, **sb, ssq_freqs=5)
    add("ssqueeze/ssq_freqs bogus", "ssqueeze", W, **sb, ssq_freqs="bogus")
    add("ssqueeze/ssq_freqs rows", "ssqueeze", W, **sb, ssq_freqs=z.flin[:10])
    add("ssqueeze/function result shape", "ssqueeze", W, **sb, squeezing=lambda A: A[:10])
    add("ssqueeze/dWx shape", "ssqueeze", W, dWx=W[:10], scales=z.sc)
    add("ssqueeze/dWx real", "ssqueeze", W, dWx=W.real, scales=z.sc)
    add("ssqueeze/gamma NaN from dWx", "ssqueeze", W, dWx=W, scales=z.sc, gamma=NAN)
    add("ssqueeze/gamma NaN from w", "ssqueeze", W, **sb, gamma=NAN)
    st = dict(w=z.ws, ssq_freqs=z.sfs, transform="stft")
    S = z.S_c128
    add("ssqueeze/stft,ssq_freqs None", "ssqueeze", S, w=z.ws, transform="stft")
    add("ssqueeze/stft,ssq_freqs a string", "ssqueeze", S, w=z.ws, ssq_freqs="linear", transform="stft")
    add("ssqueeze/stft,no Sfs from dWx", "ssqueeze", S, dWx=S, ssq_freqs=z.sfs, transform="stft")
    add("ssqueeze/stft,Sfs rows", "ssqueeze", S, dWx=S, ssq_freqs=z.sfs, Sfs=z.sfs[:10], transform="stft")
    add("ssqueeze/stft,Sfs[0]", "ssqueeze", S, dWx=S, ssq_freqs=z.sfs, Sfs=z.sfs + 0.01, transform="stft")
    add("ssqueeze/stft,ssq_freqs rows", "ssqueeze", S, **{**st, "ssq_freqs": z.sfs[:10]})
    add("phase_cwt/difftype", "phase_cwt", W, W, difftype="phase")
    add("phase_cwt/Wx a list", "phase_cwt", W.tolist(), W)
    add("phase_cwt/dWx shape", "phase_cwt", W, W[:10])
    add("phase_cwt/gamma NaN", "phase_cwt", W, W, gamma=NAN)
    add("phase_stft/Sx real", "phase_stft", S.real, S, z.sfs)
    add("phase_stft/Sfs None", "phase_stft", S, S, None)
    add("phase_stft/Sfs rows", "phase_stft", S, S, z.sfs[:10])
    add("phase_stft/dSx real", "phase_stft", S, S.real, z.sfs)
    add("phase_stft/gamma NaN", "phase_stft", S, S, z.sfs, gamma=NAN)

    # ---- extract_ridges
    add("extract_ridges/1-D", "extract_ridges", z.w[0], z.sc)
    add("extract_ridges/strings", "extract_ridges", np.full((20, 30), "a"), z.sc)
    add("extract_ridges/scales length", "extract_ridges", z.w, z.sc[:10])
    add("extract_ridges/scales 2-D", "extract_ridges", z.w, z.sc.reshape(1, -1))
    add("extract_ridges/scales 3-D", "extract_ridges", z.w, z.sc.reshape(-1, 1, 1))
    add("extract_ridges/n_ridges 0", "extract_ridges", z.w, z.sc, n_ridges=0)
    add("extract_ridges/n_ridges 1.5", "extract_ridges", z.w, z.sc, n_ridges=1.5)
    add("extract_ridges/bw negative", "extract_ridges", z.w, z.sc, bw=-1)
    add("extract_ridges/bw nan", "extract_ridges", z.w, z.sc, bw=NAN)
    return cases


def _degenerate():
    """A draw orthogonal to the admittances of the GMW orders (0, 1): its c_m is rounding error."""
    a0, a1 = up.gmw_adm_ssq(3.0, 60.0, 0), up.gmw_adm_ssq(3.0, 60.0, 1)
    return np.array([[a1, -a0]])


def _kw(fn):
    import inspect
    return tuple(inspect.signature(getattr(up, fn)).parameters)


STFT_KW = {fn: _kw(fn) for fn in STFT_FAMILY}
CWT_KW = {fn: _kw(fn) for fn in CWT_FAMILY}


@functools.lru_cache(maxsize=None)
def tables():
    z = inputs()
    t = SimpleNamespace(accepted=_accepted(z), refusals=_refusals(z))
    assert not set(t.accepted) & set(t.refusals)
    return t


def case_ids():
    t = tables()
    return list(t.accepted) + list(t.refusals)


# --------------------------------------------------------------------------------------------------------- tests ----
@functools.lru_cache(maxsize=None)
def golden():
    """case id -> outcome: the fixture lists the accepted cases one by one and groups the refusals by outcome."""
    with open(GOLDEN) as f:
        z = json.load(f)
    out = dict(z["accepted"])
    for what, cids in z["refused"].items():
        assert not set(cids) & set(out), what
        out.update((cid, what) for cid in cids)
    return out


def test_the_fixture_holds_the_table_and_nothing_else():
    assert sorted(golden()) == sorted(case_ids())


def test_the_header_names_the_outputs():
    outs = host_outputs()
    assert outs["ssq_istft_host"] == (10, [9])
    assert outs["ssq_tssq_cwt_host"] == (19, [15, 16, 17, 18])
    assert outs["ssq_extract_ridges_host"] == (16, [12, 13, 14, 15])
    assert not [n for n in outs if n.startswith("ssq_host_")]
    assert set(outs) <= set(_lib._SIGNATURES)


@pytest.mark.parametrize("cid", case_ids())
def test_record(cid):
    r = record_of(cid)
    assert outcome(r) == golden()[cid], r
