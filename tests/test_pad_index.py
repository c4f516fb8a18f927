"""The pad index map every forward kernel fetches padded samples through (csrc/pad_index.h), evaluated on the host by
`ssq_pad_index`, against np.pad; and the Python tables around it.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib
from tests.helpers import pad_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFLECT, ZERO, SYMMETRIC, REPLICATE, WRAP = range(5)


def _index(code, m, n):
    idx = C.c_int64(12345)
    assert _lib.load().ssq_pad_index(code, m, n, C.byref(idx)) == 0, (code, m, n)
    return idx.value


def _np_index(mode, m, n):
    """Source index of padded position m: np.pad of arange(n) with enough pad on both sides to hold m."""
    left, right = 3 * n + 2, 3 * n + 3
    return int(np.pad(np.arange(n), (left, right), mode=mode)[m + left])


@pytest.mark.parametrize("code,mode", [(SYMMETRIC, "symmetric"), (REPLICATE, "edge"), (WRAP, "wrap")])
def test_new_modes_agree_with_np_pad(code, mode):
    for n in range(1, 10):
        for m in range(-3 * n - 2, 4 * n + 3):
            assert _index(code, m, n) == _np_index(mode, m, n), (mode, n, m)


def test_fold_beyond_the_correction_steps():
    """Far outside the two conditional steps of pad_fold (the reciprocal branch), and at the period's multiples."""
    for n in (1, 2, 7, 1000, (1 << 31) + 5):
        for m in (-(1 << 45) - 3, -(1 << 40), -1000 * n, -5 * n - 1, -5 * n, 5 * n - 1, 5 * n, 1000 * n + 3, (1 << 45) + 11):
            assert _index(WRAP, m, n) == m % n
            r = m % (2 * n)
            assert _index(SYMMETRIC, m, n) == (r if r < n else 2 * n - 1 - r)
            assert _index(REPLICATE, m, n) == min(max(m, 0), n - 1)


def test_reflect_and_zero_keep_the_one_mirror_rule():
    """Codes 0 and 1 as the loaders have always fetched: inside -> itself; reflect -> ONE mirror about the end sample
    (-m on the left, 2n - 2 - m on the right) where that lands inside, zero beyond it; zero -> zero."""
    for n in range(1, 10):
        for m in range(-3 * n - 2, 4 * n + 3):
            inside = 0 <= m < n
            mm = -m if m < 0 else 2 * n - 2 - m
            assert _index(REFLECT, m, n) == (m if inside else mm if 0 <= mm < n else -1), (n, m)
            assert _index(ZERO, m, n) == (m if inside else -1), (n, m)
            if not inside and 0 <= mm < n:                     # and where the mirror holds it is np.pad's 'reflect'
                assert mm == _np_index("reflect", m, n) or n == 1


def test_unknown_code_and_empty_signal_are_errors():
    lib = _lib.load()
    idx = C.c_int64(7)
    for code in (-1, 5, 99):
        assert lib.ssq_pad_index(code, 0, 4, C.byref(idx)) != 0 and idx.value == -1
        assert b"pad type" in lib.ssq_last_error()
    for n in (0, -3):
        assert lib.ssq_pad_index(WRAP, 0, n, C.byref(idx)) != 0
    assert lib.ssq_pad_index(WRAP, 0, 4, None) != 0


def test_python_tables():
    from ssqueeze_rs_amd import upstream as up
    assert [up._pad_code(k) for k in ("reflect", "zero", "symmetric", "replicate", "wrap")] == [0, 1, 2, 3, 4]
    for bad in ("constant", None, "edge", 2):
        with pytest.raises(ValueError) as e:
            up._pad_code(bad)
        assert all(name in str(e.value) for name in ("reflect", "zero", "symmetric", "replicate", "wrap"))
    assert _lib.PAD == {"reflect": 0, "zero": 1}                # the drop-in's table: `.get(padtype, 0)` in _rs / batch


def test_pad_ref_restates_upstream_padsignal():
    """tests/helpers/pad_ref.py against the oracle's padsignal for the two modes that has, upstream's own 'symmetric'
    slicing (utils/common.py:144-149) where a pad fits in one period, and the split of an explicit padlength."""
    from oracle import upstream_oracle as u
    x = np.arange(1.0, 12.0)
    for padlength in (None, 16, 21, 22):
        for mode in ("reflect", "zero"):
            a, b = pad_ref.padsignal(x, mode, padlength), u.padsignal(x, mode, padlength)
            assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
        xp, n_up, n1, n2 = pad_ref.padsignal(x, "symmetric", padlength)
        assert np.array_equal(xp, np.hstack([x[::-1][-n1:], x, x[::-1][:n2]])) and len(xp) == n_up
    assert np.array_equal(pad_ref.padsignal(np.arange(1, 5), "replicate", 11)[0], [1, 1, 1, 1, 1, 2, 3, 4, 4, 4, 4])
    assert np.array_equal(pad_ref.padsignal(np.arange(1, 5), "wrap", 11)[0], [1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3])
    assert pad_ref.padsignal(np.zeros((2, 5)), "wrap")[0].shape == (2, 8)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_pad_index_under_asan_ubsan(tmp_path):
    """The header alone in a stand-alone program (tests/helpers/pad_index_san.cpp), under ASan + UBSan on the CPU."""
    exe = str(tmp_path / "pad_index_san")
    src = os.path.join(ROOT, "tests", "helpers", "pad_index_san.cpp")
    # the sanitizer runtimes are linked statically, so the program runs in whatever environment the suite has
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", src, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    if r.returncode != 0 and "cannot find" in (r.stderr or "") and ("asan" in r.stderr or "ubsan" in r.stderr):
        pytest.skip("static sanitizer runtimes not installed")
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip().endswith("ok")
