"""The two device passes of the chunked front end on their own (csrc/frontend.hip), each against its NumPy statement,
BITWISE (both only move elements):

  ssq_chunk_halo_fill  against `chunked.overlap_extend` (Dask's boundaries: "reflect" repeats the edge sample, anything
                       else pads zeros), fp32 and fp64, at 1 sample, depth = samples, depth = 0, 2 depth = two whole blocks
                       of 256 threads, and three blocks with a ragged last one on an odd channel pitch.  A NaN and a
                       -0.0 sit next to each array end and must come back mirrored as the same bits; the interior stays.
  ssq_chunks_relayout  against the index formula in the comment above `relayout_kernel`, complex64 and complex128, with
                       every window parameter away from its friendly value; the output is prefilled with a sentinel bit
                       pattern that every cell outside the written window must keep.

Every buffer is a `DevBuf` of tests/test_gpu_grid_limits.py (the allocation ends in guard bytes); the guards are read
back after every call.  Refusals return nonzero and write nothing.
"""
import ctypes as C

import numpy as np
import pytest

from ssqueeze_rs_amd import _lib, chunked
from tests.test_gpu_grid_limits import DevBuf

pytestmark = pytest.mark.gpu

RDTS = [np.float32, np.float64]
UINT = {4: np.uint32, 8: np.uint64}


def _code(rdt):
    return _lib.SSQ_F32 if np.dtype(rdt) == np.float32 else _lib.SSQ_F64


def _bits(a):
    """The array as unsigned integers of its real element size: NaN payloads and the sign of zero count."""
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.real.dtype.itemsize])


def _err():
    return _lib.load().ssq_last_error().decode()


class Bufs:
    """DevBufs of one test; every `check()` reads all guards back, leaving frees them."""

    def __init__(self):
        self.bufs = []

    def buf(self, nbytes, src=None):
        self.bufs.append(DevBuf(nbytes, src))
        return self.bufs[-1]

    def check(self):
        _lib.check(_lib.load().ssq_device_sync())
        touched = [i for i, b in enumerate(self.bufs) if not b.guard_untouched()]
        assert not touched, "the guard behind buffer(s) %s was written" % touched

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        try:
            if exc_type is None:
                self.check()
        finally:
            for b in self.bufs:
                b.free()
        return False


# ================================================================================================== halo fill ==========
HALO_SHAPES = [(1, 1, 1), (3, 7, 7), (2, 1000, 0), (2, 513, 256), (5, 1001, 300)]
HALO_FILL = 123.25                       # what the halos hold before the call


def _halo_case(rdt, channels, samples, depth):
    """([channels][depth + samples + depth] host array with HALO_FILL in the halos, the channels as (samples, channels))."""
    rng = np.random.default_rng(1000 * channels + samples + depth)
    x = rng.standard_normal((samples, channels)).astype(rdt)
    if samples >= 7:                     # one NaN and one -0.0 next to each array end
        x[1], x[2], x[-2], x[-3] = np.nan, -0.0, np.nan, -0.0
    else:
        x[0] = -0.0
    ext = np.full((channels, samples + 2 * depth), HALO_FILL, dtype=rdt)
    ext[:, depth:depth + samples] = x.T
    return ext, x


@pytest.mark.parametrize("boundary", ["reflect", "zero"])
@pytest.mark.parametrize("rdt", RDTS, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", HALO_SHAPES, ids=["x".join(map(str, s)) for s in HALO_SHAPES])
def test_halo_fill_equals_overlap_extend(shape, rdt, boundary):
    lib = _lib.load()
    channels, samples, depth = shape
    ext, x = _halo_case(rdt, channels, samples, depth)
    want = np.ascontiguousarray(chunked.overlap_extend(x, depth, boundary).T)
    assert want.shape == ext.shape
    with Bufs() as d:
        b = d.buf(ext.nbytes, ext)
        _lib.check(lib.ssq_chunk_halo_fill(_code(rdt), b.p, channels, samples, depth, 0 if boundary == "reflect" else 1, None))
        d.check()
        got = b.get(ext.shape, rdt)
    assert np.array_equal(_bits(got[:, depth:depth + samples]), _bits(ext[:, depth:depth + samples])), "interior written"
    if depth == 0:
        assert np.array_equal(_bits(got), _bits(ext))            # a no-op, bit for bit
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, "(channel, position) %s differ from overlap_extend" % bad[:8].tolist()
    if boundary == "reflect" and samples >= 7 and depth >= 3:
        # the NaN and the -0.0 themselves, where Dask's reflect puts them: position -m holds x[m - 1]
        assert np.isnan(got[:, depth - 2]).all() and np.array_equal(_bits(got[:, depth - 3]), _bits(x[2]))
        assert np.isnan(got[:, depth + samples + 1]).all()
        assert np.array_equal(_bits(got[:, depth + samples + 2]), _bits(x[-3]))


@pytest.mark.parametrize("rdt", RDTS, ids=["f32", "f64"])
def test_halo_fill_refusals_write_nothing(rdt):
    lib = _lib.load()
    channels, samples, depth = 2, 9, 4
    ext, _ = _halo_case(rdt, channels, samples, depth)
    code = _code(rdt)
    with Bufs() as d:
        b = d.buf(ext.nbytes, ext)
        for args, msg in (((code, b.p, channels, samples, samples + 1, 0, None), "overlap depth larger"),
                          ((code, b.p, channels, samples, -1, 0, None), "bad shape"),
                          ((code, b.p, 0, samples, depth, 0, None), "bad shape"),
                          ((code, b.p, -3, samples, depth, 0, None), "bad shape"),
                          ((7, b.p, channels, samples, depth, 0, None), "dtype must be"),
                          ((code, None, channels, samples, depth, 0, None), "NULL")):
            assert lib.ssq_chunk_halo_fill(*args) != 0, args
            assert msg in _err(), (args, _err())
            d.check()
            assert np.array_equal(_bits(b.get(ext.shape, rdt)), _bits(ext)), args


# =================================================================================================== relayout ==========
def _relayout_ref(inp, col0, ncols, out, out_col_base, ch_base):
    """out[(r*out_cols + out_col_base + j*ncols + c)*out_channels + ch_base + ch] = in[((ch*chunks + j)*rows + r)*cols_in + col0 + c]
    for inp [channels][chunks][rows][cols_in] and out [rows][out_cols][out_channels], written in place."""
    channels, chunks, rows, cols_in = inp.shape
    for ch in range(channels):
        for j in range(chunks):
            out[:, out_col_base + j * ncols:out_col_base + (j + 1) * ncols, ch_base + ch] = inp[ch, j, :, col0:col0 + ncols]
    return out


def _sentinel(shape, cdt):
    """What DevBuf fills a fresh allocation with, as an array: 0xA5 in every byte."""
    return np.full(int(np.prod(shape)) * np.dtype(cdt).itemsize, 0xA5, dtype=np.uint8).view(cdt).reshape(shape)


def _relayout_input(cdt, channels, chunks, rows, cols_in, seed):
    rng = np.random.default_rng(seed)
    rdt = np.float32 if cdt == np.complex64 else np.float64
    a = rng.standard_normal((channels, chunks, rows, cols_in, 2)).astype(rdt)
    return np.ascontiguousarray(a).view(cdt)[..., 0]


# (channels, chunks, rows, cols_in, col0, ncols, out_cols, out_col_base, out_channels, ch_base)
RELAYOUT_CASES = {
    "255-elements": (3, 2, 2, 90, 5, 85, 2 * 85, 0, 3, 0),                    # ncols * channels = 255: one ragged block
    "256-elements": (4, 2, 3, 64, 0, 64, 2 * 64, 0, 4, 0),                    # = 256: one whole block
    "258-elements": (3, 2, 2, 86, 0, 86, 2 * 86, 0, 3, 0),                    # = 258: a block edge inside a column
    "1285-elements": (5, 3, 2, 300, 43, 257, 3 * 257 + 9, 4, 5, 0),           # six blocks, 256 no multiple of 5
    "col0-to-the-end": (3, 2, 3, 40, 9, 31, 2 * 31, 0, 3, 0),                 # col0 > 0, col0 + ncols == cols_in
    "out-col-base": (2, 3, 2, 20, 3, 11, 3 * 11 + 12, 5, 2, 0),               # columns in front and behind stay
    "ch-base": (2, 2, 3, 17, 1, 13, 2 * 13, 0, 7, 3),                         # channels in front and behind stay
    "one-row": (3, 4, 1, 33, 2, 29, 4 * 29 + 1, 1, 4, 1),
    "one-chunk": (3, 1, 5, 33, 0, 33, 33 + 2, 2, 3, 0),
    "all-at-once": (5, 3, 4, 77, 6, 70, 3 * 70 + 8, 3, 9, 2),
}


def _run_relayout(lib, cdt, inp, col0, ncols, out_shape, out_col_base, ch_base, d, dout=None):
    channels, chunks, rows, cols_in = inp.shape
    din = d.buf(inp.nbytes, np.ascontiguousarray(inp))
    if dout is None:
        dout = d.buf(int(np.prod(out_shape)) * np.dtype(cdt).itemsize)
    code = _lib.SSQ_F32 if cdt == np.complex64 else _lib.SSQ_F64
    _lib.check(lib.ssq_chunks_relayout(code, din.p, channels, chunks, rows, cols_in, col0, ncols, dout.p, out_shape[1],
                                       out_col_base, out_shape[2], ch_base, None))
    d.check()
    return dout


@pytest.mark.parametrize("cdt", [np.complex64, np.complex128], ids=["c64", "c128"])
@pytest.mark.parametrize("case", list(RELAYOUT_CASES))
def test_relayout_equals_its_index_formula(case, cdt):
    lib = _lib.load()
    channels, chunks, rows, cols_in, col0, ncols, out_cols, out_col_base, out_channels, ch_base = RELAYOUT_CASES[case]
    inp = _relayout_input(cdt, channels, chunks, rows, cols_in, len(case))
    shape = (rows, out_cols, out_channels)
    want = _relayout_ref(inp, col0, ncols, _sentinel(shape, cdt), out_col_base, ch_base)
    with Bufs() as d:
        got = _run_relayout(lib, cdt, inp, col0, ncols, shape, out_col_base, ch_base, d).get(shape, cdt)
    written = _bits(want) != _bits(_sentinel(shape, cdt))
    assert written.sum() == 2 * rows * chunks * ncols * channels             # (no random value is the sentinel)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, "%s: cells (row, column, 2 channel + re/im) %s differ" % (case, bad[:8].tolist())


@pytest.mark.parametrize("cdt", [np.complex64, np.complex128], ids=["c64", "c128"])
def test_relayout_by_channel_groups_equals_one_call(cdt):
    """Channel groups [0, 2) and [2, 5) of one output, each from its own call, against all five channels at once."""
    lib = _lib.load()
    channels, chunks, rows, cols_in, col0, ncols, out_col_base = 5, 3, 4, 50, 7, 41, 2
    shape = (rows, chunks * ncols + 5, channels)
    inp = _relayout_input(cdt, channels, chunks, rows, cols_in, 99)
    with Bufs() as d:
        one = _run_relayout(lib, cdt, inp, col0, ncols, shape, out_col_base, 0, d).get(shape, cdt)
        dout = _run_relayout(lib, cdt, inp[:2], col0, ncols, shape, out_col_base, 0, d)
        half = dout.get(shape, cdt)
        two = _run_relayout(lib, cdt, inp[2:], col0, ncols, shape, out_col_base, 2, d, dout).get(shape, cdt)
    assert np.array_equal(_bits(one), _bits(_relayout_ref(inp, col0, ncols, _sentinel(shape, cdt), out_col_base, 0)))
    assert np.array_equal(_bits(half), _bits(_relayout_ref(inp[:2], col0, ncols, _sentinel(shape, cdt), out_col_base, 0)))
    assert np.array_equal(_bits(two), _bits(one))


@pytest.mark.parametrize("cdt", [np.complex64, np.complex128], ids=["c64", "c128"])
def test_relayout_range_refusals_write_nothing(cdt):
    lib = _lib.load()
    code = _lib.SSQ_F32 if cdt == np.complex64 else _lib.SSQ_F64
    channels, chunks, rows, cols_in, col0, ncols, out_cols, out_col_base, out_channels, ch_base = 2, 3, 2, 20, 3, 11, 40, 5, 4, 1
    inp = _relayout_input(cdt, channels, chunks, rows, cols_in, 5)
    shape = (rows, out_cols, out_channels)
    ok = dict(col0=col0, ncols=ncols, out_cols=out_cols, out_col_base=out_col_base, out_channels=out_channels, ch_base=ch_base)
    bad = [dict(col0=-1), dict(col0=cols_in - ncols + 1), dict(ch_base=-1), dict(ch_base=out_channels - channels + 1),
           dict(out_col_base=-1), dict(out_col_base=out_cols - chunks * ncols + 1), dict(out_cols=chunks * ncols + out_col_base - 1),
           dict(out_channels=channels + ch_base - 1)]
    with Bufs() as d:
        din, dout = d.buf(inp.nbytes, inp), d.buf(int(np.prod(shape)) * np.dtype(cdt).itemsize)
        for change in bad:
            a = dict(ok, **change)
            rc = lib.ssq_chunks_relayout(code, din.p, channels, chunks, rows, cols_in, a["col0"], a["ncols"], dout.p,
                                         a["out_cols"], a["out_col_base"], a["out_channels"], a["ch_base"], None)
            assert rc != 0 and "relayout window out of range" in _err(), (change, _err())
            d.check()
            assert np.array_equal(_bits(dout.get(shape, cdt)), _bits(_sentinel(shape, cdt))), change
        # and the window itself is accepted
        _lib.check(lib.ssq_chunks_relayout(code, din.p, channels, chunks, rows, cols_in, col0, ncols, dout.p, out_cols,
                                           out_col_base, out_channels, ch_base, None))
        d.check()
        want = _relayout_ref(inp, col0, ncols, _sentinel(shape, cdt), out_col_base, ch_base)
        assert np.array_equal(_bits(dout.get(shape, cdt)), _bits(want))
