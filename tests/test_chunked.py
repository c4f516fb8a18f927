"""The chunked-overlap multi-channel front end (ssqueeze_rs_amd/chunked.py) against the
reference harness' behaviour restated chunk by chunk: extend every chunk by `depth` samples (neighbours inside the
array, Dask's "reflect" at its ends), run the reference API call per channel on the extended chunk, stack as
(freq, frames, channels), concatenate the chunks (tests/stft_ssq_test.py:216-281, tests/ssq_cwt_test.py:116-192).
"""
import numpy as np
import pytest

from oracle import ssq_oracle as o
from ssqueeze_rs_amd import chunked


# ------------------------------------------------------------------------------------------ host logic (CPU) ----
def test_chunk_plan_and_overlap_extend():
    assert chunked.chunk_plan(10, 4) == [(0, 4), (4, 4), (8, 2)]
    assert chunked.chunk_plan(8, 4) == [(0, 4), (4, 4)]
    assert chunked.chunk_plan(3, 10) == [(0, 3)]
    with pytest.raises(ValueError):
        chunked.chunk_plan(0, 4)
    x = np.arange(10.0)
    e = chunked.overlap_extend(x, 3, "reflect")              # dask reflect: the edge sample is repeated
    assert np.array_equal(e, [2, 1, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 8, 7])
    z = chunked.overlap_extend(x, 2, "zero")
    assert np.array_equal(z, [0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0, 0])
    x2 = np.arange(12.0).reshape(6, 2)
    e2 = chunked.overlap_extend(x2, 2, "reflect")
    assert e2.shape == (10, 2) and np.array_equal(e2[:2, 0], [2, 0]) and np.array_equal(e2[-2:, 1], [11, 9])
    with pytest.raises(ValueError):
        chunked.overlap_extend(x, 11)


def test_kept_columns():
    # depth 1024, chunk 4096, hop 256: extended chunk 6144 samples -> 24 frames; frames 4..19 start inside the chunk
    assert chunked._kept("none", 1024, 4096, 256, 24) == (0, 24)
    assert chunked._kept("halo", 1024, 4096, 256, 24) == (4, 16)
    assert chunked._kept("halo", 1000, 4096, 256, 24) == (4, 16)       # frame starts 1024..4864 < 5096
    assert chunked._kept("halo", 5, 10, 1, 20) == (5, 10)
    with pytest.raises(ValueError):
        chunked._kept("frames", 1, 1, 1, 1)


# --------------------------------------------------------------------------------------------------- GPU ----
def _reference_harness_stft(x_sc, chunk, depth, fn):
    """process_chunk over map_overlap, restated: x_sc is (samples, channels); fn(channel_1d) -> (K, F)."""
    ext = chunked.overlap_extend(x_sc, depth, "reflect")
    outs = []
    for start, L in chunked.chunk_plan(x_sc.shape[0], chunk):
        xe = ext[start:start + L + 2 * depth]
        stacked = np.stack([fn(np.ascontiguousarray(xe[:, ch])) for ch in range(x_sc.shape[1])])
        outs.append(np.transpose(stacked, (1, 2, 0)))
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_process_stft_ssq_equals_the_per_channel_per_chunk_loop(dtype):
    from ssqueeze_rs_amd import _rs
    S, Cn, chunk, n_fft, hop, fs = 23000, 3, 8192, 256, 64, 24414.0625
    x = np.stack([o.synth_signal(S, 60 + c, dtype) for c in range(Cn)], axis=1)         # (samples, channels)
    win = np.hanning(n_fft)
    got = chunked.process_stft_ssq(x, fs=fs, n_fft=n_fft, hop_length=hop, chunk=chunk, dtype=dtype)
    parts = _reference_harness_stft(x, chunk, n_fft, lambda c: _rs.ssq_stft(
        c, win, n_fft=n_fft, win_len=n_fft, hop_len=hop, fs=fs, padtype="reflect", squeezing="sum")[0])
    want = np.concatenate(parts, axis=1)
    assert got.shape == want.shape == (129, sum(p.shape[1] for p in parts), Cn)
    assert got.dtype == (np.complex128 if dtype == np.float64 else np.complex64)
    assert np.array_equal(got, want)                     # same kernels, same windows of samples: bitwise
    # and the loop itself against the oracle on the middle chunk of channel 1 (fp64: the reference's arithmetic)
    if dtype == np.float64:
        ext = chunked.overlap_extend(x, n_fft, "reflect")
        xe = np.ascontiguousarray(ext[chunk:chunk + chunk + 2 * n_fft, 1])
        Tx_o, _ = o.ssq_stft(xe, win, n_fft=n_fft, win_len=n_fft, hop_len=hop, fs=fs)
        mid = parts[1][:, :, 1]
        assert np.abs(mid.sum(0) - Tx_o.sum(0)).max() <= 1e-9 * np.abs(Tx_o).max()
        assert (np.abs(mid - Tx_o) > 1e-9 * np.abs(Tx_o).max()).mean() <= 1e-3
    # plain stft through the same front end
    got_s = chunked.process_stft(x, n_fft=n_fft, hop_length=hop, chunk=chunk, dtype=dtype)
    parts_s = _reference_harness_stft(x, chunk, n_fft, lambda c: _rs.stft(c, n_fft, hop, win, "reflect")[0])
    assert np.array_equal(got_s, np.concatenate(parts_s, axis=1))


@pytest.mark.gpu
def test_halo_trim_removes_the_seams():
    """trim="halo": away from the two array ends the concatenation IS the whole-signal transform (bitwise: every kept
    frame reads only real samples); at the ends the Dask halo (edge sample repeated) differs from ssq_stft's own
    reflect padding -- the harness' behaviour, kept."""
    from ssqueeze_rs_amd import _rs
    S, chunk, n_fft, hop = 40960, 8192, 1024, 256
    x = o.synth_signal(S, 70, np.float32)
    got = chunked.process_stft_ssq(x, fs=1.0, n_fft=n_fft, hop_length=hop, chunk=chunk, trim="halo", dtype=np.float32)
    whole, _ = _rs.ssq_stft(x, np.hanning(n_fft), n_fft=n_fft, win_len=n_fft, hop_len=hop, fs=1.0)
    assert got.shape == (513, S // hop, 1) and whole.shape == (513, S // hop)
    edge = (n_fft // 2) // hop + 1
    assert np.array_equal(got[:, edge:-edge, 0], whole[:, edge:-edge])
    assert not np.array_equal(got[:, :edge, 0], whole[:, :edge])
    # every interior chunk seam lies inside the compared range
    assert edge < chunk // hop < S // hop - edge


@pytest.mark.gpu
def test_process_ssq_cwt_and_cwt_equal_the_loop():
    from ssqueeze_rs_amd import _rs
    S, Cn, chunk, fs = 9000, 2, 4000, 1000.0
    x = np.stack([o.synth_signal(S, 80 + c) for c in range(Cn)], axis=1)
    scales = np.logspace(1, 5, 32) / fs                   # tests/ssq_cwt_test.py:24
    depth = max(1024, S // 10)
    got, f = chunked.process_ssq_cwt(x, fs=fs, wavelet="gmw", scales=scales, nv=16, chunk=chunk)
    ext = chunked.overlap_extend(x, depth, "reflect")
    parts = []
    for start, L in chunked.chunk_plan(S, chunk):
        xe = ext[start:start + L + 2 * depth]
        parts.append(np.transpose(np.stack([_rs.ssq_cwt(np.ascontiguousarray(xe[:, ch]), wavelet="gmw", scales=scales,
                                                        fs=fs, nv=16)[0] for ch in range(Cn)]), (1, 2, 0)))
    want = np.concatenate(parts, axis=1)
    assert got.shape == want.shape == (32, S + 2 * depth * len(parts), Cn)
    assert np.array_equal(got, want)
    _, f_one = _rs.ssq_cwt(np.ascontiguousarray(ext[:chunk + 2 * depth, 0]), wavelet="gmw", scales=scales, fs=fs, nv=16)
    assert np.array_equal(f, f_one)
    Wx, sc, dWx = chunked.process_cwt(x, fs=fs, wavelet="morlet", scales=scales, chunk=chunk, trim="halo")
    assert Wx.shape == dWx.shape == (32, S, Cn) and np.array_equal(sc, scales)
    xe = np.ascontiguousarray(ext[chunk:chunk + chunk + 2 * depth, 1])
    W1, _, dW1 = _rs.cwt(xe, wavelet="morlet", scales=scales, fs=fs, derivative=True)
    assert np.array_equal(Wx[:, chunk:2 * chunk, 1], W1[:, depth:depth + chunk])
    assert np.array_equal(dWx[:, chunk:2 * chunk, 1], dW1[:, depth:depth + chunk])


# ------------------------------------------------------------------------------- more host logic (CPU) ----------
def test_halo_trim_keeps_exactly_the_whole_signal_grid():
    """trim="halo" with depth and chunk multiples of the hop: over all chunks the kept columns, as array positions
    start - depth + c hop, are range(0, S, hop) -- every frame of the whole-signal grid once, in order.  And for ANY depth
    (the second property) a chunk keeps exactly the columns of its own grid that lie inside the chunk proper."""
    rng = np.random.default_rng(20261020)
    for _ in range(20000):
        hop, a, b = int(rng.integers(1, 10)), int(rng.integers(0, 7)), int(rng.integers(1, 13))
        depth, chunk = hop * a, hop * b
        S = int(rng.integers(max(depth, 1), 201))
        pos = []
        for start, L in chunked.chunk_plan(S, chunk):
            n_out = (L + 2 * depth - 1) // hop + 1
            f0, nf = chunked._kept("halo", depth, L, hop, n_out)
            pos.extend(start - depth + c * hop for c in range(f0, f0 + nf))
        assert pos == list(range(0, S, hop)), (hop, depth, chunk, S)
    for _ in range(2000):
        hop, depth, L = int(rng.integers(1, 10)), int(rng.integers(0, 40)), int(rng.integers(1, 60))
        n_out = (L + 2 * depth - 1) // hop + 1
        f0, nf = chunked._kept("halo", depth, L, hop, n_out)
        assert list(range(f0, f0 + nf)) == [c for c in range(n_out) if depth <= c * hop < depth + L], (hop, depth, L)


def test_overlap_extend_at_its_edges():
    x = np.arange(1.0, 6.0)
    assert np.array_equal(chunked.overlap_extend(x, 5, "reflect"), [5, 4, 3, 2, 1, 1, 2, 3, 4, 5, 5, 4, 3, 2, 1])   # depth = S
    assert np.array_equal(chunked.overlap_extend(x, 5, "zero"), [0] * 5 + [1, 2, 3, 4, 5] + [0] * 5)
    e0 = chunked.overlap_extend(x, 0, "reflect")
    assert np.array_equal(e0, x) and e0 is not x and not np.shares_memory(e0, x)                # depth = 0: a copy
    with pytest.raises(ValueError, match="larger than the array"):
        chunked.overlap_extend(x, 6)                                                           # depth = S + 1
    x2 = np.arange(12.0).reshape(4, 3)                                                          # (samples, channels)
    e2 = chunked.overlap_extend(x2, 4, "reflect")
    assert e2.shape == (12, 3) and e2.dtype == x2.dtype
    for ch in range(3):
        assert np.array_equal(e2[:, ch], chunked.overlap_extend(x2[:, ch], 4, "reflect"))
    z2 = chunked.overlap_extend(x2.astype(np.float32), 3, "zero")
    assert z2.dtype == np.float32 and z2.shape == (10, 3)
    assert not z2[:3].any() and not z2[-3:].any() and np.array_equal(z2[3:7], x2)
    with pytest.raises(ValueError):
        chunked.overlap_extend(x2, 5)


def test_as_channels():
    one = chunked._as_channels(np.arange(5), np.float32)
    assert one.shape == (1, 5) and one.dtype == np.float32 and one.flags.c_contiguous      # 1-D: one channel
    sc = np.arange(12, dtype=np.int64).reshape(4, 3)[:, ::-1]                                # (samples, channels), a view
    for dt in (np.float32, np.float64):
        a = chunked._as_channels(sc, dt)
        assert a.shape == (3, 4) and a.dtype == dt and a.flags.c_contiguous and np.array_equal(a, sc.T)
    with pytest.raises(ValueError, match="1D or 2D"):
        chunked._as_channels(np.zeros((2, 3, 4)), np.float64)


def test_missing_fs_is_refused_before_any_gpu_call():
    """The three entry points whose reference function raises on fs=None (stft_ssq_test.py:197-198, ssq_cwt_test.py:104-105,
    cwt_test.py) do so before they touch the library: this holds on a machine without a GPU."""
    x = np.zeros((100, 2))
    for fn in (chunked.process_stft_ssq, chunked.process_ssq_cwt, chunked.process_cwt):
        with pytest.raises(ValueError, match=r"Sampling frequency \(fs\) must be provided"):
            fn(x)
        with pytest.raises(ValueError, match=r"Sampling frequency \(fs\) must be provided"):
            fn(x, fs=None, chunk=50)


# ------------------------------------------------------------------------------ GPU: ragged shapes, every route ----
import ctypes as C  # noqa: E402

from ssqueeze_rs_amd import _lib  # noqa: E402

F32, F64 = np.float32, np.float64
DT_IDS = {F32: "f32", F64: "f64"}
UINT = {4: np.uint32, 8: np.uint64}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.real.dtype.itemsize])


def _route(dtype, n_ext, n_fft, hop, kind):
    """The route of the plan `_stft_family` creates for extended chunks of n_ext samples (ssq_stft_plan_route)."""
    lib = _lib.load()
    win = np.ascontiguousarray(chunked._window("hann", n_fft), dtype=np.float64)
    plan, r = C.c_void_p(), C.c_int(-1)
    _lib.check(lib.ssq_stft_plan_create(C.byref(plan), _lib.SSQ_F32 if dtype == F32 else _lib.SSQ_F64, n_ext,
                                        win.ctypes.data_as(C.c_void_p), n_fft, hop, 1.0, 0, 0, -1.0, 0))
    try:
        _lib.check(lib.ssq_stft_plan_route(plan, kind, C.byref(r)))
    finally:
        lib.ssq_stft_plan_destroy(plan)
    return _lib.STFT_ROUTES[r.value]


def _channels(S, Cn, dtype, seed):
    return np.stack([o.synth_signal(S, seed + c, dtype) for c in range(Cn)], axis=1)         # (samples, channels)


def _stft_loops(x_sc, chunk, depth, n_fft, hop, fs):
    """(Tx parts, Sx parts) of the reference harness: a loop of `_rs.*` calls over `overlap_extend`."""
    from ssqueeze_rs_amd import _rs
    win = np.hanning(n_fft)
    tx = _reference_harness_stft(x_sc, chunk, depth, lambda c: _rs.ssq_stft(
        c, win, n_fft=n_fft, win_len=n_fft, hop_len=hop, fs=fs, padtype="reflect", squeezing="sum")[0])
    sx = _reference_harness_stft(x_sc, chunk, depth, lambda c: _rs.stft(c, n_fft, hop, win, "reflect")[0])
    return tx, sx


def _assert_stft_family_equals_the_loops(x, chunk, depth, n_fft, hop, dtype, fs=1.0, **kw):
    x_sc = x.reshape(-1, 1) if x.ndim == 1 else x
    d = n_fft if depth is None else depth
    tx, sx = _stft_loops(x_sc, chunk, d, n_fft, hop, fs)
    got_t = chunked.process_stft_ssq(x, fs=fs, n_fft=n_fft, hop_length=hop, chunk=chunk, depth=depth, dtype=dtype, **kw)
    got_s = chunked.process_stft(x, fs=fs, n_fft=n_fft, hop_length=hop, chunk=chunk, depth=depth, dtype=dtype, **kw)
    for got, parts, name in ((got_t, tx, "ssq_stft"), (got_s, sx, "stft")):
        want = np.concatenate(parts, axis=1)
        assert got.shape == want.shape == (n_fft // 2 + 1, sum(p.shape[1] for p in parts), x_sc.shape[1]), name
        assert got.dtype == want.dtype == (np.complex64 if dtype == F32 else np.complex128), name
        bad = np.argwhere((_bits(got) != _bits(want)).any(axis=(0, 2)))
        assert bad.size == 0, "%s: output columns %s differ from the loop" % (name, bad[:8].ravel().tolist())
    return got_t, got_s


STFT_ROUTE = {16: ("DFT", "DFT"), 17: ("DFT", "DFT"), 48: ("MIXED_RADIX", "MIXED_RADIX"), 64: ("FUSED_POW2", "FUSED_POW2"),
              333: ("BLUESTEIN", "BLUESTEIN"), 1000: ("MIXED_RADIX", "MIXED_RADIX")}          # (Tx, Sx)


def _expected_routes(n_fft, dtype):
    if n_fft == 1024:
        return ("TX1024", "FUSED_POW2") if dtype == F32 else ("FUSED_SPLIT", "FUSED_SPLIT")
    return STFT_ROUTE[n_fft]


def _assert_routes(tag, dtype, n_fft, hop, lengths):
    for n_ext in sorted(set(lengths)):
        r = (_route(dtype, n_ext, n_fft, hop, _lib.OUT_TX), _route(dtype, n_ext, n_fft, hop, _lib.OUT_SX))
        print(f"CHUNKED {tag}: n_ext={n_ext} route(Tx, Sx)={r}")
        assert r == _expected_routes(n_fft, dtype), (tag, n_ext, r)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("n_fft", [17, 48, 64, 333, 1000, 1024])
def test_process_stft_family_on_every_route(n_fft, dtype):
    """3 channels, S = 3 chunk + r with a last chunk shorter than the depth and a chunk that is no multiple of the hop:
    ALL of the output bitwise against the loop; fp64: every (channel, chunk) part of the loop against the oracle."""
    from tests.test_gpu_stft import _check_ssq_f64
    hop, Cn = max(1, n_fft // 4), 3
    chunk, r = 3 * n_fft + 7, n_fft // 2 + 3
    S = 3 * chunk + r
    assert chunk % hop != 0 and r < n_fft
    x = _channels(S, Cn, dtype, 60)
    _assert_routes(f"n_fft={n_fft} {DT_IDS[dtype]}", dtype, n_fft, hop, [L + 2 * n_fft for _, L in chunked.chunk_plan(S, chunk)])
    _assert_stft_family_equals_the_loops(x, chunk, None, n_fft, hop, dtype)
    if dtype == F64:
        ext = chunked.overlap_extend(x, n_fft, "reflect")
        for start, L in chunked.chunk_plan(S, chunk):
            for ch in range(Cn):
                _check_ssq_f64(np.ascontiguousarray(ext[start:start + L + 2 * n_fft, ch]), np.hanning(n_fft), n_fft, hop, 1.0,
                               "reflect", "sum")


def _geometries(n_fft):
    """name -> (S, chunk, depth, 1-D input)."""
    hop = n_fft // 4
    return {
        "prime-S": (1009 if n_fft == 64 else 10007, 5 * n_fft, None, False),
        "chunk-no-multiple-of-hop": (13 * n_fft + 5, 4 * n_fft + hop // 2 + 1, None, False),
        "odd-depth": (9 * n_fft + 11, 4 * n_fft, n_fft + 1, False),
        "last-chunk-shorter-than-depth": (8 * n_fft + 5, 4 * n_fft, None, False),
        "one-chunk": (3 * n_fft + 1, 7 * n_fft, None, False),                # S < chunk
        "depth-0": (10 * n_fft + n_fft // 2 + 3, 4 * n_fft, 0, False),
        "depth-S": (3 * n_fft + 1, 3 * n_fft + 1, 3 * n_fft + 1, False),
        "1-D": (9 * n_fft + 3, 4 * n_fft, None, True),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("n_fft", [64, 1024])
@pytest.mark.parametrize("geometry", list(_geometries(64)))
def test_process_stft_family_ragged_geometry(geometry, n_fft, dtype):
    S, chunk, depth, one_d = _geometries(n_fft)[geometry]
    hop = n_fft // 4
    plan = chunked.chunk_plan(S, chunk)
    d = n_fft if depth is None else depth
    if geometry == "prime-S":
        assert all(S % q for q in range(2, int(S ** 0.5) + 1))
    if geometry == "last-chunk-shorter-than-depth":
        assert plan[-1][1] < d
    if geometry in ("one-chunk", "depth-S"):
        assert len(plan) == 1
    x = o.synth_signal(S, 75, dtype) if one_d else _channels(S, 2, dtype, 70)
    _assert_routes(f"{geometry} n_fft={n_fft} {DT_IDS[dtype]}", dtype, n_fft, hop, [L + 2 * d for _, L in plan])
    got_t, _ = _assert_stft_family_equals_the_loops(x, chunk, depth, n_fft, hop, dtype)
    assert got_t.shape[2] == (1 if one_d else 2)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("slab", [1, 2])
def test_stft_slab_split_equals_the_unlimited_run(slab, dtype):
    """temp_bytes small enough for `slab` of the 3 full chunks per strided batch: several batches and relayouts per plan,
    each placed by the window pointer and `col_base` of its first chunk."""
    n_fft, hop, Cn, chunk = 64, 16, 3, 300
    S = 3 * chunk + 41
    x = _channels(S, Cn, dtype, 90)
    K, F = n_fft // 2 + 1, (chunk + 2 * n_fft - 1) // hop + 1
    per = Cn * K * F * 2 * np.dtype(dtype).itemsize
    _assert_routes(f"slab={slab} {DT_IDS[dtype]}", dtype, n_fft, hop, [L + 2 * n_fft for _, L in chunked.chunk_plan(S, chunk)])
    for fn in (chunked.process_stft_ssq, chunked.process_stft):
        whole = fn(x, fs=1.0, n_fft=n_fft, hop_length=hop, chunk=chunk, dtype=dtype)
        cut = fn(x, fs=1.0, n_fft=n_fft, hop_length=hop, chunk=chunk, dtype=dtype, temp_bytes=slab * per + per // 2)
        assert np.array_equal(_bits(cut), _bits(whole)), fn.__name__
    _assert_stft_family_equals_the_loops(x, chunk, None, n_fft, hop, dtype, temp_bytes=slab * per)


@pytest.mark.gpu
def test_more_equal_chunks_than_one_relayout_launch_takes():
    """65540 equal chunks of 16 samples (one channel, n_fft = 16, depth 16, hop 4): `ssq_chunks_relayout` takes at most
    65535 chunks a launch, so the run goes as two slabs.  64 chunks -- the first, the last, both sides of chunk 65535 and
    others drawn with a fixed seed -- against the loop."""
    from ssqueeze_rs_amd import _rs
    n_fft, hop, chunk, depth, n_chunks = 16, 4, 16, 16, 65540
    S = n_chunks * chunk
    x = np.random.default_rng(16).standard_normal((S, 1)).astype(F32)
    _assert_routes("65540 chunks", F32, n_fft, hop, [chunk + 2 * depth])
    got = chunked.process_stft_ssq(x, fs=1.0, n_fft=n_fft, hop_length=hop, chunk=chunk, depth=depth, dtype=F32)
    F = (chunk + 2 * depth - 1) // hop + 1
    assert got.shape == (9, n_chunks * F, 1) and got.dtype == np.complex64
    rng = np.random.default_rng(65535)
    picks = sorted({0, 1, 65533, 65534, 65535, 65536, n_chunks - 2, n_chunks - 1} | set(rng.integers(0, n_chunks, 56).tolist()))
    ext = chunked.overlap_extend(x, depth, "reflect")
    win = np.hanning(n_fft)
    for j in picks:
        xe = np.ascontiguousarray(ext[j * chunk:j * chunk + chunk + 2 * depth, 0])
        want = _rs.ssq_stft(xe, win, n_fft=n_fft, win_len=n_fft, hop_len=hop, fs=1.0, padtype="reflect", squeezing="sum")[0]
        assert np.array_equal(_bits(got[:, j * F:(j + 1) * F, 0]), _bits(want)), "chunk %d" % j


HALO_CASES = [(F64, 64, 16, 40 * 16, 3 * 40 * 16 + 87), (F32, 1000, 250, 6000, 3 * 6000 + 2777),
              (F32, 1024, 256, 8192, 4 * 8192 + 3001)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,n_fft,hop,chunk,S", HALO_CASES, ids=["f64-64", "f32-1000", "f32-1024"])
def test_halo_trim_equals_the_whole_signal_wherever_a_frame_lies_inside(dtype, n_fft, hop, chunk, S):
    """Every output column whose frame [s - (n_fft-1)//2, s - (n_fft-1)//2 + n_fft) lies inside [0, S) -- the exact mask,
    not an edge count -- is bitwise the whole-signal transform's column, chunk seams included."""
    from ssqueeze_rs_amd import _rs
    assert S % chunk != 0 and chunk % hop == 0 and n_fft % hop == 0
    x = o.synth_signal(S, 71, dtype)
    _assert_routes(f"halo n_fft={n_fft} {DT_IDS[dtype]}", dtype, n_fft, hop, [L + 2 * n_fft for _, L in chunked.chunk_plan(S, chunk)])
    got = chunked.process_stft_ssq(x, fs=1.0, n_fft=n_fft, hop_length=hop, chunk=chunk, trim="halo", dtype=dtype)
    whole, _ = _rs.ssq_stft(x, np.hanning(n_fft), n_fft=n_fft, win_len=n_fft, hop_len=hop, fs=1.0)
    n_cols = (S - 1) // hop + 1
    assert got.shape == (n_fft // 2 + 1, n_cols, 1) and whole.shape == got.shape[:2]
    lo = np.arange(n_cols) * hop - (n_fft - 1) // 2
    inside = (lo >= 0) & (lo + n_fft <= S)
    seams = [j * chunk // hop for j in range(1, len(chunked.chunk_plan(S, chunk)))]
    assert seams and all(inside[c - 1] and inside[c] for c in seams)
    bad = np.flatnonzero(inside & (_bits(got[:, :, 0]) != _bits(whole)).reshape(got.shape[0], n_cols, 2).any(axis=(0, 2)))
    assert bad.size == 0, "columns %s (seams at %s) differ from the whole-signal transform" % (bad[:8].tolist(), seams)
    assert not np.array_equal(got[:, 0, 0], whole[:, 0])          # the array ends are Dask's halo, not ssq_stft's padding


# ------------------------------------------------------------------------------------------- GPU: CWT family ----
CWT_FS = 1000.0
CWT_SCALES = np.logspace(1, 4, 16) / CWT_FS
CWT_S, CWT_CHUNK, CWT_DEPTH = 3001, 1201, 301


def _cwt_loop(x_sc, chunk, depth, boundary, fn):
    """[(start, L, (outputs of fn(channel) stacked as (rows, time, channels)))] over the extended chunks."""
    ext = chunked.overlap_extend(x_sc, depth, boundary)
    parts = []
    for start, L in chunked.chunk_plan(x_sc.shape[0], chunk):
        xe = ext[start:start + L + 2 * depth]
        per_ch = [fn(np.ascontiguousarray(xe[:, ch])) for ch in range(x_sc.shape[1])]
        parts.append((start, L, [None if per_ch[0][i] is None else np.transpose(np.stack([p[i] for p in per_ch]), (1, 2, 0))
                                 for i in range(len(per_ch[0]))]))
    return parts


def _ssq_cwt(c, **kw):
    from ssqueeze_rs_amd import _rs
    return (_rs.ssq_cwt(c, **kw)[0],)


def _cwt(c, **kw):
    from ssqueeze_rs_amd import _rs
    Wx, _, dWx = _rs.cwt(c, **kw)
    return Wx, dWx


def _first_window_freqs(x, boundary="reflect", **kw):
    """ssq_freqs of `_rs.ssq_cwt` on the first extended chunk of channel 0: what the front end returns."""
    from ssqueeze_rs_amd import _rs
    xe = chunked.overlap_extend(x, CWT_DEPTH, boundary)[:CWT_CHUNK + 2 * CWT_DEPTH, 0]
    return _rs.ssq_cwt(np.ascontiguousarray(xe), **kw)[1]


def _cat(parts, i):
    return np.concatenate([p[2][i] for p in parts], axis=1)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


@pytest.mark.gpu
@pytest.mark.parametrize("wavelet", ["gmw", "morlet"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_process_cwt_family_at_odd_sizes(dtype, wavelet):
    """2 channels, odd S, chunk and depth, a ragged last chunk: Tx, Wx and dWx bitwise against the loops; and the same
    with temp_bytes = 1 (one chunk per slab)."""
    x = _channels(CWT_S, 2, dtype, 80)
    kw = dict(fs=CWT_FS, wavelet=wavelet, scales=CWT_SCALES, chunk=CWT_CHUNK, depth=CWT_DEPTH, dtype=dtype)
    cd = np.complex64 if dtype == F32 else np.complex128
    tx = _cwt_loop(x, CWT_CHUNK, CWT_DEPTH, "reflect",
                   lambda c: _ssq_cwt(c, wavelet=wavelet, scales=CWT_SCALES, fs=CWT_FS, nv=16))
    got, f = chunked.process_ssq_cwt(x, nv=16, **kw)
    assert got.dtype == cd and got.shape == (16, CWT_S + 2 * CWT_DEPTH * len(tx), 2)
    assert _same(got, _cat(tx, 0))
    assert np.array_equal(f, _first_window_freqs(x, wavelet=wavelet, scales=CWT_SCALES, fs=CWT_FS, nv=16))
    wx = _cwt_loop(x, CWT_CHUNK, CWT_DEPTH, "reflect",
                   lambda c: _cwt(c, wavelet=wavelet, scales=CWT_SCALES, fs=CWT_FS, derivative=True))
    Wx, sc, dWx = chunked.process_cwt(x, **kw)
    assert np.array_equal(sc, CWT_SCALES) and _same(Wx, _cat(wx, 0)) and _same(dWx, _cat(wx, 1))
    got1, _ = chunked.process_ssq_cwt(x, nv=16, temp_bytes=1, **kw)
    Wx1, _, dWx1 = chunked.process_cwt(x, temp_bytes=1, **kw)
    assert _same(got1, got) and _same(Wx1, Wx) and _same(dWx1, dWx)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_process_cwt_family_zero_boundary(dtype):
    """padtype="zero": the device halo is boundary 1 (zeros) and the plan pads with zeros."""
    x = _channels(CWT_S, 2, dtype, 82)
    kw = dict(fs=CWT_FS, wavelet="gmw", scales=CWT_SCALES, padtype="zero", chunk=CWT_CHUNK, depth=CWT_DEPTH, dtype=dtype)
    tx = _cwt_loop(x, CWT_CHUNK, CWT_DEPTH, "zero",
                   lambda c: _ssq_cwt(c, wavelet="gmw", scales=CWT_SCALES, fs=CWT_FS, nv=16, padtype="zero"))
    got, _ = chunked.process_ssq_cwt(x, nv=16, **kw)
    assert _same(got, _cat(tx, 0))
    wx = _cwt_loop(x, CWT_CHUNK, CWT_DEPTH, "zero",
                   lambda c: _cwt(c, wavelet="gmw", scales=CWT_SCALES, fs=CWT_FS, derivative=True, padtype="zero"))
    Wx, _, dWx = chunked.process_cwt(x, **kw)
    assert _same(Wx, _cat(wx, 0)) and _same(dWx, _cat(wx, 1))
    reflect, _ = chunked.process_ssq_cwt(x, nv=16, **dict(kw, padtype="reflect"))
    assert not _same(got, reflect)


@pytest.mark.gpu
@pytest.mark.parametrize("option", [dict(ssq_freqs="linear"), dict(maprange="maximal"), dict(flipud=False), dict(gamma=1e-3),
                                    dict(squeezing="lebesgue")], ids=lambda d: "-".join(map(str, list(d.items())[0])))
def test_process_ssq_cwt_options(option):
    x = _channels(CWT_S, 2, F64, 84)
    if "gamma" in option:
        x *= 1e-18           # |Wx| is about 1e15 |x| at these scales: the threshold then drops half of the bins, not all
    kw = dict(fs=CWT_FS, wavelet="gmw", scales=CWT_SCALES, nv=16)
    tx = _cwt_loop(x, CWT_CHUNK, CWT_DEPTH, "reflect", lambda c: _ssq_cwt(c, **kw, **option))
    got, f = chunked.process_ssq_cwt(x, chunk=CWT_CHUNK, depth=CWT_DEPTH, **kw, **option)
    assert _same(got, _cat(tx, 0))
    assert np.array_equal(f, _first_window_freqs(x, **kw, **option))
    plain, f_plain = chunked.process_ssq_cwt(x, chunk=CWT_CHUNK, depth=CWT_DEPTH, **kw)
    print(f"CHUNKED ssq_cwt {option}: {(_bits(got) != _bits(plain)).mean():.3f} of the words differ from the default run, "
          f"{(got != 0).mean():.3f} of Tx is nonzero")
    assert not _same(got, plain) or not np.array_equal(f, f_plain)         # the option reached the kernels
    assert got.any()


@pytest.mark.gpu
def test_process_cwt_without_the_derivative():
    x = _channels(CWT_S, 2, F64, 86)
    wx = _cwt_loop(x, CWT_CHUNK, CWT_DEPTH, "reflect",
                   lambda c: _cwt(c, wavelet="morlet", scales=CWT_SCALES, fs=CWT_FS, derivative=False))
    Wx, sc, dWx = chunked.process_cwt(x, fs=CWT_FS, wavelet="morlet", scales=CWT_SCALES, derivative=False, chunk=CWT_CHUNK,
                                      depth=CWT_DEPTH)
    assert dWx is None and wx[0][2][1] is None and _same(Wx, _cat(wx, 0)) and np.array_equal(sc, CWT_SCALES)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_process_ssq_cwt_halo_trim(dtype):
    x = _channels(CWT_S, 2, dtype, 88)
    tx = _cwt_loop(x, CWT_CHUNK, CWT_DEPTH, "reflect",
                   lambda c: _ssq_cwt(c, wavelet="gmw", scales=CWT_SCALES, fs=CWT_FS, nv=16))
    got, _ = chunked.process_ssq_cwt(x, fs=CWT_FS, wavelet="gmw", scales=CWT_SCALES, nv=16, chunk=CWT_CHUNK, depth=CWT_DEPTH,
                                     trim="halo", dtype=dtype)
    assert got.shape == (16, CWT_S, 2)
    for start, L, (T,) in tx:
        assert _same(got[:, start:start + L], T[:, CWT_DEPTH:CWT_DEPTH + L]), (start, L)


@pytest.mark.gpu
def test_automatic_scales_that_differ_between_chunks_are_refused():
    from ssqueeze_rs_amd import _rs
    full, ragged = CWT_CHUNK + 2 * CWT_DEPTH, CWT_S - 2 * CWT_CHUNK + 2 * CWT_DEPTH
    assert _rs._scales_or_default(None, full, 4, False).shape != _rs._scales_or_default(None, ragged, 4, False).shape
    x = _channels(CWT_S, 2, F64, 89)
    for fn in (chunked.process_ssq_cwt, chunked.process_cwt):
        with pytest.raises(ValueError, match="pass `scales`"):
            fn(x, fs=CWT_FS, nv=4, chunk=CWT_CHUNK, depth=CWT_DEPTH)
