"""GPU tests of the walk kernel of `upstream.tmssq_cwt` alone (`upstream.tmssq_cwt_walk`, csrc/cwt_tmsst.hip)
against the walk by the definition (tests/helpers/tmsst_ref.walk).  The result is integer-exact: `np.array_equal`
throughout.  The sizes sit on the tile's edges (T - 1, T, T + 1 columns), span several tiles, and pass the
grid-dimension limit of 65535 rows; the maps take every path of a step: inside the staged tile and halo (LDS), outside it
(the one-step plane in device memory), out and back in, fixed points, cycles and columns that are not kept."""
import numpy as np
import pytest

from ssqueeze_rs_amd import upstream as up
from tests.helpers.tmsst_ref import walk

pytestmark = pytest.mark.gpu

T, HALO = up.tmssq_cwt_tile_cols()
ITERS = (1, 2, 7, 64)
SIZES = [1, T - 1, T, T + 1, 3 * T + 5]


def hand_maps(n):
    """The maps written by hand on n columns: a dict of int32 [n]."""
    j = np.arange(n, dtype=np.int64)
    hop = HALO + 1
    maps = {
        "identity": j,
        "none": np.full(n, -1),
        "shift": np.minimum(j + 1, n - 1),
        "two-cycle": np.where((j ^ 1) < n, j ^ 1, j),
        "shift-with-holes": np.where(j % 5 == 3, -1, np.minimum(j + 1, n - 1)),
        "all-to-zero": np.zeros(n, dtype=np.int64),            # a far jump from every tile but the first, then a fixed point
        "far-hop": np.where(j + hop < n, j + hop, j),          # every step leaves the stage
        # out of the stage and back into it: j -> j + T + HALO + 3 -> j + 1 -> ...
        "out-and-back": np.where(j % 2 == 0, np.where(j + T + HALO + 3 < n, j + T + HALO + 3, j),
                                 np.maximum(j - (T + HALO + 2), 0)),
        "ends-cycle": np.where(j == 0, n - 1, np.where(j == n - 1, 0, j)),
    }
    return {k: v.astype(np.int32) for k, v in maps.items()}


@pytest.mark.parametrize("n", SIZES)
def test_maps_written_by_hand(n):
    maps = hand_maps(n)
    stack = np.stack(list(maps.values()))                      # [9, n]: one row a map
    for it in ITERS:
        got = up.tmssq_cwt_walk(stack, it)
        want = walk(stack, it)
        assert got.dtype == np.int32 and got.shape == stack.shape
        for r, name in enumerate(maps):
            assert np.array_equal(got[r], want[r]), (name, n, it)
    assert np.array_equal(up.tmssq_cwt_walk(stack, 1), stack)


def test_the_hand_maps_take_the_far_path():
    """At 3 T + 5 columns the far hop, the jump to column 0 and the cycle between the ends land outside the stage of the
    tile they started in: the read of the one-step plane in device memory is what these maps test."""
    n = 3 * T + 5
    maps = hand_maps(n)
    j = np.arange(n)
    for name in ("far-hop", "out-and-back", "all-to-zero", "ends-cycle"):
        t = maps[name].astype(np.int64)
        t0 = j // T * T
        outside = (t < t0 - HALO) | (t >= np.minimum(t0 + T, n) + HALO)
        assert outside.any(), name
    assert not np.array_equal(walk(maps["out-and-back"], 3), walk(maps["out-and-back"], 2))


def random_maps(n, rows, seed):
    """Seeded maps [3, rows, n] with a third of the entries -1: targets uniform over the row, within +-50 of their column,
    and a mix of the two."""
    rng = np.random.default_rng(seed)
    j = np.arange(n)[None, :]
    uni = rng.integers(0, n, size=(rows, n))
    near = np.clip(j + rng.integers(-50, 51, size=(rows, n)), 0, n - 1)
    mix = np.where(rng.random((rows, n)) < 0.5, uni, near)
    out = np.stack([uni, near, mix])
    out[rng.random(out.shape) < 1 / 3] = -1
    return out.astype(np.int32)


@pytest.mark.parametrize("n", SIZES)
def test_random_maps(n):
    maps = random_maps(n, 5, n)                                # a batch of 3 (one kind a signal) x 5 rows
    for it in ITERS:
        got = up.tmssq_cwt_walk(maps, it)
        assert got.shape == maps.shape and np.array_equal(got, walk(maps, it)), (n, it)
    assert np.array_equal(up.tmssq_cwt_walk(maps[2], 7), walk(maps[2], 7))            # [rows, n] without a batch


def test_past_the_grid_dimension_limit():
    """65537 rows of 16 columns: two launches, the second of two rows."""
    rows, n = 65537, 16
    rng = np.random.default_rng(7)
    maps = rng.integers(-1, n, size=(rows, n)).astype(np.int32)
    for it in (2, 64):
        assert np.array_equal(up.tmssq_cwt_walk(maps, it), walk(maps, it)), it
