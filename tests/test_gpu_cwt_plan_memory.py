"""A CWT plan gives back the device memory it took (csrc/api_cwt.hip: every table belongs to the plan's `DeviceBufs`).

Three plans that between them hold every table a plan can have:

| case         | N       | scales               | tables beyond the common ones                                            |
| fp32 tiles   | 350 003 | Morlet 2^(j/4), case | register core (psiT, tw1024, tw20), analytic tiles (osHa, xa_*), 4-row,  |
|              |         | C of test_gpu_cwt_   | 8-row, decimated and full-circle tile tables, f2a / f2z / twz            |
|              |         | tiles.py             |                                                                          |
| fp64 zoom    | 20 000  | Morlet 2^(j/4)       | two-step with band-limited scales: the compact twiddles behind tw1 / tw2 |
|              |         | (nv = 4), j = 4..51  | and inside twz, f2z                                                      |
| upstream     | 4 096   | GMW, log-piecewise   | the row weights (d_ups_const), allocated by the first host call that     |
|              |         |                      | needs them; through the host path and its plan cache                     |

Per case: the footprint is the drop of free device memory while one plan is alive; after eight create / destroy rounds
(upstream: call / `ssq_host_cache_clear` rounds) free memory must not be lower than after the first round by more than
HALF a footprint.  That bound is a condition, not a measurement: one leaked table of the dominant kind (the wavelet
table, or any of the tile tables) per round exceeds it after eight rounds many times over, the allocator's granularity
does not come near it.
"""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from ssqueeze_rs_amd import _lib
from ssqueeze_rs_amd import upstream as up
from tests.test_gpu_cwt_tiles import _scales, _segments

pytestmark = pytest.mark.gpu

ROUNDS = 8


def _free():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _plan_round(dtype, N, scales):
    """One create / destroy of a reference-variant Morlet plan; free memory while it is alive."""
    lib = _lib.load()
    vp = C.c_void_p
    plan = vp()
    sc = np.ascontiguousarray(scales, dtype=np.float64)
    _lib.check(lib.ssq_cwt_plan_create(C.byref(plan), dtype, N, _lib.WAVELET["morlet"], sc.ctypes.data_as(vp), len(sc),
                                       1.0, _lib.PAD["reflect"]))
    alive = _free()
    _lib.check(lib.ssq_cwt_plan_destroy(plan))
    return alive


def _upstream_round(x, scales):
    """One host call on log-piecewise scales (its plan, the row weights and the scratch stay cached) and the clear."""
    Tx = up.ssq_cwt(x, ("gmw", {"beta": 8}), scales=scales)[0]
    assert np.isfinite(Tx).all()
    del Tx
    gc.collect()                                           # the pinned result goes back to the pool ...
    alive = _free()
    _lib.load().ssq_host_cache_clear()                     # ... and the pool, the scratch and the plans are let go
    return alive


def _assert_rounds_give_memory_back(one_round):
    one_round()                                            # code objects, streams, the runtime's own pools: not a plan's
    before = _free()
    footprint = before - one_round()
    print(f"footprint {footprint} bytes")
    assert footprint > 0
    after = []
    for _ in range(ROUNDS):
        one_round()
        after.append(_free())
    print("free after each round, relative to the first:", [a - after[0] for a in after])
    assert after[-1] >= after[0] - footprint // 2, (footprint, after)


def test_fp32_plan_with_register_core_and_every_tile_table():
    N, scales = 350_003, _scales("C", "morlet")
    seg, reg, _ = _segments(N, "morlet", scales)
    assert reg and all(seg[k][1] > seg[k][0] for k in ("analytic", "rows4", "rows8", "decimated", "full")), seg
    _assert_rounds_give_memory_back(lambda: _plan_round(_lib.SSQ_F32, N, scales))


def test_fp64_two_step_plan_with_band_limited_scales():
    scales = 2.0 ** (np.arange(4, 52) / 4.0)               # nv = 4; from a = 117 on the spectrum fits 2048 bins (mode Z)
    _assert_rounds_give_memory_back(lambda: _plan_round(_lib.SSQ_F64, 20_000, scales))


def test_upstream_log_piecewise_host_path():
    N = 4096
    scales = up.process_scales("log-piecewise", N, ("gmw", {"beta": 8})).reshape(-1)
    x = np.random.default_rng(4096).standard_normal(N)
    try:
        _assert_rounds_give_memory_back(lambda: _upstream_round(x, scales))
    finally:
        _lib.load().ssq_host_cache_clear()
