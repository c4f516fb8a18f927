"""The wait counts of `stft_tx1024_kernel`'s tile loop (csrc/stft_fused.hip), read from the gfx950 assembly.  No GPU.

The kernel prefetches the next tile's 16 samples in the middle of a tile and issues the tile's Tx stores after them.
Loads and stores share the one in-order `vmcnt` counter, so an `s_waitcnt vmcnt(N)` that guards a prefetched sample
with N below the number of stores behind it also waits for stores of the tile just read out -- once per tile, with
every wave of the CU at the same point.  The wait-count pass takes the FEWEST operations behind a load over all paths
that reach the wait, so each interior instantiation has exactly one read-out path (template parameter PAIRED) and takes
the window multiply and pass 0 of the NEXT tile at the end of the loop body, behind the read-out: every way to those
waits then leads through a read-out's stores.  This test holds the generated code to that, in the
tile LOOP (the block's first tile, ahead of the loop, has no store behind its samples and waits vmcnt(7..0), as it must):

  * every `s_waitcnt` with a `vmcnt(N)` between the loop's second `s_barrier` and the next sample prefetch -- the
    waits for the prefetched samples -- has N >= the number of unconditional Tx stores of that read-out: 4 sweeps of
    16 bytes for the paired path, 8 sweeps of 8 bytes for the per-frame path (the last, partial sweep is conditional);
  * there is no other `vmcnt` wait anywhere in the loop (in particular no `vmcnt(0)`);
  * the kernel uses at most 128 vector registers (16 waves per CU) and no scratch.

The file is compiled once per module with the flags of `ssqueeze_rs_amd/build.py`.  The test reads wait counts, barriers,
branches and the names of global loads and stores, nothing else.
"""
import os
import re
import subprocess

import pytest

from ssqueeze_rs_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ssqueeze_rs_amd", "csrc", "stft_fused.hip")
# stft_tx1024_kernel<EDGE = false, LEB = false, WKDBG = false, PAIRED>(StftDev<float>)
KERNEL = "_ZN3ssq18stft_tx1024_kernelILb0ELb0ELb0ELb%dEEEvNS_7StftDevIfEE"
# read-out -> (mangled name, unconditional Tx stores per tile and thread, store instruction)
CASES = {
    "paired": (KERNEL % 1, 4, "global_store_dwordx4"),
    "per_frame": (KERNEL % 0, 8, "global_store_dwordx2"),
}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    try:
        hipcc = build._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("tx1024_isa") / "stft_fused.s")
    cmd = [hipcc, *build.CXXFLAGS, "-S", "--cuda-device-only", SRC, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out) as f:
        return f.read().split("\n")


def _body(asm, name):
    """The instructions and labels of kernel `name`, comments stripped."""
    start = asm.index(next(ln for ln in asm if ln.startswith(name + ":")))
    end = next(k for k in range(start, len(asm)) if asm[k].startswith(".Lfunc_end"))
    body = [ln.split(";")[0].strip() for ln in asm[start + 1:end]]
    return [ln for ln in body if ln]


def _walk(body, start, stop=None):
    """Indices reachable from `start` along fall-through and both ways of every branch, up to s_endpgm -- and not past
    the first instruction of a path whose mnemonic starts with `stop`."""
    label = {ln[:-1]: k for k, ln in enumerate(body) if ln.endswith(":")}
    seen, todo = set(), [start]
    while todo:
        k = todo.pop()
        while k < len(body) and k not in seen:
            seen.add(k)
            op = body[k].split()
            if op[0] == "s_endpgm" or (stop and op[0].startswith(stop)):
                break
            if op[0].startswith("s_cbranch") or op[0] == "s_branch":
                todo.append(label[op[1]])
                if op[0] == "s_branch":
                    break
            k += 1
    return seen


def _vm_waits(body, idx):
    out = []
    for k in sorted(idx):
        m = re.match(r"s_waitcnt\b.*\bvmcnt\((\d+)\)", body[k])
        if m:
            out.append(int(m.group(1)))
    return out


def _meta(asm, name, key):
    """`key` of the kernel's entry in the amdhsa.kernels metadata (entries open with '  - .', keys sit at that depth)."""
    at = next(k for k, ln in enumerate(asm) if re.match(r"    \.name:\s*%s\s*$" % re.escape(name), ln))
    lo = max(k for k in range(at + 1) if asm[k].startswith("  - ."))
    hi = next((k for k in range(at + 1, len(asm)) if asm[k].startswith("  - .") or not asm[k].startswith("  ")), len(asm))
    vals = [int(m.group(1)) for ln in asm[lo:hi] for m in [re.match(r"  [ -] \.%s:\s*(\d+)\s*$" % key, ln)] if m]
    assert len(vals) == 1, (name, key, vals)
    return vals[0]


@pytest.mark.parametrize("case", list(CASES))
def test_loop_top_waits_leave_the_tx_stores_in_flight(asm, case):
    name, n_stores, store_op = CASES[case]
    body = _body(asm, name)

    def is_store(k):
        return body[k].split()[0].startswith("global_store")

    # the tile loop's two barriers are the ones that lie on a cycle; the read-out's stores come between the first and
    # the second
    barriers = [k for k, ln in enumerate(body) if ln == "s_barrier"]
    cyc = [b for b in barriers if b in _walk(body, b + 1)]
    assert len(cyc) == 2, (case, barriers, cyc)
    second = [b for b in cyc if not any(is_store(k) for k in _walk(body, b + 1, stop="s_barrier"))]
    assert len(second) == 1, (case, cyc, second)
    b2 = second[0]
    loop = _walk(body, b2 + 1)
    stores = [k for k in sorted(loop) if is_store(k)]
    assert len(stores) == n_stores + 1 and all(body[k].split()[0] == store_op for k in stores), \
        (case, [body[k] for k in stores])               # the unconditional sweeps + the conditional last one
    guard = _vm_waits(body, _walk(body, b2 + 1, stop="global_load"))     # up to the next tile's sample prefetch
    every = _vm_waits(body, loop)
    print(f"TX1024 ISA {case}: vmcnt waits for the prefetched samples {guard}; in the whole loop {every}")
    assert guard, "no vmcnt wait guards the prefetched samples: the loop is not the one this test knows"
    assert min(guard) >= n_stores, (case, guard)
    assert sorted(every) == sorted(guard), (case, "a vmcnt wait elsewhere in the loop", every, guard)
    assert 0 not in every


@pytest.mark.parametrize("case", list(CASES))
def test_registers_and_scratch(asm, case):
    name = CASES[case][0]
    assert _meta(asm, name, "vgpr_count") <= 128
    assert _meta(asm, name, "private_segment_fixed_size") == 0
