"""Compare the gfx950 machine code of two source trees kernel by kernel (no GPU needed).

    python tools/compare_isa.py OLD_TREE NEW_TREE [--rename OLD_SUBSTR=NEW_SUBSTR ...]
    python tools/compare_isa.py --prebuilt OLD_DIR NEW_DIR ...      (directories of *.co built that way)

Builds a device-only code object of every file in build.py's SOURCES for both trees (build.py's CXXFLAGS plus
--offload-device-only --no-gpu-bundle-output), splits `llvm-objdump -d` by kernel symbol and reads each kernel's
resources from `llvm-readelf --notes`.  Per kernel it prints one of:
  same         identical instructions and resources
  kernarg      instructions differ only in the immediate offsets of kernarg s_loads
  scalar       the vector, LDS and memory instructions are identical in order and operands once SGPR numbers are
               masked; only scalar instructions differ (a kernarg struct of a new layout is loaded by other s_loads,
               so SGPR allocation and the scalar schedule move); every resource but .sgpr_count is identical
  regalloc     the same vector, LDS and memory opcodes in the same order, register numbers may differ; every
               resource but .sgpr_count is identical
  DIFFERENT    anything else (the first differing lines follow)
.kernarg_segment_size is reported, not compared.
and lists the kernels that exist in only one tree.  --rename maps a substring of OLD's kernel symbols before
matching (for a kernel whose template parameters changed).  Exit status 1 if any kernel is DIFFERENT.
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
OBJDUMP = os.path.join(ROCM, "llvm/bin/llvm-objdump")
READELF = os.path.join(ROCM, "llvm/bin/llvm-readelf")
RES_KEYS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
            ".vgpr_spill_count", ".sgpr_spill_count")


def tree_build_config(tree: str):
    sys.path.insert(0, tree)
    try:
        import importlib
        mod = importlib.import_module("ssqueeze_rs_amd.build")
        importlib.reload(mod)
        return list(mod.SOURCES), list(mod.CXXFLAGS), mod._hipcc()
    finally:
        sys.path.pop(0)
        for k in [k for k in sys.modules if k.startswith("ssqueeze_rs_amd")]:
            del sys.modules[k]


def build_objects(tree: str, out: str, jobs: int) -> dict[str, str]:
    sources, flags, hipcc = tree_build_config(tree)
    csrc = os.path.join(tree, "ssqueeze_rs_amd", "csrc")
    os.makedirs(out, exist_ok=True)
    objs = {s: os.path.join(out, s + ".co") for s in sources}

    def one(s):
        cmd = [hipcc, *flags, "--offload-device-only", "--no-gpu-bundle-output", "-c", os.path.join(csrc, s), "-o", objs[s]]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)}\n{r.stderr}")

    with ThreadPoolExecutor(max_workers=jobs) as ex:
        list(ex.map(one, sources))
    return objs


def kernels(obj: str) -> dict[str, list[str]]:
    """symbol -> disassembled instruction lines (comments and addresses stripped)."""
    txt = subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", "--no-show-raw-insn", "--no-leading-addr", obj],
                         capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        ins = line.split(";")[0].split("//")[0].strip()
        if ins:
            out[cur].append(re.sub(r"\s+", " ", ins))
    return out


def resources(obj: str) -> dict[str, dict[str, str]]:
    """symbol -> the RES_KEYS entries of its amdhsa.kernels map (keys at the map's own indentation only)."""
    txt = subprocess.run([READELF, "--notes", obj], capture_output=True, text=True, check=True).stdout
    maps, cur = [], None
    for line in txt.splitlines():
        m = re.match(r"^  (- |  )(\.\w+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
            maps.append(cur)
        if cur is not None:
            cur[m.group(2)] = m.group(3).strip()
    return {d[".name"]: {k: d.get(k) for k in RES_KEYS} for d in maps if ".name" in d}


KERNARG = re.compile(r"^(s_load_\w+ s\[?[\d:]+\]?, s\[0:1\]), 0x[0-9a-f]+$")
SGPR = re.compile(r"\bs(\d+|\[\d+:\d+\])")


def vector_stream(ins: list[str]) -> list[str]:
    return [SGPR.sub("s#", x) for x in ins if not x.startswith("s_") and x != "..."]


def vector_opcodes(ins: list[str]) -> list[str]:
    return [x.split()[0] for x in vector_stream(ins)]


def classify(a: list[str], b: list[str]):
    if a == b:
        return "same", None
    if len(a) == len(b):
        diffs = [(x, y) for x, y in zip(a, b) if x != y]
        if all(KERNARG.match(x) and KERNARG.match(y) and KERNARG.match(x).group(1) == KERNARG.match(y).group(1)
               for x, y in diffs):
            return "kernarg", diffs
    if vector_stream(a) == vector_stream(b):
        return "scalar", None
    if vector_opcodes(a) == vector_opcodes(b):
        return "regalloc", None
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return "DIFFERENT", (i, x, y, len(a), len(b))
    return "DIFFERENT", (min(len(a), len(b)), "<end>", "<end>", len(a), len(b))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], help="OLD_SUBSTR=NEW_SUBSTR applied to OLD's symbols")
    ap.add_argument("--prebuilt", action="store_true", help="OLD and NEW are directories of device code objects")
    ap.add_argument("-j", type=int, default=8)
    args = ap.parse_args()
    renames = [r.split("=", 1) for r in args.rename]
    with tempfile.TemporaryDirectory() as tmp:
        side = {}
        for tag, tree in (("old", args.old), ("new", args.new)):
            if args.prebuilt:
                objs = [os.path.join(tree, f) for f in sorted(os.listdir(tree)) if f.endswith(".co")]
            else:
                objs = build_objects(os.path.abspath(tree), os.path.join(tmp, tag), args.j).values()
            ks, rs = {}, {}
            for o in objs:
                ks.update(kernels(o))
                rs.update(resources(o))
            ks = {k: v for k, v in ks.items() if k in rs}          # kernels only (resources exist for entry points)
            side[tag] = (ks, rs)
    (ko, ro), (kn, rn) = side["old"], side["new"]

    def mapped(name):
        for a, b in renames:
            name = name.replace(a, b)
        return name

    old_by_new = {mapped(k): k for k in ko}
    bad = 0
    counts = {"same": 0, "kernarg": 0, "scalar": 0, "regalloc": 0, "DIFFERENT": 0}
    for k in sorted(set(old_by_new) & set(kn)):
        status, info = classify(ko[old_by_new[k]], kn[k])
        r0, r1 = ro[old_by_new[k]], rn[k]
        if status in ("scalar", "regalloc"):
            r0, r1 = ({x: v for x, v in r.items() if x != ".sgpr_count"} for r in (r0, r1))
        if r0 != r1 and status != "DIFFERENT":
            status, info = "DIFFERENT", ("resources", r0, r1)
        counts[status] += 1
        if status != "same":
            print(f"{status:9s} {k}")
            if status == "DIFFERENT":
                bad += 1
                print("          ", info)
    only_old = sorted(k for n, k in old_by_new.items() if n not in kn)
    only_new = sorted(set(kn) - set(old_by_new))
    print(f"\n{len(kn)} kernels in NEW: {counts['same']} same, {counts['kernarg']} kernarg offsets only, "
          f"{counts['scalar']} scalar code only, {counts['regalloc']} register numbers only, "
          f"{counts['DIFFERENT']} different")
    print(f"only in OLD ({len(only_old)}):")
    for k in only_old:
        print("   ", k)
    print(f"only in NEW ({len(only_new)}):")
    for k in only_new:
        print("   ", k)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
