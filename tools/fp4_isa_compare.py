#!/usr/bin/env python
"""Device code of the two MXFP4 matrix-core kernels of this tree against another tree's, without a GPU:

    python tools/fp4_isa_compare.py <other tree> [--out FILE.md]

Both trees' csrc/gemv_fp4_thin.hip and csrc/gemm_fp4.hip are compiled with ``hipcc <FLAGS of emu_amd/build.py> --cuda-device-only -S``.
Per ``fp4_thin_kernel`` / ``fp4_gemm_kernel`` instantiation: VGPR / AGPR / SGPR / LDS bytes / scratch bytes from the kernel's
metadata, the instruction count, and whether the opcode sequence from the first to the last ``v_mfma`` equals the other tree's.  A
kernel of this tree whose template arguments end in one ``bool`` more than the other tree's is matched to it when that last argument
is ``false`` (the instantiations that are dispatched for the same problems); the ones ending in ``true`` are listed as new.
(profiles/fp4_ktail.md, profiles/fp4_tile_refactor_equivalence.md section 2.)
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emu_amd.build import FLAGS, _hipcc  # noqa: E402

FILES = ("gemv_fp4_thin.hip", "gemm_fp4.hip")
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels(tree, tmp, files=FILES, prefixes=("fp4_thin_kernel", "fp4_gemm_kernel")):
    """{demangled kernel name: (metadata dict, [opcode, ...])} of the kernels of a tree's files whose names start with one of prefixes."""
    res = {}
    for f in files:
        asm = os.path.join(tmp, f + ".s")
        subprocess.run([_hipcc(), *FLAGS, "--cuda-device-only", "-S", os.path.join(tree, "emu_amd", "csrc", f), "-o", asm], check=True,
                       capture_output=True)
        text = open(asm).read()
        meta = {}
        for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
            blk = ".agpr_count:" + blk
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            meta[name] = {k: int(re.search(re.escape(k) + r":\s+(\d+)", blk).group(1)) for k in META}
        body = {}
        for m in re.finditer(r"^(\w+):\s*;\s*@\1\n(.*?)^\s*s_endpgm", text, re.S | re.M):
            ops = []
            for line in m.group(2).split("\n"):
                line = line.split(";")[0].strip()
                if line and not line.startswith(".") and not line.endswith(":"):
                    ops.append(line.split()[0])
            body[m.group(1)] = ops
        names = demangle(sorted(meta))
        for k in meta:
            short = re.sub(r"^void \(anonymous namespace\)::|\(GemvArgs(, int, int)?\)$", "", names[k])
            if short.startswith(prefixes):
                res[short] = (meta[k], body[k])
    return res


def kloop(ops):
    idx = [i for i, o in enumerate(ops) if o.startswith("v_mfma")]
    return ops[idx[0]:idx[-1] + 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("--out")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as t1, tempfile.TemporaryDirectory() as t2:
        mine, other = kernels(ROOT, t1), kernels(a.other, t2)
    fmt = lambda m: " / ".join(str(m[k]) for k in META)
    lines = ["| kernel | other: VGPR / AGPR / SGPR / LDS / scratch | this tree | instructions | first-to-last-MFMA opcodes |", "|---|---|---|---|---|"]
    new = ["| new kernel | VGPR / AGPR / SGPR / LDS / scratch | instructions |", "|---|---|---|"]
    bad = 0
    for name in sorted(mine):
        m, ops = mine[name]
        twin = name if name in other else re.sub(r", false>$", ">", name)
        if twin in other:
            om, oops = other[twin]
            same = kloop(ops) == kloop(oops)
            grew = any(m[k] > om[k] for k in META if k != ".sgpr_count")
            bad += (not same) + grew
            lines.append(f"| `{name}` | {fmt(om)} | {fmt(m)}{' **larger**' if grew else ''} | {len(oops)} -> {len(ops)} | {'same' if same else '**differ**'} |")
        else:
            bad += m[".private_segment_fixed_size"] != 0
            new.append(f"| `{name}` | {fmt(m)} | {len(ops)} |")
    text = "\n".join(lines) + "\n\n" + "\n".join(new) + f"\n\n{bad} finding(s)\n"
    if a.out:
        open(a.out, "w").write(text)
    print(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
