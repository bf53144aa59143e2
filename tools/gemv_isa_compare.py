#!/usr/bin/env python
"""Device code of the few-row weight streams of this tree against another tree's, without a GPU:

    python tools/gemv_isa_compare.py <other tree> [--out FILE.md]

Both trees' csrc/gemv.hip, csrc/gemv_thin.hip and csrc/gemv_fp4.hip are compiled as tools/fp4_isa_compare.py compiles its files.
Every kernel of the other tree must have a twin here with the same WHOLE opcode sequence and equal VGPR / AGPR / SGPR / LDS / scratch.
The other tree's ``gemv_fp8v8_kernel<...>`` is matched to this tree's ``gemv_fp8_kernel<..., 8>`` and its ``gemv_fp8_kernel<...>`` to
``gemv_fp8_kernel<..., 16>`` (one kernel with the bytes per weight load as a template argument); a tree that already has the merged
kernel is matched name by name.  Kernels only this tree has are listed as new.  (profiles/gemv_plan_refactor_equivalence.md section 2.)
"""
import argparse
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fp4_isa_compare import META, kernels  # noqa: E402

FILES = ("gemv.hip", "gemv_thin.hip", "gemv_fp4.hip")
PREFIXES = ("gemv_", "thin_stream_kernel")


def twin_name(other_name, mine):
    """this tree's name of a kernel of the other tree"""
    if other_name in mine:
        return other_name
    m = re.match(r"gemv_fp8(v8)?_kernel<(.*)>$", other_name)
    return f"gemv_fp8_kernel<{m.group(2)}, {8 if m.group(1) else 16}>" if m else other_name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("--out")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as t1, tempfile.TemporaryDirectory() as t2:
        mine, other = kernels(ROOT, t1, FILES, PREFIXES), kernels(a.other, t2, FILES, PREFIXES)
    fmt = lambda m: " / ".join(str(m[k]) for k in META)
    lines = ["| kernel of the other tree | twin here | VGPR / AGPR / SGPR / LDS / scratch | instructions | opcode sequence |", "|---|---|---|---|---|"]
    bad, matched = 0, set()
    for name in sorted(other):
        om, oops = other[name]
        twin = twin_name(name, mine)
        if twin not in mine:
            bad += 1
            lines.append(f"| `{name}` | **none** | {fmt(om)} | {len(oops)} | |")
            continue
        matched.add(twin)
        m, ops = mine[twin]
        same, equal = ops == oops, all(m[k] == om[k] for k in META)
        bad += (not same) + (not equal)
        lines.append(f"| `{name}` | {'same name' if twin == name else '`' + twin + '`'} | {fmt(om)}{'' if equal else ' -> **' + fmt(m) + '**'} | "
                     f"{len(oops)}{'' if len(ops) == len(oops) else ' -> ' + str(len(ops))} | {'same' if same else '**differ**'} |")
    new = [f"| `{n}` | {fmt(mine[n][0])} | {len(mine[n][1])} |" for n in sorted(mine) if n not in matched]
    text = "\n".join(lines) + f"\n\n{len(other)} kernels of the other tree, {len(matched)} matched, {len(new)} only here\n"
    if new:
        text += "\n| new kernel | VGPR / AGPR / SGPR / LDS / scratch | instructions |\n|---|---|---|\n" + "\n".join(new) + "\n"
    text += f"\n{bad} finding(s)\n"
    if a.out:
        open(a.out, "w").write(text)
    print(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
