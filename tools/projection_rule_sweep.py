"""Sweep of the rule that picks a LLaMA layer projection's kernel, between two builds of libemu_hip.so (CPU only, no HIP call):

    python tools/projection_rule_sweep.py new.json
    EMU_HIP_TOOLS=1 EMU_HIP_LIB=/path/to/other/libemu_hip.so python tools/projection_rule_sweep.py other.json

A library that exports emu_llama_projection_kernel is asked through it.  An older one is asked the way its LlamaCall::project chained
its three hooks: emu_llama_weight_kernel, the W8A8 GEMM as bf16 in a matrix without an fp8 copy, then emu_llama_pack_kernel and
emu_llama_pack_thin_kernel, each only for a kernel inside the range it accepts (the others pass through, as in the engine).

The grid: the ten legal mode pairs; rows 1, 2, 3, 4, 8, 9, 16, 17, 20, 64, 65, 770; three width triples (hidden / heads_local *
head_dim / ffn_local); the four layer projections with the norm their call fuses and their epilogue; pack off, on, on plus wide; a
packed set with the rows emu_bf16_pack_rows names, with the other rows, and none; no inhibitor and each of the three alone; emu_gemm_tune
0 and 1 << 17; the fp8 copy present and absent.  One digit (the kernel) per point in the nesting order of POINT_ORDER, one string per
(mode pair, width triple), written as its runs: "7x96" = 96 points in a row answer 7, a bare digit = one point.  Equal files = the same
rule (profiles/projection_rule_equivalence.md)."""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emu_amd import _lib  # noqa: E402

NONE, RESID, SWIGLU = 0, 1, 2                       # emu_amd/ops.py: EPI_*
MODES = [(f8, 0) for f8 in range(7)] + [(0, f4) for f4 in (1, 2, 3)]
ROWS = (1, 2, 3, 4, 8, 9, 16, 17, 20, 64, 65, 770)
WIDTHS = ((6656, 6656, 17920), (6656, 896, 2240), (256, 256, 512))
PACK = ((0, 0), (1, 0), (1, 1))                     # (pack on, wide on)
SETS = ("named", "other", "none")
INHIBIT = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))      # (fused mode, decode tail, warm mask)
TUNES = (0, 1 << 17)
POINT_ORDER = ["rows", "fp8 copy (present, absent)", "pack (off, on, on + wide)", "set (named rows, other rows, none)",
               "projection (qkv, o_proj, gate/up, down)", "tune (0, 1 << 17)", "inhibitor (none, fused, tail, warm)"]      # (long runs)


def projections(H, HD, Fl, norm):
    """(N, K, norm in front, epilogue) of qkv, o_proj, gate/up and down; `norm`: the call fuses its two norms into the streams."""
    return ((3 * HD, H, norm, NONE), (H, HD, 0, RESID), (2 * Fl, H, norm, SWIGLU), (H, Fl, 0, RESID))


def ask_new(L, mode, widths, rows, proj, pack, set_rows, inhibit, tune, has_fp8):
    N, K, norm, epi = proj
    q = _lib.ProjectionC(fp8=mode[0], fp4=mode[1], pack=pack[0], pack_wide=pack[1], rows=rows, hidden=widths[0], heads_dim_local=widths[1],
                         ffn_local=widths[2], N=N, K=K, norm=norm, epi=epi, has_fp8=has_fp8, pack_rows=set_rows, set_n=N if set_rows else 0,
                         set_k=K if set_rows else 0, fused_mode=inhibit[0], tail_mode=inhibit[1], warm_mask=inhibit[2], tune=tune)
    return L.emu_llama_projection_kernel(q)


def ask_old(L, mode, widths, rows, proj, pack, set_rows, inhibit, tune, has_fp8):
    N, K, norm, epi = proj
    k = L.emu_llama_weight_kernel(mode[0], mode[1], rows, *widths)
    if k == 2 and not has_fp8:
        k = 0
    if 0 <= k <= 7:
        k = L.emu_llama_pack_kernel(k, rows, set_rows, pack[0], *inhibit, N, K, norm, epi, tune)
    if 0 <= k <= 8:
        k = L.emu_llama_pack_thin_kernel(k, rows, set_rows, N if set_rows else 0, K if set_rows else 0, pack[0], pack[1], N, K, norm, epi, tune)
    return k


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else "projection_rule_sweep.json"
    L = _lib.lib()
    ask = ask_new if hasattr(L, "emu_llama_projection_kernel") else ask_old
    answers, points = {}, 0
    for mode, widths in itertools.product(MODES, WIDTHS):
        digits = []
        for rows in ROWS:
            call = L.emu_llama_weight_kernel(mode[0], mode[1], rows, *widths)
            norm = int(call in (1, 3) or rows == 1)             # pick_path: the quantised 1..2-row streams and every one-row step
            for has_fp8, pack, which, proj, tune, inhibit in itertools.product((1, 0), PACK, SETS, projections(*widths, norm), TUNES, INHIBIT):
                r = L.emu_bf16_pack_rows(*proj, tune)
                set_rows = {"named": r, "other": 6 - r if r else 2, "none": 0}[which]
                k = ask(L, mode, widths, rows, proj, pack, set_rows, inhibit, tune, has_fp8)
                assert 0 <= k <= 9, (mode, widths, rows, proj, pack, set_rows, inhibit, tune, has_fp8, k)
                digits.append(str(k))
        runs = [(k, len(list(g))) for k, g in itertools.groupby(digits)]
        answers["fp8=%d fp4=%d | %d/%d/%d" % (mode + widths)] = " ".join(f"{k}x{n}" if n > 1 else k for k, n in runs)
        points += len(digits)
    json.dump({"point_order": POINT_ORDER, "rows": ROWS, "points": points, "answers": answers}, open(out_path, "w"), indent=1)
    print(f"{points} points -> {out_path} ({'emu_llama_projection_kernel' if ask is ask_new else 'the three chained hooks'})")


if __name__ == "__main__":
    main()
