#!/usr/bin/env python
"""The few-row MXFP4 stream on the matrix cores (csrc/gemv_fp4_thin.hip) against what it replaces, one process (needs a GPU):

    python tools/fp4_wide_time.py [--layers 60] [--iters 30] [--rounds 2] [--out profiles/fp4_wide.md]
    python tools/fp4_wide_time.py --ab          # 16 / 32 weight rows per workgroup (emu_gemm_tune bits 28-29); prints only
    python tools/fp4_wide_time.py --shards --out FILE.md   # leg 1 at 5 / 8 / 16 rows on the TP = 4 / 8 per-rank shapes, through
                                                           # ops.linear_fp4w_mfma (K = 896 / 2240 / 4480: a partial last K stage)

1. Every weight stream on its own at the LLaMA-33B shapes (HIP events, the weights rotating through more copies than the infinity
   cache holds, the contenders alternating in windows of one run): at 5 / 8 / 16 rows the bf16 few-row stream (gemv_thin.hip)
   against the new kernel; at 1 / 2 rows the VALU fp4 stream (gemv_fp4.hip, no fused norm) against the new kernel.
2. A 5-beam step at --layers layers behind a 770-row prompt: bf16 against ``use_fp4(True, wide=True)``, ms per step from the
   difference of two beam searches of different lengths (the prefill and the set-up cancel), windows alternating.

Writes both tables to --out.  Synthetic weights: quality on a trained checkpoint is not measured here.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emu_amd import mxfp4, ops, synth  # noqa: E402
from emu_amd._lib import lib  # noqa: E402
from emu_amd.conf.emu_conf import LlamaCfg  # noqa: E402
from emu_amd.constants import VOCAB_EMU2_CHAT  # noqa: E402
from emu_amd.llama import EmuHipContext, LlamaEngine  # noqa: E402

BF16 = torch.bfloat16
HBM = 8.0e12
SHAPES = [("qkv", 19968, 6656, 0), ("o+res", 6656, 6656, 1), ("gateup+swiglu", 35840, 6656, 2), ("down+res", 6656, 17920, 1),
          ("lm_head", 32274, 6656, 0)]
# per-rank shapes of the 33B model at TP = 4 / 8 (emu_amd/tp.py): the row-parallel matrices' K is no multiple of 256 there
SHARD_SHAPES = [("o+res tp8", 6656, 896, 1), ("down+res tp8", 6656, 2240, 1), ("down+res tp4", 6656, 4480, 1), ("qkv tp8", 2688, 6656, 0),
                ("gateup+swiglu tp8", 4480, 6656, 2)]


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def weight_sets(N, K, dev, want_bf16):
    """> 600 MB of 4-bit copies (and as many bf16 copies, if wanted) of an [N, K] matrix."""
    n4 = max(1, int(600e6 // (N * K * 17 / 32)) + 1)
    nb = max(1, int(600e6 // (N * K * 2)) + 1)
    w4, wb = [], []
    for c in range(max(n4, nb if want_bf16 else 0)):
        w = (torch.randn(N, K, device=dev) * 0.02).to(BF16)
        if c < n4:
            w4.append(ops.quantize_mxfp4_rows(w))
        if want_bf16 and c < nb:
            wb.append(w)
        del w
    return w4, wb


def stream_leg(a, dev, rows_list, against):
    """rows: [name, N, K, M, other us, other frac, new us, new frac]; against = 'bf16' (thin bf16 stream) or 'valu' (gemv_fp4)."""
    out = []
    fp4_mfma = ops.linear_fp4w_mfma if a.shards else ops.linear_fp4w_thin
    for name, N, K, epi in (SHARD_SHAPES if a.shards else SHAPES):
        w4, wb = weight_sets(N, K, dev, against == "bf16")
        if a.shards:                                     # scale rows at the kernels' stride once, not per launch
            w4 = [(q, mxfp4.pad_scales(sc, K)) for q, sc in w4]
        for M in rows_list:
            xv = torch.randn(M, K, device=dev).to(BF16)
            res = torch.randn(M, N, device=dev).to(BF16) if epi == 1 else None
            i = [0]

            def new():
                i[0] += 1
                fp4_mfma(xv, *w4[i[0] % len(w4)], res=res, epi=epi)

            def other():
                i[0] += 1
                if against == "bf16":
                    ops.linear(xv, wb[i[0] % len(wb)], res=res, epi=epi)
                else:
                    ops.linear_fp4w(xv, *w4[i[0] % len(w4)], res=res, epi=epi)
            t_new, t_other = [], []
            for _ in range(a.rounds):
                t_other.append(timeit(other, a.iters))
                t_new.append(timeit(new, a.iters))
            tn, to = min(t_new), min(t_other)
            b_new = N * K * 17 / 32
            b_other = N * K * 2 if against == "bf16" else b_new
            row = [name, N, K, M, to * 1e6, b_other / to / HBM, tn * 1e6, b_new / tn / HBM]
            print("stream", against, row, flush=True)
            out.append(row)
        del w4, wb
        torch.cuda.empty_cache()
    return out


def ab_leg(a, dev):
    print("fp4 few-row stream, weight rows per workgroup A/B, us per launch: heuristic / 16 / 32")
    for name, N, K, epi in SHAPES:
        w4, _ = weight_sets(N, K, dev, False)
        for M in (5, 16):
            xv = torch.randn(M, K, device=dev).to(BF16)
            res = torch.randn(M, N, device=dev).to(BF16) if epi == 1 else None
            i = [0]

            def fn():
                i[0] += 1
                ops.linear_fp4w_thin(xv, *w4[i[0] % len(w4)], res=res, epi=epi)
            ts = []
            for pin in (0, 1, 2):
                lib().emu_gemm_tune(pin << 28)
                ts.append(min(timeit(fn, a.iters) for _ in range(a.rounds)) * 1e6)
            lib().emu_gemm_tune(0)
            print(f"{name:16s} M={M:2d} " + " ".join(f"{t:8.1f}" for t in ts), flush=True)
        del w4
        torch.cuda.empty_cache()


def beam_leg(a, dev):
    lcfg = LlamaCfg(num_hidden_layers=a.layers)
    lm = LlamaEngine(lcfg, VOCAB_EMU2_CHAT, EmuHipContext(dev))
    t0 = time.time()
    lm.load_weights(synth.iter_synth(synth.llama_param_shapes(lcfg, VOCAB_EMU2_CHAT), seed=0, device=dev, dtype=BF16))
    lm.quantize_fp4()
    torch.cuda.synchronize()
    print(f"weights + fp4 copies ready in {time.time() - t0:.0f}s, {torch.cuda.memory_allocated() / 2**30:.1f} GiB", flush=True)
    S, nb = a.prompt, 5
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(1, S, lcfg.hidden_size, generator=g) * 0.02).to(BF16).to(dev)
    mask = torch.ones(1, S, dtype=torch.long)
    n0, n1 = a.short, a.long

    def call(n):
        lm.beam_search_generate(x, mask, nb, n, min_len=n)
        torch.cuda.synchronize()

    def per_step():
        ts = {}
        for n in (n0, n1):
            call(n)                                  # warm-up: graph capture of this length
            t = time.perf_counter()
            call(n)
            ts[n] = time.perf_counter() - t
        return (ts[n1] - ts[n0]) / (n1 - n0) * 1e3
    times = {"bf16": [], "fp4 wide": []}
    for rnd in range(a.rounds):
        for mode in times:
            lm.use_fp4(mode != "bf16", wide=True)
            times[mode].append(per_step())
            print(f"round {rnd} {mode}: {times[mode][-1]:.3f} ms per 5-beam step", flush=True)
    lm.use_fp4(False)
    return times, S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--prompt", type=int, default=770)
    ap.add_argument("--short", type=int, default=8)
    ap.add_argument("--long", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp4_wide.md"))
    ap.add_argument("--ab", action="store_true", help="only the rows-per-workgroup A/B (prints, writes nothing)")
    ap.add_argument("--skip", default="", help="comma list of legs to leave out: stream, beam")
    ap.add_argument("--shards", action="store_true", help="only leg 1 at 5 / 8 / 16 rows, on the TP = 4 / 8 per-rank shapes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fp4_wide_time.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    if a.ab:
        with torch.no_grad():
            ab_leg(a, dev)
        return
    skip = set(a.skip.split(","))
    out = ["# MXFP4 weights for 3..16-row steps on the matrix cores: measured against the bf16 few-row stream", "",
           f"Written by `tools/fp4_wide_time.py` ({torch.cuda.get_device_name(0)}; one process, so every comparison is same-run, same-box).",
           "Synthetic weights: **quality of round-to-nearest MXFP4 on the real Emu2 checkpoint is not measured**.  The mode is opt-in",
           "(`LlamaEngine.use_fp4(True, wide=True)`).", ""]
    with torch.no_grad():
        if "stream" not in skip:
            wide = stream_leg(a, dev, (5, 8, 16), "bf16")
            out += ["## Every weight stream on its own, 5 / 8 / 16 rows: bf16 few-row stream against the 4-bit matrix-core stream", "",
                    f"HIP events around {a.iters} launches, weights rotating through > 600 MB of copies, {a.rounds} windows per contender",
                    "alternating, best window; fraction = algorithmic weight bytes (bf16 2, fp4 17/32 per weight) / time / 8 TB/s.", "",
                    "| stream | N | K | rows | bf16 us | frac | fp4 us | frac | fp4 / bf16 time |", "|---|---|---|---|---|---|---|---|---|"]
            for r in wide:
                out.append(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]} | {r[4]:.1f} | {r[5]:.3f} | {r[6]:.1f} | {r[7]:.3f} | {r[6] / r[4]:.3f} |")
        if "stream" not in skip and not a.shards:
            narrow = stream_leg(a, dev, (1, 2), "valu")
            out += ["", "## 1 / 2 rows: the VALU 4-bit stream (`gemv_fp4_kernel`, no fused norm) against the matrix-core stream", "",
                    "Same method.  This table says whether one-row fp4 decode should move onto the matrix cores.", "",
                    "| stream | N | K | rows | VALU us | frac | MFMA us | frac | MFMA / VALU time |", "|---|---|---|---|---|---|---|---|---|"]
            for r in narrow:
                out.append(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]} | {r[4]:.1f} | {r[5]:.3f} | {r[6]:.1f} | {r[7]:.3f} | {r[6] / r[4]:.3f} |")
            wins = sum(1 for r in narrow if r[6] < r[4])
            out += ["", f"The matrix-core stream is faster than the VALU stream in {wins} of {len(narrow)} of these cases.", ""]
        if "beam" not in skip and not a.shards:
            times, S = beam_leg(a, dev)
            b, f = min(times["bf16"]), min(times["fp4 wide"])
            out += [f"## A 5-beam step, {a.layers} layers at the LLaMA-33B shape, TP = 1", "",
                    f"Prompt of {S} rows, 5 beams; ms per step = (time of a {a.long}-token search - time of a {a.short}-token search) / {a.long - a.short},",
                    f"each search run once to warm up (graph capture) and once timed, host clock between device synchronisations, {a.rounds} windows",
                    "per stream alternating; best window, all windows in brackets.", "",
                    "| stream | ms per 5-beam step | windows | time / bf16 |", "|---|---|---|---|",
                    f"| bf16 | {b:.3f} | {', '.join(f'{v:.3f}' for v in times['bf16'])} | 1.000 |",
                    f"| fp4 wide | {f:.3f} | {', '.join(f'{v:.3f}' for v in times['fp4 wide'])} | {f / b:.3f} |", ""]
            if f < b:
                out += [f"The 5-beam step is **faster** with the 4-bit stream in this run: {f:.3f} ms against {b:.3f} ms (x{b / f:.2f}).", ""]
            else:
                out += [f"**The 5-beam step is NOT faster with the 4-bit stream in this run: {f:.3f} ms against {b:.3f} ms.**  The mode stays opt-in.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(out))
    print("\n".join(out))


if __name__ == "__main__":
    main()
