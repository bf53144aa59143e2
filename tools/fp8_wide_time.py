#!/usr/bin/env python
"""The few-row fp8 stream on the matrix cores (csrc/gemv_fp8_thin.hip) against what it replaces, one process (needs a GPU):

    python tools/fp8_wide_time.py [--layers 60] [--iters 30] [--rounds 3] [--out profiles/fp8_wide.md]
    python tools/fp8_wide_time.py --ab          # 16 / 32 weight rows per workgroup (emu_gemm_tune bits 28-29); prints only

1. Every weight stream on its own at the LLaMA-33B shapes (HIP events, the weights rotating through more copies than the infinity
   cache holds, the contenders alternating in windows of one run): at 3 / 5 / 8 / 16 rows the bf16 few-row stream (gemv_thin.hip;
   3 rows: the v_dot2c block kernel the planner picks there) and the MXFP4 few-row stream (gemv_fp4_thin.hip) against the new kernel;
   at 2 rows the VALU fp8 stream (gemv_fp8_kernel, no fused norm) against the new kernel -- reported only, the rule stays.
2. A 5-beam step at --layers layers behind a 770-row prompt: bf16, ``use_fp8(True)`` (5 rows stay on bf16), ``use_fp8(True,
   wide=True)`` and ``use_fp4(True, wide=True)``, ms per step from the difference of two beam searches of different lengths (the
   prefill and the set-up cancel), windows alternating; then the 20-row step of four prompts x five beams, where the mode ends.

Writes the tables to --out, every window next to the best one.  Synthetic weights: quality on a trained checkpoint is not measured.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emu_amd import ops, synth  # noqa: E402
from emu_amd._lib import lib  # noqa: E402
from emu_amd.conf.emu_conf import LlamaCfg  # noqa: E402
from emu_amd.constants import VOCAB_EMU2_CHAT  # noqa: E402
from emu_amd.llama import EmuHipContext, LlamaEngine  # noqa: E402

BF16 = torch.bfloat16
HBM = 8.0e12
SHAPES = [("qkv", 19968, 6656, 0), ("o+res", 6656, 6656, 1), ("gateup+swiglu", 35840, 6656, 2), ("down+res", 6656, 17920, 1),
          ("lm_head", 32274, 6656, 0)]


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


def weight_sets(N, K, dev, kinds):
    """> 600 MB of copies of an [N, K] matrix in each of ``kinds`` ("bf16", "fp8", "fp4"), all from the same random matrices."""
    per = {"bf16": 2.0, "fp8": 1.0, "fp4": 17 / 32}
    need = {k: max(1, int(600e6 // (N * K * per[k])) + 1) for k in kinds}
    sets = {k: [] for k in kinds}
    for c in range(max(need.values())):
        w = (torch.randn(N, K, device=dev) * 0.02).to(BF16)
        if "bf16" in kinds and c < need["bf16"]:
            sets["bf16"].append((w,))
        if "fp8" in kinds and c < need["fp8"]:
            sets["fp8"].append(ops.quantize_fp8_rows(w))
        if "fp4" in kinds and c < need["fp4"]:
            sets["fp4"].append(ops.quantize_mxfp4_rows(w))
        del w
    return sets


CALL = {"bf16": ops.linear, "fp8": ops.linear_fp8w_thin, "fp4": ops.linear_fp4w_thin, "fp8 valu": ops.linear_fp8w}
BYTES = {"bf16": 2.0, "fp8": 1.0, "fp4": 17 / 32, "fp8 valu": 1.0}


def stream_leg(a, dev, rows_list, contenders):
    """rows: [name, N, K, M, {contender: [window seconds]}]; the contenders' windows alternate."""
    out = []
    kinds = sorted({c.split()[0] for c in contenders})
    for name, N, K, epi in SHAPES:
        sets = weight_sets(N, K, dev, kinds)
        for M in rows_list:
            xv = torch.randn(M, K, device=dev).to(BF16)
            res = torch.randn(M, N, device=dev).to(BF16) if epi == 1 else None
            i = [0]

            def run(c):
                def fn():
                    i[0] += 1
                    ws = sets[c.split()[0]]
                    CALL[c](xv, *ws[i[0] % len(ws)], res=res, epi=epi)
                return fn
            t = {c: [] for c in contenders}
            for _ in range(a.rounds):
                for c in contenders:
                    t[c].append(timeit(run(c), a.iters))
            print("stream", name, N, K, M, {c: [round(v * 1e6, 1) for v in ts] for c, ts in t.items()}, flush=True)
            out.append([name, N, K, M, t])
        del sets
        torch.cuda.empty_cache()
    return out


def ab_leg(a, dev):
    print("fp8 few-row stream, weight rows per workgroup A/B, us per launch: heuristic / 16 / 32")
    for name, N, K, epi in SHAPES:
        sets = weight_sets(N, K, dev, ["fp8"])["fp8"]
        for M in (5, 16):
            xv = torch.randn(M, K, device=dev).to(BF16)
            res = torch.randn(M, N, device=dev).to(BF16) if epi == 1 else None
            i = [0]

            def fn():
                i[0] += 1
                ops.linear_fp8w_thin(xv, *sets[i[0] % len(sets)], res=res, epi=epi)
            ts = []
            for pin in (0, 1, 2):
                lib().emu_gemm_tune(pin << 28)
                ts.append(min(timeit(fn, a.iters) for _ in range(a.rounds)) * 1e6)
            lib().emu_gemm_tune(0)
            print(f"{name:16s} M={M:2d} " + " ".join(f"{t:8.1f}" for t in ts), flush=True)
        del sets
        torch.cuda.empty_cache()


MODES = {"bf16": lambda lm: None, "fp8 (5 rows on bf16)": lambda lm: lm.use_fp8(True), "fp8 wide": lambda lm: lm.use_fp8(True, wide=True),
         "fp4 wide": lambda lm: lm.use_fp4(True, wide=True)}


def beam_leg(a, dev):
    lcfg = LlamaCfg(num_hidden_layers=a.layers)
    lm = LlamaEngine(lcfg, VOCAB_EMU2_CHAT, EmuHipContext(dev))
    t0 = time.time()
    lm.load_weights(synth.iter_synth(synth.llama_param_shapes(lcfg, VOCAB_EMU2_CHAT), seed=0, device=dev, dtype=BF16))
    lm.quantize_fp8()
    lm.quantize_fp4()
    torch.cuda.synchronize()
    print(f"weights + fp8 + fp4 copies ready in {time.time() - t0:.0f}s, {torch.cuda.memory_allocated() / 2**30:.1f} GiB", flush=True)
    S, nb = a.prompt, 5
    g = torch.Generator().manual_seed(2)
    n0, n1 = a.short, a.long
    result = {}
    for prompts in (1, 4):
        x = (torch.randn(prompts, S, lcfg.hidden_size, generator=g) * 0.02).to(BF16).to(dev)
        mask = torch.ones(prompts, S, dtype=torch.long)

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
        times = {mode: [] for mode in MODES}
        for rnd in range(a.rounds):
            for mode, switch in MODES.items():
                switch(lm)
                times[mode].append(per_step())
                lm.use_fp8(False) if getattr(lm, "fp8_decode", False) else None
                lm.use_fp4(False) if getattr(lm, "fp4_decode", False) else None
                print(f"{prompts * nb} rows, round {rnd} {mode}: {times[mode][-1]:.3f} ms per step", flush=True)
        result[prompts * nb] = times
    return result, S


def windows(ts, scale=1e6, fmt="{:.1f}"):
    return fmt.format(min(ts) * scale) + " (" + " ".join(fmt.format(v * scale) for v in ts) + ")"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=770)
    ap.add_argument("--short", type=int, default=8)
    ap.add_argument("--long", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_wide.md"))
    ap.add_argument("--ab", action="store_true", help="only the rows-per-workgroup A/B (prints, writes nothing)")
    ap.add_argument("--skip", default="", help="comma list of legs to leave out: stream, beam")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fp8_wide_time.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    if a.ab:
        with torch.no_grad():
            ab_leg(a, dev)
        return
    skip = set(a.skip.split(","))
    out = ["# fp8 weights for 3..16-row steps on the matrix cores: measured against the bf16 and the MXFP4 few-row streams", "",
           f"Written by `tools/fp8_wide_time.py` ({torch.cuda.get_device_name(0)}; one process, so every comparison is same-run, same-box).",
           "Synthetic weights: **quality of per-row e4m3 weights on the real Emu2 checkpoint is not measured**.  The mode is opt-in",
           "(`LlamaEngine.use_fp8(True, wide=True)`).", ""]
    with torch.no_grad():
        if "stream" not in skip:
            wide = stream_leg(a, dev, (3, 5, 8, 16), ("bf16", "fp4", "fp8"))
            out += ["## Every weight stream on its own, 3 / 5 / 8 / 16 rows", "",
                    f"HIP events around {a.iters} launches, weights rotating through > 600 MB of copies, {a.rounds} windows per contender",
                    "alternating; us per launch: best window, all windows in brackets (their spread is the noise of the run).  bf16 = what",
                    "`ops.linear` launches (the thin LDS-DMA stream from 4 rows, the v_dot2c kernel at 3), fp4 = `gemv_fp4_thin.hip`, fp8 = the",
                    "new kernel.  HBM share = the new kernel's algorithmic weight bytes (N x K) / its best time / 8 TB/s.", "",
                    "| stream | N | K | rows | bf16 us | fp4 us | fp8 us | fp8 / bf16 | fp8 / fp4 | fp8 HBM share |", "|---|---|---|---|---|---|---|---|---|---|"]
            for name, N, K, M, t in wide:
                b, f4, f8 = min(t["bf16"]), min(t["fp4"]), min(t["fp8"])
                out.append(f"| {name} | {N} | {K} | {M} | {windows(t['bf16'])} | {windows(t['fp4'])} | {windows(t['fp8'])} | {f8 / b:.3f} | "
                           f"{f8 / f4:.3f} | {N * K / f8 / HBM:.3f} |")
            lose = [(r[0], r[3]) for r in wide if min(r[4]["fp8"]) >= min(r[4]["bf16"])]
            out += ["", "fp8 is not faster than bf16 at: " + (", ".join(f"{n} at {m} rows" for n, m in lose) if lose else "none of these cases") + ".", ""]
            narrow = stream_leg(a, dev, (2,), ("fp8 valu", "fp8"))
            out += ["## 2 rows: the VALU fp8 stream (`gemv_fp8_kernel`, no fused norm) against the matrix-core stream", "",
                    "Same method.  Reported only: 1..2 rows stay on the VALU stream, which also fuses the RMSNorm.", "",
                    "| stream | N | K | rows | VALU us | MFMA us | MFMA / VALU time |", "|---|---|---|---|---|---|---|"]
            for name, N, K, M, t in narrow:
                out.append(f"| {name} | {N} | {K} | {M} | {windows(t['fp8 valu'])} | {windows(t['fp8'])} | {min(t['fp8']) / min(t['fp8 valu']):.3f} |")
            out.append("")
        if "beam" not in skip:
            result, S = beam_leg(a, dev)
            out += [f"## A 5-beam step, {a.layers} layers at the LLaMA-33B shape, TP = 1", "",
                    f"Prompts of {S} rows, 5 beams; ms per step = (time of a {a.long}-token search - time of a {a.short}-token search) / {a.long - a.short},",
                    f"each search run once to warm up (graph capture) and once timed, host clock between device synchronisations, {a.rounds} windows",
                    "per mode alternating; best window, all windows in brackets.  20 rows = four prompts x five beams: past 16 rows every mode",
                    "but `use_fp4(..., all_rows=True)` reads the bf16 weights.", ""]
            for rows, times in result.items():
                b = min(times["bf16"])
                out += [f"### {rows} rows per step", "", "| mode | ms per step | time / bf16 |", "|---|---|---|"]
                out += [f"| {mode} | {windows(ts, 1.0, '{:.3f}')} | {min(ts) / b:.3f} |" for mode, ts in times.items()]
                out.append("")
            t5 = result[5]
            b, f = t5["bf16"], t5["fp8 wide"]
            spread = max(max(b) - min(b), max(f) - min(f))
            if min(b) - min(f) > spread:
                out += [f"The 5-beam step is **faster** with the few-row fp8 stream in this run: {min(f):.3f} ms against {min(b):.3f} ms "
                        f"(x{min(b) / min(f):.2f}); the windows of the two modes spread over at most {spread:.3f} ms.", ""]
            else:
                out += [f"**The 5-beam step is NOT below the bf16 one by more than the spread of the windows in this run: {min(f):.3f} ms against "
                        f"{min(b):.3f} ms, spread {spread:.3f} ms.**  The mode stays opt-in.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(out))
    print("\n".join(out))


if __name__ == "__main__":
    main()
