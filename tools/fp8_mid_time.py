#!/usr/bin/env python
"""The fp8 W8A16 GEMM for steps of 17..64 rows (csrc/gemm_fp8.hip, ``use_fp8(True, wide=True, mid=True)``) against what it replaces
and what stands next to it, one process (needs a GPU):

    python tools/fp8_mid_time.py [--layers 60] [--iters 20] [--rounds 3] [--skip shape,engine] [--out profiles/fp8_mid.md]
    python tools/fp8_mid_time.py --ab           # the narrow form's ring: 4 stages, one workgroup per CU / 2 stages, two (emu_gemm_tune bit 20); prints only

(a) Every projection on its own at the five LLaMA-33B shapes and 20 / 32 / 33 / 64 rows (HIP events, the weights rotating through
    more copies than the infinity cache holds, the contenders alternating in windows of one run): the new kernel, the bf16 GEMM
    (``ops.linear``), the W8A8 GEMM (``ops.linear_fp8`` on activations quantised beforehand: the per-row quantisation it needs in
    front is NOT in its time) and the 4-bit GEMM (``ops.linear_fp4w_gemm``).
(b) Steps at --layers layers behind a 770-row prompt, ms per step from the difference of two beam searches of different lengths
    (the prefill and the set-up cancel), windows alternating between the modes: the 20-row step of four prompts x five beams under
    bf16, fp8 mode 3 (``wide``), mode 5 (``wide, mid``) and ``use_fp4(True, wide=True, all_rows=True)``; the 5-row step of one prompt
    under modes 3 and 5, which must not differ.

Writes the tables to --out, every window next to the best one.  Synthetic weights: quality on a trained checkpoint is not measured.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from emu_amd import ops, synth  # noqa: E402
from emu_amd._lib import lib  # noqa: E402
from emu_amd.conf.emu_conf import LlamaCfg  # noqa: E402
from emu_amd.constants import VOCAB_EMU2_CHAT  # noqa: E402
from emu_amd.llama import EmuHipContext, LlamaEngine  # noqa: E402
from fp8_wide_time import BF16, HBM, SHAPES, timeit, weight_sets, windows  # noqa: E402

ROWS = (20, 32, 33, 64)
CONTENDERS = ("bf16", "w8a8", "fp4", "fp8")
TUNE_TWO_PER_CU = 1 << 20


def shape_leg(a, dev, rows_list=ROWS):
    """rows: [name, N, K, M, {contender: [window seconds]}]; the contenders' windows alternate."""
    out = []
    for name, N, K, epi in SHAPES:
        sets = weight_sets(N, K, dev, ["bf16", "fp8", "fp4"])
        for M in rows_list:
            xv = torch.randn(M, K, device=dev).to(BF16)
            x8, xs = ops.quantize_fp8_rows(xv)
            res = torch.randn(M, N, device=dev).to(BF16) if epi == 1 else None
            i = [0]

            def pick(kind):
                i[0] += 1
                return sets[kind][i[0] % len(sets[kind])]
            call = {"bf16": lambda: ops.linear(xv, *pick("bf16"), res=res, epi=epi),
                    "w8a8": lambda: ops.linear_fp8(x8, xs, *pick("fp8"), res=res, epi=epi),
                    "fp4": lambda: ops.linear_fp4w_gemm(xv, *pick("fp4"), res=res, epi=epi),
                    "fp8": lambda: ops.linear_fp8w_gemm(xv, *pick("fp8"), res=res, epi=epi)}
            t = {c: [] for c in CONTENDERS}
            for _ in range(a.rounds):
                for c in CONTENDERS:
                    t[c].append(timeit(call[c], a.iters))
            print("shape", name, N, K, M, {c: [round(v * 1e6, 1) for v in ts] for c, ts in t.items()}, flush=True)
            out.append([name, N, K, M, t])
        del sets
        torch.cuda.empty_cache()
    return out


def ab_leg(a, dev):
    print("fp8 W8A16 GEMM, narrow form, us per launch (best of the windows): ring 4, one workgroup per CU / ring 2, two per CU")
    for name, N, K, epi in SHAPES:
        sets = weight_sets(N, K, dev, ["fp8"])["fp8"]
        for M in (20, 32):
            xv = torch.randn(M, K, device=dev).to(BF16)
            res = torch.randn(M, N, device=dev).to(BF16) if epi == 1 else None
            i = [0]

            def fn():
                i[0] += 1
                ops.linear_fp8w_gemm(xv, *sets[i[0] % len(sets)], res=res, epi=epi)
            ts = {0: [], TUNE_TWO_PER_CU: []}
            for _ in range(a.rounds):
                for tune in ts:
                    lib().emu_gemm_tune(tune)
                    ts[tune].append(timeit(fn, a.iters) * 1e6)
            lib().emu_gemm_tune(0)
            print(f"{name:16s} M={M:2d} " + " / ".join(f"{min(v):8.1f} ({' '.join(f'{w:.1f}' for w in v)})" for v in ts.values()), flush=True)
        del sets
        torch.cuda.empty_cache()


def off(lm):
    if getattr(lm, "fp8_decode", False):
        lm.use_fp8(False)
    if getattr(lm, "fp4_decode", False):
        lm.use_fp4(False)


MODES20 = {"bf16": lambda lm: None, "fp8 mode 3 (wide)": lambda lm: lm.use_fp8(True, wide=True),
           "fp8 mode 5 (wide, mid)": lambda lm: lm.use_fp8(True, wide=True, mid=True),
           "fp4 all rows": lambda lm: lm.use_fp4(True, wide=True, all_rows=True)}
MODES5 = {k: MODES20[k] for k in ("fp8 mode 3 (wide)", "fp8 mode 5 (wide, mid)")}


def engine_leg(a, dev):
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
    for prompts, modes in ((4, MODES20), (1, MODES5)):
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
        times = {mode: [] for mode in modes}
        for rnd in range(a.rounds):
            for mode, switch in modes.items():
                switch(lm)
                times[mode].append(per_step())
                off(lm)
                print(f"{prompts * nb} rows, round {rnd} {mode}: {times[mode][-1]:.3f} ms per step", flush=True)
        result[prompts * nb] = times
    return result, S


def spread(*lists):
    return max(max(ts) - min(ts) for ts in lists)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=770)
    ap.add_argument("--short", type=int, default=8)
    ap.add_argument("--long", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_mid.md"))
    ap.add_argument("--ab", action="store_true", help="only the narrow form's ring-depth A/B (prints, writes nothing)")
    ap.add_argument("--skip", default="", help="comma list of legs to leave out: shape, engine")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fp8_mid_time.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    if a.ab:
        with torch.no_grad():
            ab_leg(a, dev)
        return
    skip = set(a.skip.split(","))
    out = ["# fp8 weights for 17..64-row steps: the W8A16 GEMM measured against the bf16, the W8A8 and the 4-bit GEMM", "",
           f"Written by `tools/fp8_mid_time.py` ({torch.cuda.get_device_name(0)}; one process, so every comparison is same-run, same-box).",
           "Synthetic weights: **quality of per-row e4m3 weights on the real Emu2 checkpoint is not measured**.  The mode is opt-in",
           "(`LlamaEngine.use_fp8(True, wide=True, mid=True)`).", ""]
    with torch.no_grad():
        if "shape" not in skip:
            rows = shape_leg(a, dev)
            out += ["## Every projection on its own, 20 / 32 / 33 / 64 rows", "",
                    f"HIP events around {a.iters} launches, weights rotating through > 600 MB of copies, {a.rounds} windows per contender",
                    "alternating; us per launch: best window, all windows in brackets (their spread is the noise of the run).  bf16 = what",
                    "`ops.linear` launches (the bf16 GEMM), W8A8 = `ops.linear_fp8` on activations quantised beforehand (the per-row",
                    "quantisation the engine runs in front of it is not in this time), fp4 = `gemm_fp4.hip`, fp8 = the new kernel.",
                    "HBM share = the new kernel's algorithmic weight bytes (N x K) / its best time / 8 TB/s.", "",
                    "| projection | N | K | rows | bf16 us | W8A8 us | fp4 us | fp8 us | fp8 / bf16 | fp8 / W8A8 | fp8 / fp4 | fp8 HBM share |",
                    "|---|---|---|---|---|---|---|---|---|---|---|---|"]
            lose = []
            for name, N, K, M, t in rows:
                b, w, f4, f8 = (min(t[c]) for c in CONTENDERS)
                out.append(f"| {name} | {N} | {K} | {M} | {windows(t['bf16'])} | {windows(t['w8a8'])} | {windows(t['fp4'])} | {windows(t['fp8'])} | "
                           f"{f8 / b:.3f} | {f8 / w:.3f} | {f8 / f4:.3f} | {N * K / f8 / HBM:.3f} |")
                if b - f8 <= spread(t["bf16"], t["fp8"]):
                    lose.append(f"{name} at {M} rows")
            out += ["", "**fp8 is not below the bf16 GEMM by more than the spread of the windows at: " + ", ".join(lose) + ".**" if lose else
                    "fp8 is below the bf16 GEMM by more than the spread of the windows in every one of these cases.", ""]
        if "engine" not in skip:
            result, S = engine_leg(a, dev)
            out += [f"## Beam-search steps, {a.layers} layers at the LLaMA-33B shape, TP = 1", "",
                    f"Prompts of {S} rows, 5 beams; ms per step = (time of a {a.long}-token search - time of a {a.short}-token search) / {a.long - a.short},",
                    f"each search run once to warm up (graph capture) and once timed, host clock between device synchronisations, {a.rounds} windows",
                    "per mode alternating; best window, all windows in brackets.  20 rows = four prompts x five beams; mode 3's 20-row step is",
                    "the behaviour before this kernel (bf16 weights past 16 rows).  5 rows = one prompt: modes 3 and 5 run the same kernels.", ""]
            for rows_, times in result.items():
                b = min(next(iter(times.values())))
                first = next(iter(times))
                out += [f"### {rows_} rows per step", "", f"| mode | ms per step | time / {first} |", "|---|---|---|"]
                out += [f"| {mode} | {windows(ts, 1.0, '{:.3f}')} | {min(ts) / b:.3f} |" for mode, ts in times.items()]
                out.append("")
            t3, t5 = result[20]["fp8 mode 3 (wide)"], result[20]["fp8 mode 5 (wide, mid)"]
            sp = spread(t3, t5)
            if min(t3) - min(t5) > sp:
                out += [f"The 20-row step is **faster** in mode 5 than in mode 3 in this run: {min(t5):.3f} ms against {min(t3):.3f} ms "
                        f"(x{min(t3) / min(t5):.2f}); the windows of the two modes spread over at most {sp:.3f} ms.", ""]
            else:
                out += [f"**The 20-row step in mode 5 is NOT below mode 3's by more than the spread of the windows in this run: {min(t5):.3f} ms "
                        f"against {min(t3):.3f} ms, spread {sp:.3f} ms.**", ""]
            s3, s5 = result[5]["fp8 mode 3 (wide)"], result[5]["fp8 mode 5 (wide, mid)"]
            sp = spread(s3, s5)
            out += [f"The 5-row step: mode 3 {min(s3):.3f} ms, mode 5 {min(s5):.3f} ms, spread of the windows {sp:.3f} ms -- " +
                    ("unchanged." if abs(min(s3) - min(s5)) <= sp else "**they differ by more than the spread.**"), ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(out))
    print("\n".join(out))


if __name__ == "__main__":
    main()
