#!/usr/bin/env python
"""The MXFP4 GEMM for 17 rows and more (csrc/gemm_fp4.hip, ``use_fp4(True, wide=True, all_rows=True)``) against the bf16 path it
replaces, one process (needs a GPU):

    python tools/fp4_gemm_time.py [--layers 60] [--iters 20] [--rounds 2] [--skip shape,engine] [--out profiles/fp4_prefill.md]
    python tools/fp4_gemm_time.py --shards --out FILE.md   # leg 1 at 20 / 64 rows on the TP = 4 / 8 per-rank shapes, through
                                                           # ops.linear_fp4w_mfma (K = 896 / 2240 / 4480: a partial last K stage)

1. Every projection on its own at the LLaMA-33B widths, M = 20 / 64 / 770 / 1544 rows: ``ops.linear`` on bf16 weights against
   ``ops.linear_fp4w_gemm`` (HIP events, the weights rotating through more than 600 MB of copies, the contenders alternating).
2. One engine of --layers layers with synthetic weights: the whole prefill of 770 and of 1544 rows, bf16 (fused RoPE epilogue,
   K-slice sum + RMSNorm fusion: the default path) against mode 3; the 20-row 5-beam step of four prompts in mode 2 (bf16
   fallback) against mode 3; device memory before and after ``release_bf16()``.

Writes the tables to --out.  Synthetic weights: quality on a trained checkpoint is not measured here.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emu_amd import mxfp4, ops, synth  # noqa: E402
from emu_amd.conf.emu_conf import LlamaCfg  # noqa: E402
from emu_amd.constants import VOCAB_EMU2_CHAT  # noqa: E402
from emu_amd.llama import EmuHipContext, LlamaEngine  # noqa: E402

BF16 = torch.bfloat16
SHAPES = [("qkv", 19968, 6656, 0), ("o+res", 6656, 6656, 1), ("gateup+swiglu", 35840, 6656, 2), ("down+res", 6656, 17920, 1),
          ("lm_head", 32274, 6656, 0)]
# per-rank shapes of the 33B model at TP = 4 / 8 (emu_amd/tp.py): the row-parallel matrices' K is no multiple of 256 there
SHARD_SHAPES = [("o+res tp8", 6656, 896, 1), ("down+res tp8", 6656, 2240, 1), ("down+res tp4", 6656, 4480, 1), ("qkv tp8", 2688, 6656, 0),
                ("gateup+swiglu tp8", 4480, 6656, 2)]
ROWS = (20, 64, 770, 1544)


def timeit(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e-3


def shape_leg(a, dev):
    """rows: [name, N, K, M, bf16 us, fp4 us]"""
    out = []
    fp4_mfma = ops.linear_fp4w_mfma if a.shards else ops.linear_fp4w_gemm
    for name, N, K, epi in (SHARD_SHAPES if a.shards else SHAPES):
        n4 = max(1, int(600e6 // (N * K * 17 / 32)) + 1)
        nb = max(1, int(600e6 // (N * K * 2)) + 1)
        w4, wb = [], []
        for c in range(max(n4, nb)):
            w = (torch.randn(N, K, device=dev) * 0.02).to(BF16)
            if c < n4:
                q, sc = ops.quantize_mxfp4_rows(w)
                w4.append((q, mxfp4.pad_scales(sc, K) if a.shards else sc))   # scale rows at the kernels' stride once, not per launch
            if c < nb:
                wb.append(w)
            del w
        for M in (ROWS[:2] if a.shards else ROWS):
            xv = torch.randn(M, K, device=dev).to(BF16)
            res = torch.randn(M, N, device=dev).to(BF16) if epi == 1 else None
            i = [0]

            def new():
                i[0] += 1
                fp4_mfma(xv, *w4[i[0] % len(w4)], res=res, epi=epi)

            def other():
                i[0] += 1
                ops.linear(xv, wb[i[0] % len(wb)], res=res, epi=epi)
            t_new, t_other = [], []
            for _ in range(a.rounds):
                t_other.append(timeit(other, a.iters))
                t_new.append(timeit(new, a.iters))
            row = [name, N, K, M, min(t_other) * 1e6, min(t_new) * 1e6]
            print("shape", row, flush=True)
            out.append(row)
        del w4, wb
        torch.cuda.empty_cache()
    return out


def engine_leg(a, dev):
    lcfg = LlamaCfg(num_hidden_layers=a.layers)
    lm = LlamaEngine(lcfg, VOCAB_EMU2_CHAT, EmuHipContext(dev))
    t0 = time.time()
    lm.load_weights(synth.iter_synth(synth.llama_param_shapes(lcfg, VOCAB_EMU2_CHAT), seed=0, device=dev, dtype=BF16))
    lm.quantize_fp4()
    torch.cuda.synchronize()
    print(f"weights + fp4 copies ready in {time.time() - t0:.0f}s, {torch.cuda.memory_allocated() / 1e9:.2f} GB", flush=True)
    res = {"prefill": {}, "beam": {}}
    g = torch.Generator().manual_seed(2)
    modes = {"bf16": dict(enable=False), "mode 2": dict(enable=True, wide=True), "mode 3": dict(enable=True, wide=True, all_rows=True)}

    def switch(mode):
        lm.use_fp4(**modes[mode])
    # ---- whole prefill
    for S in (770, 1544):
        x = (torch.randn(1, S, lcfg.hidden_size, generator=g) * 0.02).to(BF16).to(dev)
        mask = torch.ones(1, S, dtype=torch.long)

        def run():
            lm.prefill(x, mask)
        times = {"bf16": [], "mode 3": []}
        for _ in range(a.rounds):
            for mode in times:
                switch(mode)
                times[mode].append(timeit(run, 3) * 1e3)
        res["prefill"][S] = times
        print("prefill", S, times, flush=True)
    # ---- 20-row 5-beam step: four prompts x five beams
    S, nb, n0, n1 = 64, 5, 6, 22
    x = (torch.randn(4, S, lcfg.hidden_size, generator=g) * 0.02).to(BF16).to(dev)
    mask = torch.ones(4, S, dtype=torch.long)

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
    times = {"mode 2": [], "mode 3": []}
    for _ in range(a.rounds):
        for mode in times:
            switch(mode)
            times[mode].append(per_step())
    res["beam"] = times
    print("20-row beam step", times, flush=True)
    # ---- memory
    switch("mode 3")
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    lm.release_bf16()
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated()
    fp4 = sum(t.numel() for pair in lm._fp4.values() for t in pair)
    res["mem"] = (before, after, fp4)
    x = (torch.randn(1, 770, lcfg.hidden_size, generator=g) * 0.02).to(BF16).to(dev)
    lm.prefill(x, torch.ones(1, 770, dtype=torch.long))      # still runs
    torch.cuda.synchronize()
    print("memory", res["mem"], flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp4_prefill.md"))
    ap.add_argument("--skip", default="", help="comma list of legs to leave out: shape, engine")
    ap.add_argument("--shards", action="store_true", help="only leg 1 at 20 / 64 rows, on the TP = 4 / 8 per-rank shapes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fp4_gemm_time.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    skip = set(a.skip.split(","))
    out = ["# MXFP4 GEMM for 17 rows and more (prefill, beams x batch): measured against the bf16 path", "",
           f"Written by `tools/fp4_gemm_time.py` ({torch.cuda.get_device_name(0)}; one process, so every comparison is same-run, same-box).",
           "Synthetic weights: **quality of round-to-nearest MXFP4 on the real Emu2 checkpoint is not measured**.  The mode is opt-in",
           "(`LlamaEngine.use_fp4(True, wide=True, all_rows=True)`).",
           f"Command: `python tools/fp4_gemm_time.py --layers {a.layers} --iters {a.iters} --rounds {a.rounds}"
           + (f" --skip {a.skip}" if a.skip else "") + "`.", ""]
    with torch.no_grad():
        if "shape" not in skip:
            rows = shape_leg(a, dev)
            out += ["## Every projection on its own: `ops.linear` on bf16 weights against `ops.linear_fp4w_gemm`", "",
                    f"HIP events around {a.iters} launches, weights rotating through > 600 MB of copies, {a.rounds} windows per contender",
                    "alternating, best window.", "",
                    "| projection | N | K | rows | bf16 us | fp4 us | fp4 / bf16 time |", "|---|---|---|---|---|---|---|"]
            for r in rows:
                out.append(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]} | {r[4]:.1f} | {r[5]:.1f} | {r[5] / r[4]:.3f} |")
            slow = [r for r in rows if r[3] <= 64 and r[5] > r[4]]
            out += ["", "At 20 and 64 rows (bound by the weight stream; after `release_bf16()` there is no bf16 to fall back to) the 4-bit GEMM is "
                    + ("not slower than bf16 on any of the five shapes." if not slow else
                       "**slower than bf16** at: " + ", ".join(f"{r[0]} M={r[3]} (x{r[5] / r[4]:.2f})" for r in slow) + "."), ""]
        if "engine" not in skip and not a.shards:
            res = engine_leg(a, dev)
            out += [f"## Whole prefill, {a.layers} layers at the LLaMA-33B shape, TP = 1", "",
                    "bf16 = the default path (RoPE / KV append / V^T in the qkv epilogue, K-slice sums with the RMSNorm); mode 3 = 4-bit GEMMs, unfused",
                    f"RoPE and norms.  HIP events around 3 prefills, {a.rounds} windows per contender alternating; best window, all windows in brackets.", "",
                    "| rows | bf16 ms | mode 3 ms | mode 3 / bf16 |", "|---|---|---|---|"]
            for S, t in res["prefill"].items():
                b, f = min(t["bf16"]), min(t["mode 3"])
                out.append(f"| {S} | {b:.1f} ({', '.join(f'{v:.1f}' for v in t['bf16'])}) | {f:.1f} ({', '.join(f'{v:.1f}' for v in t['mode 3'])}) | {f / b:.3f} |")
            t = res["beam"]
            b, f = min(t["mode 2"]), min(t["mode 3"])
            out += ["", "## The 20-row step: four prompts x five beams", "",
                    "ms per step = difference of two beam searches of different lengths (prefill and set-up cancel), graphs warmed up.", "",
                    "| mode | ms per 20-row step | windows |", "|---|---|---|",
                    f"| mode 2 (20 rows fall back to bf16) | {b:.3f} | {', '.join(f'{v:.3f}' for v in t['mode 2'])} |",
                    f"| mode 3 (4-bit GEMM) | {f:.3f} | {', '.join(f'{v:.3f}' for v in t['mode 3'])} |", "",
                    f"mode 3 / mode 2 = {f / b:.3f}.", ""]
            before, after, fp4 = res["mem"]
            out += ["## Device memory of the engine", "",
                    "| | GB (`torch.cuda.memory_allocated`) |", "|---|---|",
                    f"| mode 3, both weight sets resident | {before / 1e9:.2f} |", f"| after `release_bf16()` | {after / 1e9:.2f} |",
                    f"| of which 4-bit tensors | {fp4 / 1e9:.2f} |", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(out))
    print("\n".join(out))


if __name__ == "__main__":
    main()
