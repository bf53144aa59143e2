#!/usr/bin/env python
"""LLaMA on the fp8 weights alone (``use_fp8(True, wide=True, mid=True, all_rows=True)``): the 65-rows-and-up form of the W8A16 GEMM
(csrc/gemm_fp8.hip, ``ops.linear_fp8w_tile``) against the bf16 path it replaces, one process (needs a GPU):

    python tools/fp8_all_time.py [--layers 60] [--iters 20] [--rounds 2] [--skip shape,engine] [--out profiles/fp8_all.md]

1. Every projection on its own at the LLaMA-33B widths, M = 65 / 128 / 300 / 770 rows: ``ops.linear`` on bf16 weights against
   ``ops.linear_fp8w_tile`` and, for the four layer shapes, the W8A8 GEMM ``ops.linear_fp8`` with the per-row quantisation of the
   activations in front of it, as the engine runs it (HIP events, the weights rotating through more than 600 MB of copies, the
   contenders alternating).
2. One engine of --layers layers with synthetic weights: the whole prefill of 770 and of 1544 rows under bf16 (fused RoPE epilogue,
   K-slice sum + RMSNorm fusion: the default path), mode 5 + all_rows and mode 6 + all_rows; the 80-row step of 16 prompts x 5 beams
   under bf16, mode 5 (80 rows fall back to bf16), mode 5 + all_rows and mode 6 + all_rows; device memory before and after
   ``release_bf16()``.

Writes the tables to --out.  Synthetic weights: quality on a trained checkpoint is not measured here.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emu_amd import ops, synth  # noqa: E402
from emu_amd.conf.emu_conf import LlamaCfg  # noqa: E402
from emu_amd.constants import VOCAB_EMU2_CHAT  # noqa: E402
from emu_amd.llama import EmuHipContext, LlamaEngine  # noqa: E402

BF16 = torch.bfloat16
SHAPES = [("qkv", 19968, 6656, 0), ("o+res", 6656, 6656, 1), ("gateup+swiglu", 35840, 6656, 2), ("down+res", 6656, 17920, 1),
          ("lm_head", 32274, 6656, 0)]
ROWS = (65, 128, 300, 770)
ALL = dict(wide=True, mid=True, all_rows=True)


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
    """rows: [name, N, K, M, bf16 us, W8A16 tile us, W8A8 us or None]"""
    out = []
    for name, N, K, epi in SHAPES:
        n8 = max(1, int(600e6 // (N * K)) + 1)
        nb = max(1, int(600e6 // (N * K * 2)) + 1)
        w8, wb = [], []
        for c in range(max(n8, nb)):
            w = (torch.randn(N, K, device=dev) * 0.02).to(BF16)
            if c < n8:
                w8.append(ops.quantize_fp8_rows(w))
            if c < nb:
                wb.append(w)
            del w
        for M in ROWS:
            xv = torch.randn(M, K, device=dev).to(BF16)
            res = torch.randn(M, N, device=dev).to(BF16) if epi == 1 else None
            i = [0]

            def tile():
                i[0] += 1
                ops.linear_fp8w_tile(xv, *w8[i[0] % len(w8)], res=res, epi=epi)

            def w8a8():
                i[0] += 1
                x8, xs = ops.quantize_fp8_rows(xv)               # per row, ahead of every GEMM: what the engine's W8A8 prefill does
                ops.linear_fp8(x8, xs, *w8[i[0] % len(w8)], res=res, epi=epi)

            def bf16():
                i[0] += 1
                ops.linear(xv, wb[i[0] % len(wb)], res=res, epi=epi)
            contenders = {"bf16": bf16, "tile": tile}
            if name != "lm_head":                                # the head has no W8A8 GEMM in the engine
                contenders["w8a8"] = w8a8
            t = {k: [] for k in contenders}
            for _ in range(a.rounds):
                for k, fn in contenders.items():
                    t[k].append(timeit(fn, a.iters))
            row = [name, N, K, M, min(t["bf16"]) * 1e6, min(t["tile"]) * 1e6, min(t["w8a8"]) * 1e6 if "w8a8" in t else None]
            print("shape", row, flush=True)
            out.append(row)
        del w8, wb
        torch.cuda.empty_cache()
    return out


def engine_leg(a, dev):
    lcfg = LlamaCfg(num_hidden_layers=a.layers)
    lm = LlamaEngine(lcfg, VOCAB_EMU2_CHAT, EmuHipContext(dev))
    t0 = time.time()
    lm.load_weights(synth.iter_synth(synth.llama_param_shapes(lcfg, VOCAB_EMU2_CHAT), seed=0, device=dev, dtype=BF16))
    lm.quantize_fp8()
    torch.cuda.synchronize()
    print(f"weights + fp8 copies ready in {time.time() - t0:.0f}s, {torch.cuda.memory_allocated() / 1e9:.2f} GB", flush=True)
    res = {"prefill": {}, "beam": {}}
    g = torch.Generator().manual_seed(2)
    modes = {"bf16": dict(enable=False), "mode 5": dict(enable=True, wide=True, mid=True), "mode 5 + all_rows": dict(enable=True, **ALL),
             "mode 6 + all_rows": dict(enable=True, prefill=True, **ALL)}

    def switch(mode):
        lm.use_fp8(**modes[mode])
    # ---- whole prefill
    for S in (770, 1544):
        x = (torch.randn(1, S, lcfg.hidden_size, generator=g) * 0.02).to(BF16).to(dev)
        mask = torch.ones(1, S, dtype=torch.long)

        def run():
            lm.prefill(x, mask)
        times = {"bf16": [], "mode 5 + all_rows": [], "mode 6 + all_rows": []}
        for _ in range(a.rounds):
            for mode in times:
                switch(mode)
                times[mode].append(timeit(run, 3) * 1e3)
        res["prefill"][S] = times
        print("prefill", S, times, flush=True)
    # ---- 80-row step: 16 prompts x five beams
    S, nb, n0, n1 = 64, 5, 6, 22
    x = (torch.randn(16, S, lcfg.hidden_size, generator=g) * 0.02).to(BF16).to(dev)
    mask = torch.ones(16, S, dtype=torch.long)

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
    times = {m: [] for m in modes}
    for _ in range(a.rounds):
        for mode in times:
            switch(mode)
            times[mode].append(per_step())
    res["beam"] = times
    print("80-row beam step", times, flush=True)
    # ---- memory
    switch("mode 5 + all_rows")
    lm.release_kv()                                  # the KV caches of the legs above (16 x 5 beam rows: tens of GB) are not the weights'
    lm._ws = None
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    lm.release_bf16()
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated()
    fp8 = sum(t.numel() * t.element_size() for pair in lm._fp8.values() for t in pair)
    res["mem"] = (before, after, fp8, lm.embed.numel() * lm.embed.element_size())
    x = (torch.randn(1, 770, lcfg.hidden_size, generator=g) * 0.02).to(BF16).to(dev)
    for mode in ("mode 5 + all_rows", "mode 6 + all_rows"):  # still runs, either way
        switch(mode)
        lm.prefill(x, torch.ones(1, 770, dtype=torch.long))
    torch.cuda.synchronize()
    print("memory", res["mem"], flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_all.md"))
    ap.add_argument("--skip", default="", help="comma list of legs to leave out: shape, engine")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fp8_all_time.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    skip = set(a.skip.split(","))
    out = ["# LLaMA on the fp8 weights alone: the W8A16 GEMM for 65 rows and more, measured against the bf16 path", "",
           f"Written by `tools/fp8_all_time.py` ({torch.cuda.get_device_name(0)}; one process, so every comparison is same-run, same-box).",
           "Synthetic weights: **quality of per-row-scaled e4m3 on the real Emu2 checkpoint is not measured**.  The mode is opt-in",
           "(`LlamaEngine.use_fp8(True, wide=True, mid=True, all_rows=True)`, with or without `prefill=True`).",
           f"Command: `python tools/fp8_all_time.py --layers {a.layers} --iters {a.iters} --rounds {a.rounds}"
           + (f" --skip {a.skip}" if a.skip else "") + "`.", ""]
    with torch.no_grad():
        if "shape" not in skip:
            rows = shape_leg(a, dev)
            out += ["## Every projection on its own: `ops.linear` on bf16 weights against `ops.linear_fp8w_tile` and the W8A8 GEMM", "",
                    f"HIP events around {a.iters} launches, weights rotating through > 600 MB of copies, {a.rounds} windows per contender",
                    "alternating, best window.  W8A8 = `ops.quantize_fp8_rows` of the activations + `ops.linear_fp8`, as the engine's fp8 prefill runs",
                    "a layer projection; the head has no W8A8 GEMM.", "",
                    "| projection | N | K | rows | bf16 us | W8A16 tile us | W8A8 us | tile / bf16 time | tile / W8A8 time |", "|---|---|---|---|---|---|---|---|---|"]
            for r in rows:
                w = f"{r[6]:.1f}" if r[6] is not None else "-"
                out.append(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]} | {r[4]:.1f} | {r[5]:.1f} | {w} | {r[5] / r[4]:.3f} | "
                           + (f"{r[5] / r[6]:.3f}" if r[6] is not None else "-") + " |")
            slow = [r for r in rows if r[5] > r[4]]
            out += ["", "The W8A16 tile is " + ("not slower than bf16 on any of the shapes and row counts." if not slow else
                                               "**slower than bf16** at: " + ", ".join(f"{r[0]} M={r[3]} (x{r[5] / r[4]:.2f})" for r in slow) + "."), ""]
        if "engine" not in skip:
            res = engine_leg(a, dev)
            out += [f"## Whole prefill, {a.layers} layers at the LLaMA-33B shape, TP = 1", "",
                    "bf16 = the default path (RoPE / KV append / V^T in the qkv epilogue, K-slice sums with the RMSNorm); mode 5 + all_rows = the W8A16",
                    "tile in every projection, unfused RoPE and norms; mode 6 + all_rows = W8A8 GEMMs in the layers (the head is not part of a prefill).",
                    f"HIP events around 3 prefills, {a.rounds} windows per contender alternating; best window, all windows in brackets.", "",
                    "| rows | bf16 ms | mode 5 + all_rows ms | mode 6 + all_rows ms | mode 5 / bf16 | mode 6 / bf16 |", "|---|---|---|---|---|---|"]
            for S, t in res["prefill"].items():
                b, f5, f6 = (min(t[k]) for k in ("bf16", "mode 5 + all_rows", "mode 6 + all_rows"))
                cell = lambda k: f"{min(t[k]):.1f} ({', '.join(f'{v:.1f}' for v in t[k])})"
                out.append(f"| {S} | {cell('bf16')} | {cell('mode 5 + all_rows')} | {cell('mode 6 + all_rows')} | {f5 / b:.3f} | {f6 / b:.3f} |")
            t = res["beam"]
            b = min(t["bf16"])
            out += ["", "## The 80-row step: 16 prompts x five beams", "",
                    "ms per step = difference of two beam searches of different lengths (prefill and set-up cancel), graphs warmed up.", "",
                    "| mode | ms per 80-row step | windows | / bf16 |", "|---|---|---|---|"]
            for k, note in (("bf16", ""), ("mode 5", " (80 rows fall back to bf16)"), ("mode 5 + all_rows", " (W8A16 tile)"),
                            ("mode 6 + all_rows", " (W8A8 layers, W8A16 tile head)")):
                out.append(f"| {k}{note} | {min(t[k]):.3f} | {', '.join(f'{v:.3f}' for v in t[k])} | {min(t[k]) / b:.3f} |")
            before, after, fp8, emb = res["mem"]
            out += ["", "## Device memory of the engine", "",
                    "KV caches and workspace released first (`release_kv()`), so the figures are the weights': bf16 matrices, their 13-bit packed",
                    "sets (o_proj and down_proj, packed at load; `release_bf16()` drops them with the bf16 rows), the fp8 set, the embedding.", "",
                    "| | GB (`torch.cuda.memory_allocated`) |", "|---|---|",
                    f"| mode 5 + all_rows, both weight sets resident | {before / 1e9:.2f} |", f"| after `release_bf16()` | {after / 1e9:.2f} |",
                    f"| of which fp8 tensors and their row scales | {fp8 / 1e9:.2f} |", f"| of which the bf16 embedding | {emb / 1e9:.2f} |", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(out))
    print("\n".join(out))


if __name__ == "__main__":
    main()
