#!/usr/bin/env python
"""The MXFP4 decode stream against the bf16 and fp8 streams, one process, same box (needs a GPU):

    python tools/fp4_time.py [--layers 60] [--steps 64] [--warmup 8] [--out profiles/fp4_decode.md]

1. ms/token of a greedy decode at the LLaMA-33B shape with synthetic weights (the bench's flagship workload and its timing
   discipline: hipGraph-replayed steps, a host clock between device synchronisations, warm-up first), the three streams
   alternating so that clock and neighbours hit all of them alike; only the same-run ratios count.
2. Every weight stream on its own (HIP events, the weights rotating through more copies than the infinity cache holds): time and
   algorithmic bytes over time as a fraction of the 8 TB/s HBM peak, for the four layer shapes and the head.
3. The teacher-forced logit comparison of tests/test_gpu_fp4.py (h) on the tiny fixture.

Writes the three tables to --out.  Quality on a trained checkpoint is not measured here (synthetic weights).
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
from emu_amd.llama import EmuHipContext, GreedyState, LlamaEngine  # noqa: E402

BF16 = torch.bfloat16
HBM = 8.0e12
MODES = ("bf16", "fp8", "fp4")


def set_mode(lm, mode):
    if getattr(lm, "fp8_decode", False):
        lm.use_fp8(False)
    if getattr(lm, "fp4_decode", False):
        lm.use_fp4(False)
    if mode == "fp8":
        lm.use_fp8(True)
    elif mode == "fp4":
        lm.use_fp4(True)


def decode_leg(a, dev):
    lcfg = LlamaCfg(num_hidden_layers=a.layers)
    lm = LlamaEngine(lcfg, VOCAB_EMU2_CHAT, EmuHipContext(dev))
    t0 = time.time()
    lm.load_weights(synth.iter_synth(synth.llama_param_shapes(lcfg, VOCAB_EMU2_CHAT), seed=0, device=dev, dtype=BF16))
    lm.quantize_fp8()
    lm.quantize_fp4()
    torch.cuda.synchronize()
    print(f"weights + fp8 + fp4 copies ready in {time.time() - t0:.0f}s, {torch.cuda.memory_allocated() / 2**30:.1f} GiB", flush=True)
    S = a.prompt
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(1, S, lcfg.hidden_size, generator=g) * 0.02).to(BF16).to(dev)
    mask = torch.ones(1, S, dtype=torch.long)
    total = a.warmup + a.steps + 8
    s_max = lm.kv_capacity(S + total + 8)
    lm.alloc_kv(1, s_max)
    hidden, kstart, next_pos = lm.prefill(x, mask, s_max)
    cur = ops.argmax(lm.logits(hidden[:, -1, :]), suppress_id=2)
    out_ids = torch.zeros(total + 1, 1, device=dev, dtype=torch.int32)
    st = GreedyState(lm, 1, cur, next_pos, S, kstart, out_ids)
    bytes_tok, times = {}, {m: [] for m in MODES}
    for rnd in range(a.rounds):
        for mode in MODES:
            set_mode(lm, mode)
            bytes_tok[mode] = lm.weight_bytes_per_token()
            st.reset(cur, next_pos, S)
            for _ in range(a.warmup):
                st.step_graph()
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.steps):
                st.step_graph()
            torch.cuda.synchronize()
            times[mode].append((time.perf_counter() - t) / a.steps * 1e3)
            print(f"round {rnd} {mode}: {times[mode][-1]:.3f} ms/token", flush=True)
    set_mode(lm, "bf16")
    return {m: (min(times[m]), times[m], bytes_tok[m]) for m in MODES}, S


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


def gemv_leg(a, dev):
    """(name, N, K, epi, norm) x the three formats, one row of activations."""
    shapes = [("qkv+norm", 19968, 6656, 0, True), ("o+res", 6656, 6656, 1, False), ("gateup+norm+swiglu", 35840, 6656, 2, True),
              ("down+res", 6656, 17920, 1, False), ("lm_head+norm", 32274, 6656, 0, True),
              ("tp8 o+res", 6656, 896, 1, False), ("tp8 down+res", 6656, 2240, 1, False)]
    rows = []
    for name, N, K, epi, norm in shapes:
        xv = torch.randn(1, K, device=dev).to(BF16)
        res = torch.randn(1, N, device=dev).to(BF16) if epi == 1 else None
        gain = torch.randn(K, device=dev).to(BF16) if norm else None
        row = [name, N, K]
        for mode in MODES:
            per_w = {"bf16": 2.0, "fp8": 1.0, "fp4": 17.0 / 32.0}[mode]
            n_copy = max(1, int(600e6 // (N * K * per_w)) + 1)
            ws = []
            for _ in range(n_copy):
                w = (torch.randn(N, K, device=dev) * 0.02).to(BF16)
                ws.append(w if mode == "bf16" else ops.quantize_fp8_rows(w) if mode == "fp8" else ops.quantize_mxfp4_rows(w))
            del w
            i = [0]

            def fn():
                i[0] = (i[0] + 1) % n_copy
                if mode == "bf16":
                    ops.linear(xv, ws[i[0]], res=res, norm_w=gain, eps=1e-6, epi=epi)
                elif mode == "fp8":
                    ops.linear_fp8w(xv, *ws[i[0]], res=res, norm_w=gain, eps=1e-6, epi=epi)
                else:
                    ops.linear_fp4w(xv, *ws[i[0]], res=res, norm_w=gain, eps=1e-6, epi=epi)
            t = timeit(fn, a.iters)
            row += [t * 1e6, N * K * per_w / t / HBM]
            del ws
            torch.cuda.empty_cache()
        print("gemv", row, flush=True)
        rows.append(row)
    return rows


def ab_leg(a, dev):
    """The fp4 stream's launch geometry A/B (emu_gemm_tune bits 24-27): row sets per workgroup x weight rows per lane."""
    from emu_amd._lib import lib
    shapes = [("qkv+norm", 19968, 6656, 0, True), ("o+res", 6656, 6656, 1, False), ("gateup+norm+swiglu", 35840, 6656, 2, True),
              ("down+res", 6656, 17920, 1, False), ("lm_head+norm", 32274, 6656, 0, True)]
    combos = [(rs, r) for rs in (0, 1, 2, 3) for r in (1, 2)]
    print("fp4 geometry A/B, us per launch; columns: " + " ".join(f"sets{[0, 1, 2, 4][rs] or 'auto'}/rows{4 * r}" for rs, r in combos))
    for name, N, K, epi, norm in shapes:
        xv = torch.randn(1, K, device=dev).to(BF16)
        res = torch.randn(1, N, device=dev).to(BF16) if epi == 1 else None
        gain = torch.randn(K, device=dev).to(BF16) if norm else None
        n_copy = max(1, int(600e6 // (N * K * 17 / 32)) + 1)
        ws = [ops.quantize_mxfp4_rows((torch.randn(N, K, device=dev) * 0.02).to(BF16)) for _ in range(n_copy)]
        i = [0]

        def fn():
            i[0] = (i[0] + 1) % n_copy
            ops.linear_fp4w(xv, *ws[i[0]], res=res, norm_w=gain, eps=1e-6, epi=epi)
        ts = []
        for rs, r in combos:
            lib().emu_gemm_tune((rs << 24) | (r << 26))
            ts.append(timeit(fn, a.iters) * 1e6)
        lib().emu_gemm_tune(0)
        print(f"{name:22s} " + " ".join(f"{t:8.1f}" for t in ts), flush=True)
        del ws
        torch.cuda.empty_cache()


def accuracy_leg():
    from tests import tiny
    from tests.test_gpu_fp4 import _tiny_model, fp4_vs_bf16_teacher_forced
    golden = os.path.join(ROOT, "tests", "golden")
    m, *_ = _tiny_model(golden)
    zm = tiny.load(golden, "generate_margin_tiny.npz")
    ids, mask = torch.from_numpy(zm["pen_ids"]), torch.from_numpy(zm["pen_mask"])
    rel, agree, margin, change = fp4_vs_bf16_teacher_forced(m, ids, mask, 8)
    lm = m.decoder.lm
    werr = []
    for key in ("0.wqkv", "0.wo", "0.wgu", "0.wdown", "lm_head"):
        src = (lm.lm_head if key == "lm_head" else lm._keep[key]).float()
        werr.append((key, float((lm.fp4_dequantized(key) - src).norm() / src.norm())))
    return rel, agree, margin, change, werr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--prompt", type=int, default=770)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp4_decode.md"))
    ap.add_argument("--ab", action="store_true", help="only the launch-geometry A/B of the fp4 stream (prints, writes nothing)")
    ap.add_argument("--skip", default="", help="comma list of legs to leave out: decode, gemv, accuracy")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fp4_time.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    if a.ab:
        with torch.no_grad():
            ab_leg(a, dev)
        return
    skip = set(a.skip.split(","))
    out = ["# MXFP4 decode stream: measured against the bf16 and fp8 streams", "",
           f"Written by `tools/fp4_time.py` ({torch.cuda.get_device_name(0)}; one process, so every comparison is same-run, same-box).",
           "Synthetic weights: **quality of round-to-nearest MXFP4 on the real Emu2 checkpoint is not measured** -- the logits of a",
           "random-init model say nothing about a trained one.  The mode is opt-in (`LlamaEngine.use_fp4`).", ""]
    with torch.no_grad():
        if "accuracy" not in skip:
            rel, agree, margin, change, werr = accuracy_leg()
            out += ["## Teacher-forced logits, fp4 stream against the bf16 stream (tiny fixture, tests/test_gpu_fp4.py (h))", "",
                    "Prompts `pen_ids` of `tests/golden/generate_margin_tiny.npz` (2 rows), the bf16 run's greedy tokens fed to both streams;",
                    "prefill is bf16 in both, so step 0 differs by the head alone.", "",
                    "| step | " + " | ".join(str(i) for i in range(len(rel))) + " |", "|---|" + "---|" * len(rel),
                    "| relative L2 of the logits | " + " | ".join(f"{r:.4f}" for r in rel) + " |",
                    "| arg-max agrees (rows) | " + " | ".join(f"{int(agree[:, i].sum())}/{agree.shape[0]}" for i in range(len(rel))) + " |", "",
                    f"Arg-max agreement {int(agree.sum())} of {agree.numel()}; decisions that flip although the bf16 top-2 margin exceeds the row's",
                    f"largest logit change: {int((~((margin <= change) | agree)).sum())} (the test asserts 0).  Weight round-trip error (relative L2,",
                    "packed tiny matrices): " + ", ".join(f"`{k}` {e:.3f}" for k, e in werr) + ".", ""]
        if "decode" not in skip:
            res, S = decode_leg(a, dev)
            torch.cuda.empty_cache()
            out += [f"## Greedy decode, {a.layers} layers at the LLaMA-33B shape, TP = 1", "",
                    f"Prompt of {S} rows, {a.warmup} warm-up + {a.steps} timed hipGraph-replayed steps per window, host clock between device",
                    f"synchronisations, {a.rounds} windows per stream, the streams alternating; best window, all windows in brackets.", "",
                    "| stream | ms/token | windows | weight bytes/token | bytes / bf16 | time / bf16 | time / fp8 |", "|---|---|---|---|---|---|---|"]
            for mode in MODES:
                t, allt, b = res[mode]
                out.append(f"| {mode} | {t:.3f} | {', '.join(f'{v:.3f}' for v in allt)} | {b / 1e9:.2f} GB | {b / res['bf16'][2]:.3f} | "
                           f"{t / res['bf16'][0]:.3f} | {t / res['fp8'][0]:.3f} |")
            verdict = "faster" if res["fp4"][0] < res["fp8"][0] else "NOT faster"
            out += ["", f"The fp4 stream is **{verdict}** per token than the fp8 stream in this run "
                    f"({res['fp4'][0]:.3f} vs {res['fp8'][0]:.3f} ms; bf16 {res['bf16'][0]:.3f} ms).  A step is not weight bytes alone: decode attention,",
                    "the residual / norm traffic and the launches themselves do not shrink with the weights.", ""]
        if "gemv" not in skip:
            rows = gemv_leg(a, dev)
            out += ["## Every weight stream on its own (one row of activations)", "",
                    f"HIP events around {a.iters} launches, weights rotating through > 600 MB of copies; fraction = algorithmic weight bytes",
                    "(bf16 2, fp8 1, fp4 17/32 per weight) / time / 8 TB/s.", "",
                    "| stream | N | K | bf16 us | frac | fp8 us | frac | fp4 us | frac | fp4 / fp8 time |", "|---|---|---|---|---|---|---|---|---|---|"]
            for r in rows:
                out.append(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]:.1f} | {r[4]:.3f} | {r[5]:.1f} | {r[6]:.3f} | {r[7]:.1f} | {r[8]:.3f} | {r[7] / r[5]:.3f} |")
            out.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print("\n".join(out))


if __name__ == "__main__":
    main()
