#!/usr/bin/env python
"""What the device loop of contrastive search costs and buys, one process, same box (needs a GPU):

    python tools/contrastive_time.py [--layers 60] [--prompt 770] [--short 8] [--long 24] [--out profiles/device_contrastive.md]

1. ms per step of contrastive search (penalty_alpha 0.6) at the LLaMA-33B shape with synthetic weights behind a 770-row prompt, for
   k = 4 and k = 8 candidates, B = 1 and B = 4 prompts: (a) the host loop of ``contrastive_generate``, run twice (its spread is the
   yardstick), (b) the device loop, eager launches, (c) the device loop replayed from a hipGraph.  Every leg is one whole call of
   ``contrastive_generate`` at two lengths; the step time is (t(long) - t(short)) / (long - short), so the prefill, the fan-out and a
   graph's capture drop out.  A host clock between device synchronisations; every leg is warmed by one short call first.
2. The three new kernels alone (HIP events over 100 back-to-back launches) at the context lengths 771 and 1026: pick (V = 32 274),
   score (both launches, H = 6656), keep (one slot of every layer of the cache the legs left behind).

Writes both tables to --out.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emu_amd import _lib, ops, synth  # noqa: E402
from emu_amd.conf.emu_conf import LlamaCfg  # noqa: E402
from emu_amd.constants import VOCAB_EMU2_CHAT  # noqa: E402
from emu_amd.llama import EmuHipContext, LlamaEngine  # noqa: E402

BF16 = torch.bfloat16
ALPHA, PAD, NO_EOS = 0.6, 32000, -1


def step_ms(lm, x, mask, k, short, long_, **kw):
    def run(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        lm.contrastive_generate(x, mask, n, ALPHA, k, eos_id=NO_EOS, pad_id=PAD, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t
    run(short)                                               # warm-up: allocations, lazy module loads
    a, b = run(short), run(long_)
    return (b - a) / (long_ - short) * 1e3


def events(fn, reps=100):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def kernels_alone(lm, dev, B, k, S):
    """Microseconds per launch of pick, score (two launches) and keep at a context of ``length`` rows."""
    L, V, H, out = _lib.lib(), lm.vocab, lm.cfg.hidden_size, []
    sm = ops.stream(dev)
    i32 = dict(dtype=torch.int32, device=dev)
    lg = (torch.randn(B * k, V, device=dev) * 3).to(BF16)
    cand = torch.randn(B * k, H, device=dev).to(BF16)
    ids, p = torch.zeros(B * k, **i32), torch.zeros(B * k, device=dev)
    sel, unf, kstart = torch.zeros(B, **i32), torch.ones(B, **i32), torch.zeros(B, **i32)
    hist, step = torch.zeros(4, B, **i32), torch.zeros(1, **i32)
    for length in (771, 1026):
        Lc = length + 4
        ctx = torch.nn.functional.normalize(torch.randn(B, Lc, H, device=dev), dim=2)
        ws = torch.empty(L.emu_contrastive_workspace_bytes(B, k, Lc), dtype=torch.uint8, device=dev)
        t_pick = events(lambda: L.emu_contrastive_pick_bf16(lg.data_ptr(), V, V, B, k, 4, sel.data_ptr(), hist.data_ptr(), B, step.data_ptr(),
                                                            1.0, NO_EOS, 0, ids.data_ptr(), p.data_ptr(), sm))
        t_score = events(lambda: L.emu_contrastive_score(ctx.data_ptr(), cand.data_ptr(), ids.data_ptr(), p.data_ptr(), kstart.data_ptr(),
                                                         step.data_ptr(), B, k, H, length, 4, Lc, ALPHA, 1.0 - ALPHA, NO_EOS, PAD,
                                                         hist.data_ptr(), unf.data_ptr(), sel.data_ptr(), None, ws.data_ptr(), ws.numel(), sm))
        # the cache of the legs: B * k rows; the slot's position does not change what moves
        t_keep = events(lambda: L.emu_llama_contrastive_keep_kv(lm.handle, sel.data_ptr(), step.data_ptr(), k, S, 4, sm))
        out.append((B, k, length, t_pick, t_score, t_keep))
        print(f"kernels B={B} k={k} context {length}: pick {t_pick:.1f} us, score {t_score:.1f} us, keep {t_keep:.1f} us", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--prompt", type=int, default=770)
    ap.add_argument("--short", type=int, default=8)
    ap.add_argument("--long", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lcfg = LlamaCfg(num_hidden_layers=a.layers)
    lm = LlamaEngine(lcfg, VOCAB_EMU2_CHAT, EmuHipContext(dev))
    t0 = time.time()
    lm.load_weights(synth.iter_synth(synth.llama_param_shapes(lcfg, VOCAB_EMU2_CHAT), seed=0, device=dev, dtype=BF16))
    torch.cuda.synchronize()
    print(f"{a.layers} layers ready in {time.time() - t0:.0f}s, {torch.cuda.memory_allocated() / 2**30:.1f} GiB", flush=True)
    lines = [f"## Contrastive search, {a.layers} layers at the LLaMA-33B shape, TP = 1, prompt {a.prompt}, penalty_alpha {ALPHA}", "",
             f"ms per step = (t({a.long} tokens) - t({a.short} tokens)) / {a.long - a.short}, whole calls of `contrastive_generate`.", "",
             "| B | k | host loop, 1st run | host loop, 2nd run | device loop, eager | device loop, hipGraph replay |", "|---|---|---|---|---|---|"]
    kern = []
    with torch.no_grad():
        for B in (1, 4):
            g = torch.Generator().manual_seed(2)
            x = (torch.randn(B, a.prompt, lcfg.hidden_size, generator=g) * 0.02).to(BF16).to(dev)
            mask = torch.ones(B, a.prompt, dtype=torch.long)
            for k in (4, 8):
                legs = [step_ms(lm, x, mask, k, a.short, a.long),
                        step_ms(lm, x, mask, k, a.short, a.long, device_contrastive=True),
                        step_ms(lm, x, mask, k, a.short, a.long, device_contrastive=True, use_graph=True),
                        step_ms(lm, x, mask, k, a.short, a.long)]
                print(f"B={B} k={k}: host {legs[0]:.3f} / {legs[3]:.3f}, device eager {legs[1]:.3f}, replay {legs[2]:.3f} ms/step", flush=True)
                lines.append(f"| {B} | {k} | {legs[0]:.3f} | {legs[3]:.3f} | {legs[1]:.3f} | {legs[2]:.3f} |")
                lm.prefill(x, mask, lm.kv_capacity(a.prompt + a.long))
                lm.fan_out_kv(B, k, a.prompt, lm.s_max)     # the legs' cache of B * k rows, for the keep launch
                kern += kernels_alone(lm, dev, B, k, a.prompt)
                lm.set_kv_share(0, 0)
    lines += ["", "## The new kernels alone (HIP events over 100 back-to-back launches, microseconds per launch)", "",
              "| B | k | context rows | pick (V = 32 274) | score, both launches (H = 6656) | keep (one slot, every layer) |", "|---|---|---|---|---|---|"]
    lines += [f"| {B} | {k} | {n} | {t1:.1f} | {t2:.1f} | {t3:.1f} |" for B, k, n, t1, t2, t3 in kern]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
