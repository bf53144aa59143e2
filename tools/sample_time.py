#!/usr/bin/env python
"""What the device sampler costs and buys, one process, same box (needs a GPU):

    python tools/sample_time.py [--layers 60] [--steps 48] [--warmup 8] [--rounds 3] [--out profiles/device_sampler.md]

1. ms/token of sampled decoding (temperature 0.7, top_p 0.9: the chat demo's defaults) at the LLaMA-33B shape with synthetic
   weights, B = 1 and B = 4: (a) the host-driven loop of ``sample_generate``, (b) the device loop, eager launches, (c) the device loop
   replayed from a hipGraph -- and the greedy step of the same run (eager and replayed) as the floor.  The legs alternate inside every
   round so that clock and neighbours hit all of them alike; a host clock between device synchronisations, warm-up first; the median
   over the rounds is reported with the spread.
2. The sample kernel alone (HIP events around a batch of launches, V = 32 274) for 1, 5 and 64 rows, next to the ``argmax_kernel``
   launch it stands beside in the step.

Writes both tables to --out.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emu_amd import ops, synth  # noqa: E402
from emu_amd.conf.emu_conf import LlamaCfg  # noqa: E402
from emu_amd.constants import VOCAB_EMU2_CHAT  # noqa: E402
from emu_amd.llama import (EmuHipContext, GreedyState, LlamaEngine, SampleState, process_logits,  # noqa: E402
                           sample_params)

BF16 = torch.bfloat16
OPTS = dict(temperature=0.7, top_p=0.9)
PAD, NO_EOS = 32000, -1


def host_loop(lm, row, pos, kstart, S, B, n):
    """The per-token body of ``LlamaEngine.sample_generate``'s host path (no EOS in reach), n tokens."""
    dev = lm.device
    out = torch.full((B, n), PAD, dtype=torch.int64, device=dev)
    unfinished = torch.ones(B, dtype=torch.int64, device=dev)
    hid = torch.empty(B, lm.cfg.hidden_size, device=dev, dtype=BF16)
    for step in range(n):
        scores = process_logits(lm.logits(row).float(), out[:, :step], False, NO_EOS, True, OPTS["temperature"], None, OPTS["top_p"])
        nxt = torch.multinomial(torch.softmax(scores, dim=-1), num_samples=1).squeeze(1)
        nxt = nxt * unfinished + PAD * (1 - unfinished)
        out[:, step] = nxt
        unfinished = unfinished * (nxt != NO_EOS).long()
        if int(unfinished.max().item()) == 0:
            break
        ops.embed_gather(nxt.to(torch.int32).contiguous(), lm.embed, out=hid)
        lm.forward(hid, B, 1, pos, torch.full((B,), S + step, device=dev, dtype=torch.int32), kstart, ctx=S + step + 1)
        pos, row = pos + 1, hid


def decode_legs(a, dev, lm, B):
    S, n = a.prompt, a.warmup + a.steps
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(B, S, lm.cfg.hidden_size, generator=g) * 0.02).to(BF16).to(dev)
    mask = torch.ones(B, S, dtype=torch.long)
    s_max = lm.kv_capacity(S + n + 8)
    hidden, kstart, next_pos = lm.prefill(x, mask, s_max)
    row0 = hidden[:, -1, :].clone()
    cur = ops.argmax(lm.logits(row0), suppress_id=2)
    gs = GreedyState(lm, B, cur, next_pos, S, kstart, torch.zeros(n + 2, B, device=dev, dtype=torch.int32))
    uni = torch.rand(n + 2, B, device=dev)
    ss = SampleState(lm, B, next_pos, S, kstart, torch.full((n + 2, B), PAD, device=dev, dtype=torch.int32), uni,
                     sample_params(True, OPTS["temperature"], None, OPTS["top_p"], 1.0, None, 0, NO_EOS, PAD))

    def reset_sample():
        ss.pos.copy_(next_pos); ss.slot.fill_(S); ss.ctx.fill_(S + 1); ss.step_idx.zero_(); ss.unfinished.fill_(1)
        lm.logits(row0, out=ss.logits)
        ss.first()

    def timed(step_fn, reset):
        reset()
        for _ in range(a.warmup):
            step_fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(a.steps - 1):
            step_fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / (a.steps - 1) * 1e3

    def host():
        torch.cuda.synchronize()
        t = time.perf_counter()
        host_loop(lm, row0, next_pos.clone(), kstart, S, B, a.steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / a.steps * 1e3

    legs = {
        "host loop (sample_generate as it is)": host,
        "device loop, eager": lambda: timed(ss.step, reset_sample),
        "device loop, hipGraph replay": lambda: timed(ss.step_graph, reset_sample),
        "greedy step, eager (floor)": lambda: timed(gs.step, lambda: gs.reset(cur, next_pos, S)),
        "greedy step, hipGraph replay (floor)": lambda: timed(gs.step_graph, lambda: gs.reset(cur, next_pos, S)),
    }
    host_loop(lm, row0, next_pos.clone(), kstart, S, B, 4)            # warm the torch ops of the host path
    times = {k: [] for k in legs}
    for rnd in range(a.rounds):
        for k, fn in legs.items():
            times[k].append(fn())
            print(f"B={B} round {rnd} {k}: {times[k][-1]:.3f} ms/token", flush=True)
    return times


def kernel_leg(dev, reps=200):
    V, rows_out = VOCAB_EMU2_CHAT, []
    par = sample_params(True, OPTS["temperature"], None, OPTS["top_p"], 1.0, None, 0, NO_EOS, PAD)
    par_k = sample_params(True, OPTS["temperature"], 50, OPTS["top_p"], 1.3, None, 0, NO_EOS, PAD)
    for R in (1, 5, 64):
        x = (torch.randn(R, V, generator=torch.Generator().manual_seed(R)) * 3).to(BF16).to(dev)
        step = torch.tensor([8], dtype=torch.int32, device=dev)
        hist = torch.randint(0, V, (16, R), dtype=torch.int32, device=dev)
        uni = torch.rand(16, R, device=dev)
        out = torch.empty(R, dtype=torch.int32, device=dev)

        def ev(fn):
            for _ in range(20):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps * 1e3

        rows_out.append((R, ev(lambda: ops.sample(x, step, par, out, uniforms=uni)),
                         ev(lambda: ops.sample(x, step, par_k, out, hist=hist, uniforms=uni)),
                         ev(lambda: ops.argmax(x, out=out))))
        print(f"kernel rows={R}: top-p {rows_out[-1][1]:.1f} us, penalty + top-k + top-p {rows_out[-1][2]:.1f} us, "
              f"argmax {rows_out[-1][3]:.1f} us", flush=True)
    return rows_out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--layers", type=int, default=60)
    p.add_argument("--steps", type=int, default=48)
    p.add_argument("--warmup", type=int, default=8)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--prompt", type=int, default=512)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    lcfg = LlamaCfg(num_hidden_layers=a.layers)
    lm = LlamaEngine(lcfg, VOCAB_EMU2_CHAT, EmuHipContext(dev))
    t0 = time.time()
    lm.load_weights(synth.iter_synth(synth.llama_param_shapes(lcfg, VOCAB_EMU2_CHAT), seed=0, device=dev, dtype=BF16))
    torch.cuda.synchronize()
    print(f"{a.layers} layers ready in {time.time() - t0:.0f}s, {torch.cuda.memory_allocated() / 2**30:.1f} GiB", flush=True)
    lines = [f"## Sampled decoding, {a.layers} layers at the LLaMA-33B shape, TP = 1, prompt {a.prompt}, temperature 0.7, top_p 0.9", "",
             f"ms/token, median of {a.rounds} alternating rounds of {a.steps} tokens (min .. max).", "",
             "| leg | B = 1 | B = 4 |", "|---|---|---|"]
    with torch.no_grad():
        res = {B: decode_legs(a, dev, lm, B) for B in (1, 4)}
        for k in res[1]:
            cell = lambda v: f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"
            lines.append(f"| {k} | {cell(res[1][k])} | {cell(res[4][k])} |")
        lines += ["", "## The sample kernel alone, V = 32 274 (HIP events over 200 back-to-back launches, microseconds per launch)", "",
                  "| rows | top_p 0.9, temperature 0.7 | + repetition penalty 1.3 (8 ids), top_k 50 | argmax_kernel |", "|---|---|---|---|"]
        for R, t1, t2, t3 in kernel_leg(dev):
            lines.append(f"| {R} | {t1:.1f} | {t2:.1f} | {t3:.1f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
