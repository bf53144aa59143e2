#!/usr/bin/env python
"""What the device beam sampler costs and buys, one process, same box (needs a GPU):

    python tools/beam_sample_time.py [--layers 60] [--steps 32] [--rounds 3] [--out profiles/beam_sampler.md]

1. ms per beam step of beam-search sampling with the demo backend's options (five beams, temperature 0.7, top_k 3, top_p 0.9,
   length_penalty 1; repetition_penalty 1.0 and 1.2) at the LLaMA-33B shape with synthetic weights, prompt 512, B = 1 and B = 4:
   (a) the host loop of ``beam_search_generate`` as it is (``torch.multinomial``), (b) the device loop
   (``device_beam_sampler=True``), eager launches, (c) the device loop replayed from a hipGraph -- and the deterministic device beam
   step of the same run (``emu_beam_step_bf16``, replayed) as the floor.  Every leg is the difference of two whole calls of
   ``--short`` and ``--short + --steps`` new tokens (no EOS in reach, so every call runs to its limit), which takes the prefill, the
   cache fan-out and the first eager step out of the figure; both lengths are run once untimed first (graphs captured, torch ops
   warm).  The legs alternate inside every round; the median over the rounds is reported with the spread.
2. The step's two launches alone (HIP events around a batch of calls, V = 32 274, five beams): ``emu_beam_sample_step_bf16`` sampling
   and penalised, next to the two launches of ``emu_beam_step_bf16``.

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
from emu_amd._lib import lib  # noqa: E402
from emu_amd.conf.emu_conf import LlamaCfg  # noqa: E402
from emu_amd.constants import VOCAB_EMU2_CHAT  # noqa: E402
from emu_amd.llama import EmuHipContext, LlamaEngine, sample_params  # noqa: E402

BF16 = torch.bfloat16
NB = 5
DEMO = dict(do_sample=True, temperature=0.7, top_k=3, top_p=0.9, length_penalty=1.0)
PAD, NO_EOS = 32000, -1


def decode_legs(a, dev, lm, B):
    S = a.prompt
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(B, S, lm.cfg.hidden_size, generator=g) * 0.02).to(BF16).to(dev)
    mask = torch.ones(B, S, dtype=torch.long)

    def call(n, graph, **kw):
        lm.beam_graph = graph
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = lm.beam_search_generate(x, mask, NB, n, min_len=0, eos_id=NO_EOS, pad_id=PAD, hf_semantics="4.31", **kw)
        torch.cuda.synchronize()
        lm.beam_graph = True
        assert out.shape[1] == n, (out.shape, n)                   # the call ran to its limit
        return time.perf_counter() - t

    def leg(graph, **kw):
        return lambda: (call(a.short + a.steps, graph, **kw) - call(a.short, graph, **kw)) / a.steps * 1e3

    legs = {}
    for pen in (1.0, 1.2):
        o = dict(DEMO, repetition_penalty=pen)
        legs[f"host loop (beam_search_generate as it is), repetition_penalty {pen}"] = leg(True, **o)
        legs[f"device loop, eager, repetition_penalty {pen}"] = leg(False, device_beam_sampler=True, **o)
        legs[f"device loop, hipGraph replay, repetition_penalty {pen}"] = leg(True, device_beam_sampler=True, **o)
    legs["deterministic device beam step, hipGraph replay (floor)"] = leg(True, length_penalty=1.0)
    for k, fn in legs.items():                                     # untimed: both lengths of every leg
        fn()
    times = {k: [] for k in legs}
    for rnd in range(a.rounds):
        for k, fn in legs.items():
            times[k].append(fn())
            print(f"B={B} round {rnd} {k}: {times[k][-1]:.3f} ms/step", flush=True)
    return times


def kernel_leg(dev, reps=200):
    V, L_, rows_out = VOCAB_EMU2_CHAT, 64, []
    L = lib()
    for B in (1, 4):
        i32 = dict(dtype=torch.int32, device=dev)
        x = (torch.randn(B * NB, V, generator=torch.Generator().manual_seed(B)) * 3).to(BF16).to(dev)
        run = torch.randint(0, V, (B, NB, L_), **i32)
        seq = run.clone()
        rs = -torch.rand(B, NB, device=dev) * 4
        bs = torch.full((B, NB), -1.0e9, device=dev)
        fin, ln = torch.zeros(B, NB, dtype=torch.uint8, device=dev), torch.zeros(B, NB, **i32)
        opn = torch.ones(B, dtype=torch.uint8, device=dev)
        tok, flat = torch.zeros(B * NB, **i32), torch.zeros(B * NB, dtype=torch.int64, device=dev)
        uni = torch.rand(1, B, 2 * NB, device=dev)
        ws = torch.empty(max(L.emu_beam_sample_workspace_bytes(B, NB, V), L.emu_beam_step_workspace_bytes(B, NB, V)),
                         dtype=torch.uint8, device=dev)
        rs0 = rs.clone()
        state = (x.data_ptr(), NB * V, V, V, B, NB, L_, 8, None, 0, NO_EOS, 1.0, 1, run.data_ptr(), seq.data_ptr(), rs.data_ptr(),
                 bs.data_ptr(), fin.data_ptr(), ln.data_ptr(), opn.data_ptr(), tok.data_ptr(), flat.data_ptr(), ws.data_ptr(), ws.numel())

        def sampled(par, acc431):
            def f():
                rs.copy_(rs0)                                      # (the step updates its state: every launch sees the same scores)
                rc = L.emu_beam_sample_step_bf16(*state, par, acc431, uni.data_ptr(), 1, None, None, 0, ops.stream(dev))
                assert rc == 0, rc
            return f

        def plain():
            rs.copy_(rs0)
            rc = L.emu_beam_step_bf16(*state, ops.stream(dev))
            assert rc == 0, rc

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

        base = ev(lambda: rs.copy_(rs0))
        demo = sample_params(True, 0.7, 3, 0.9, 1.2, None, 0, NO_EOS, PAD, min_keep=2)
        wide = sample_params(True, 0.7, None, 0.9, 1.0, None, 0, NO_EOS, PAD, min_keep=2)
        pen = sample_params(False, None, None, None, 1.2, None, 0, NO_EOS, PAD, min_keep=2)
        rows_out.append((B, ev(sampled(demo, 1)) - base, ev(sampled(wide, 0)) - base, ev(sampled(pen, 0)) - base, ev(plain) - base))
        print("kernels B=%d: demo %.1f us, top_p only %.1f us, penalised %.1f us, emu_beam_step_bf16 %.1f us" % rows_out[-1], flush=True)
    return rows_out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--layers", type=int, default=60)
    p.add_argument("--steps", type=int, default=32)
    p.add_argument("--short", type=int, default=8)
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
    lines = [f"## Beam-search sampling, {a.layers} layers at the LLaMA-33B shape, TP = 1, prompt {a.prompt}, {NB} beams, temperature 0.7, "
             "top_k 3, top_p 0.9, length_penalty 1", "",
             f"ms per beam step: (a call of {a.short + a.steps} new tokens - a call of {a.short}) / {a.steps}; median of {a.rounds} "
             "alternating rounds (min .. max).", "", "| leg | B = 1 | B = 4 |", "|---|---|---|"]
    with torch.no_grad():
        kern = kernel_leg(dev)
        res = {B: decode_legs(a, dev, lm, B) for B in (1, 4)}
    cell = lambda v: f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"
    for k in res[1]:
        lines.append(f"| {k} | {cell(res[1][k])} | {cell(res[4][k])} |")
    lines += ["", f"## The step's two launches alone, V = 32 274, {NB} beams (HIP events over 200 back-to-back calls, microseconds per "
              "call, the state reset's copy subtracted)", "",
              "| prompts | emu_beam_sample_step_bf16: the demo's options, \"4.31\" order | top_p 0.9 only, \"5.x\" order | penalised, no "
              "sampling | emu_beam_step_bf16 |", "|---|---|---|---|---|"]
    for B, t1, t2, t3, t4 in kern:
        lines.append(f"| {B} | {t1:.1f} | {t2:.1f} | {t3:.1f} | {t4:.1f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
