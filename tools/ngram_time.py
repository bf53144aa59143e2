#!/usr/bin/env python
"""What the no-repeat n-gram ban costs inside the device token loops, and what the device loops give against the host loop with the
same ban; one process, same box (needs a GPU):

    python tools/ngram_time.py [--layers 60] [--rounds 5] [--out profiles/ngram_ban.md]

ms per step at the LLaMA-33B shape with synthetic weights, prompt 770, TP = 1, one prompt, ``no_repeat_ngram_size = 3``, no EOS in
reach (every call runs to its limit), for three modes:

* one beam at the chat settings (sampling, temperature 0.7, top_p 0.9);
* five beams, deterministic (the reference's default search, length_penalty 0 as Emu1's captions);
* five beams, sampling at the demo backend's settings (temperature 0.7, top_k 3, top_p 0.9, length_penalty 1).

Legs per mode: the host loop with the ban (what every call with ``no_repeat_ngram_size`` ran before, and still runs without
``device_ngram_ban``), the device loop with the ban (``device_ngram_ban=True``, hipGraph replay), and the device loop without a ban.
Every figure is (a call of 24 new tokens - a call of 8) / 16, which takes the prefill, the cache fan-out and the first eager step
out; both lengths run once untimed first.  The legs alternate inside every round; the median over the rounds is reported with the
spread (min .. max).

Then the selection launches alone at ``cur = 255`` (the longest history the beam kernels take) with and without the ban: device
events around 200 launches per window, windows alternating, median and spread over the rounds.
"""
import argparse
import ctypes as C
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
NB, N, LONG, SHORT = 5, 3, 24, 8
PAD, NO_EOS = 32000, -1
CHAT = dict(do_sample=True, temperature=0.7, top_p=0.9)
DEMO = dict(do_sample=True, temperature=0.7, top_k=3, top_p=0.9, length_penalty=1.0)
LAUNCHES = 200


def selection_alone(V, rounds, dev):
    """us per launch of the three selection steps at cur = 255, rows as in a 5-beam search / one row for the sample kernel."""
    L = lib()
    g = torch.Generator().manual_seed(1)
    i32 = dict(dtype=torch.int32, device=dev)
    lg = (torch.randn(NB, V, generator=g) * 3.0).to(BF16).to(dev)
    hist = torch.randint(3, V, (256, NB), generator=g).to(torch.int32).to(dev)         # [steps, rows]: the sample kernel's history
    run = hist.t().contiguous().view(1, NB, 256)                                        # [B, nb, L]: the beam kernels'
    seq = run.clone()
    rs, bs = torch.zeros(1, NB, device=dev), torch.full((1, NB), -1.0e9, device=dev)
    fin, slen = torch.zeros(1, NB, dtype=torch.uint8, device=dev), torch.zeros(1, NB, **i32)
    opn, tok = torch.ones(1, dtype=torch.uint8, device=dev), torch.zeros(NB, **i32)
    flat = torch.zeros(NB, dtype=torch.int64, device=dev)
    ws = torch.empty(max(L.emu_beam_step_workspace_bytes(1, NB, V), L.emu_beam_sample_workspace_bytes(1, NB, V)), dtype=torch.uint8,
                     device=dev)
    step = torch.tensor([255], **i32)
    uni1 = torch.full((256, NB), 0.5, device=dev)
    unib = torch.full((1, 1, 2 * NB), 0.5, device=dev)
    out = torch.zeros(NB, **i32)
    chat = sample_params(True, 0.7, None, 0.9, 1.0, None, 0, NO_EOS, PAD)
    demo = sample_params(True, 0.7, 3, 0.9, 1.0, None, 0, NO_EOS, PAD, min_keep=2)
    st = lambda: ops.stream(dev)
    state = (lg.data_ptr(), NB * V, V, V, 1, NB, 256, 255, None, 0, NO_EOS, 1.0, 0, run.data_ptr(), seq.data_ptr(), rs.data_ptr(),
             bs.data_ptr(), fin.data_ptr(), slen.data_ptr(), opn.data_ptr(), tok.data_ptr(), flat.data_ptr(), ws.data_ptr(), ws.numel())
    sample = (lg.data_ptr(), V, 1, V, hist.data_ptr(), NB, 256, step.data_ptr(), uni1.data_ptr(), NB, 256, C.byref(chat), None,
              out.data_ptr(), None, 0)
    tail = (C.byref(demo), 0, unib.data_ptr(), 1, None, None, 0)
    banned = lambda kind: getattr(L, ops.SELECT_ENTRY[kind, "ngram"])
    legs = {
        ("sample kernel, 1 row, chat settings", "no ban"): lambda: L.emu_sample_bf16(*sample, st()),
        ("sample kernel, 1 row, chat settings", "ban"): lambda: banned("sample")(*sample, N, st()),
        ("beam step, 5 rows, deterministic", "no ban"): lambda: L.emu_beam_step_bf16(*state, st()),
        ("beam step, 5 rows, deterministic", "ban"): lambda: banned("beam_step")(*state, N, st()),
        ("beam sample step, 5 rows, demo settings", "no ban"): lambda: L.emu_beam_sample_step_bf16(*state, *tail, st()),
        ("beam sample step, 5 rows, demo settings", "ban"): lambda: banned("beam_sample_step")(*state, *tail, N, st()),
    }
    times = {k: [] for k in legs}
    for rnd in range(rounds + 1):                                 # round 0 is the warm-up
        for k, fn in legs.items():
            run.copy_(hist.t().reshape(1, NB, 256))                # (the step at the length limit rewrites its state: same input every window)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(LAUNCHES):
                rc = fn()
            b.record()
            torch.cuda.synchronize()
            assert rc == 0, (k, rc)
            if rnd:
                times[k].append(a.elapsed_time(b) / LAUNCHES * 1e3)
    return times


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--layers", type=int, default=60)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--prompt", type=int, default=770)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    V = VOCAB_EMU2_CHAT
    lcfg = LlamaCfg(num_hidden_layers=a.layers)
    lm = LlamaEngine(lcfg, V, EmuHipContext(dev))
    t0 = time.time()
    lm.load_weights(synth.iter_synth(synth.llama_param_shapes(lcfg, V), seed=0, device=dev, dtype=BF16))
    torch.cuda.synchronize()
    print(f"{a.layers} layers ready in {time.time() - t0:.0f}s", flush=True)
    x = (torch.randn(1, a.prompt, lcfg.hidden_size, generator=torch.Generator().manual_seed(2)) * 0.02).to(BF16).to(dev)
    mask = torch.ones(1, a.prompt, dtype=torch.long)

    def timed(fn, n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn(n)
        torch.cuda.synchronize()
        assert out.shape[1] == n, (out.shape, n)                  # the call ran to its limit
        return time.perf_counter() - t

    def leg(fn):
        return lambda: (timed(fn, LONG) - timed(fn, SHORT)) / (LONG - SHORT) * 1e3

    one = lambda **kw: (lambda n: lm.sample_generate(x, mask, n, min_len=0, eos_id=NO_EOS, pad_id=PAD, use_graph=True, **CHAT, **kw))
    beam = lambda **kw: (lambda n: lm.beam_search_generate(x, mask, NB, n, min_len=0, eos_id=NO_EOS, pad_id=PAD, hf_semantics="4.31",
                                                           **kw))
    ban = dict(no_repeat_ngram_size=N)
    modes = {
        "one beam, chat settings": (one(**ban), one(device_sampler=True, device_ngram_ban=True, **ban), one(device_sampler=True)),
        "5 beams, deterministic": (beam(length_penalty=0.0, **ban), beam(length_penalty=0.0, device_ngram_ban=True, **ban),
                                   beam(length_penalty=0.0)),
        "5 beams, sampling, demo settings": (beam(**DEMO, **ban), beam(device_beam_sampler=True, device_ngram_ban=True, **DEMO, **ban),
                                             beam(device_beam_sampler=True, **DEMO)),
    }
    kinds = ("host loop, ban", "device loop, ban", "device loop, no ban")
    legs = {(m, k): leg(fn) for m, fns in modes.items() for k, fn in zip(kinds, fns)}
    with torch.no_grad():
        for fn in legs.values():                                  # untimed: both lengths of every leg (graphs captured, torch ops warm)
            fn()
        times = {k: [] for k in legs}
        for rnd in range(a.rounds):
            for k, fn in legs.items():
                times[k].append(fn())
                print(f"round {rnd} {k}: {times[k][-1]:.3f} ms/step", flush=True)
        alone = selection_alone(V, a.rounds, dev)
    for k, v in alone.items():
        print(f"{k}: {['%.2f' % t for t in v]} us/launch", flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    cell = lambda k: f"{med[k]:.3f} ({min(times[k]):.3f} .. {max(times[k]):.3f})"
    lines = [f"## No-repeat n-gram ban (n = {N}), {a.layers} layers at the LLaMA-33B shape, TP = 1, prompt {a.prompt}, one prompt", "",
             f"ms per step: (a call of {LONG} new tokens - a call of {SHORT}) / {LONG - SHORT}; median of {a.rounds} alternating rounds "
             "(min .. max).  No EOS in reach: every call runs to its limit.", "",
             "| mode | host loop, ban | device loop, ban | device loop, no ban | host - device, both with the ban | "
             "ban cost: device ban - device no ban | largest spread of the windows involved |", "|---|---|---|---|---|---|---|"]
    for m in modes:
        h, d, u = (m, kinds[0]), (m, kinds[1]), (m, kinds[2])
        lines.append(f"| {m} | {cell(h)} | {cell(d)} | {cell(u)} | {med[h] - med[d]:+.3f} | {med[d] - med[u]:+.3f} | "
                     f"{max(spread[h], spread[d], spread[u]):.3f} |")
    am = {k: statistics.median(v) for k, v in alone.items()}
    acell = lambda k: f"{am[k]:.2f} ({min(alone[k]):.2f} .. {max(alone[k]):.2f})"
    lines += ["", f"### The selection launches alone at cur = 255 (V = {V})", "",
              f"us per launch, device events around {LAUNCHES} launches; median of {a.rounds} alternating windows (min .. max).", "",
              "| launch | no ban | ban | ban - no ban | largest spread |", "|---|---|---|---|---|"]
    for name in dict.fromkeys(k[0] for k in alone):
        u, d = (name, "no ban"), (name, "ban")
        lines.append(f"| {name} | {acell(u)} | {acell(d)} | {am[d] - am[u]:+.2f} | "
                     f"{max(max(alone[u]) - min(alone[u]), max(alone[d]) - min(alone[d])):.2f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
