#!/usr/bin/env python
"""What the constraint costs inside the device token loops, and what the device loop gains over the host loop with the same trie;
one process, same box (needs a GPU):

    python tools/constrained_time.py [--layers 60] [--rounds 5] [--out profiles/constrained_decoding.md]

ms per step at the LLaMA-33B shape with synthetic weights, prompt 770, TP = 1, for three tries of depth 8 (so that a call of 8 new
tokens never reaches an EOS and runs to its limit):

* "yes/no": two chains of 8 tokens -- the root has two children, every other node one (the shape of the reference's VizWiz trie,
  Emu1/mm_eval/models/emu.py:96-109, kept up for 8 steps);
* 1000 random sequences of 8 tokens;
* whole vocabulary: at every one of the 8 levels the node holds every id but EOS as a child.

Legs: the 5-beam device loop (hipGraph replay) unconstrained and with each trie, the 5-beam host loop with each trie (forced by
handing over the trie's callable), and the one-beam device loop (greedy through the sample kernel, hipGraph replay) unconstrained and
with each trie.  Every figure is (a call of 8 new tokens - a call of 2) / 6, which takes the prefill, the cache fan-out and the first
eager step out; both lengths run once untimed first.  The legs alternate inside every round; the median over the rounds is reported
with the spread (min .. max), and the two differences the README quotes are written next to it.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emu_amd import synth  # noqa: E402
from emu_amd.conf.emu_conf import LlamaCfg  # noqa: E402
from emu_amd.constants import VOCAB_EMU2_CHAT  # noqa: E402
from emu_amd.constrain import TokenTrie  # noqa: E402
from emu_amd.llama import EmuHipContext, LlamaEngine  # noqa: E402

BF16 = torch.bfloat16
NB, DEPTH, LONG, SHORT = 5, 8, 8, 2
PAD, EOS, NO_EOS = 32000, 2, -1


def tries(V):
    g = torch.Generator().manual_seed(0)
    ids = lambda n: [int(t) for t in torch.randint(3, V, (n,), generator=g)]
    yes_no = TokenTrie([ids(DEPTH), ids(DEPTH)], EOS, V)
    rand = TokenTrie([ids(DEPTH) for _ in range(1000)], EOS, V)
    # a trie over sequences cannot hold the whole vocabulary at 8 levels in a row (V ** 8 sequences), so this one's tables are written
    # directly: level k's node holds every id but EOS, and all of them lead to level k + 1's node; the last level's lead to EOS
    other = [t for t in range(V) if t != EOS]
    whole = TokenTrie.__new__(TokenTrie)
    whole._eos, whole._vocab, whole._count, whole._min_depth, whole._tables = EOS, V, len(other) ** DEPTH, DEPTH, {}
    whole._first = tuple(k * len(other) for k in range(DEPTH)) + (DEPTH * len(other), DEPTH * len(other) + 1)
    whole._tok = tuple(other) * DEPTH + (EOS,)
    whole._child = tuple(k + 1 for k in range(DEPTH) for _ in other) + (-1,)
    return {"yes/no (2 chains of 8)": yes_no, "1000 random sequences of 8": rand, "whole vocabulary at every level": whole}


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
    tt = tries(V)
    for name, t in tt.items():
        t.tables(dev)
        print(f"trie {name}: {t.nodes} nodes, {t.edges} edges", flush=True)
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

    beam = lambda **kw: (lambda n: lm.beam_search_generate(x, mask, NB, n, min_len=0, pad_id=PAD, hf_semantics="4.31", **kw))
    one = lambda **kw: (lambda n: lm.sample_generate(x, mask, n, min_len=0, do_sample=False, pad_id=PAD, device_sampler=True,
                                                     use_graph=True, **kw))
    legs = {("beam", "device", None): leg(beam(eos_id=NO_EOS)), ("one", "device", None): leg(one(eos_id=NO_EOS))}
    for name, t in tt.items():
        legs[("beam", "device", name)] = leg(beam(eos_id=EOS, constraint=t))
        legs[("beam", "host", name)] = leg(beam(eos_id=EOS, constraint=t.as_callable()))
        legs[("one", "device", name)] = leg(one(eos_id=EOS, constraint=t))
    with torch.no_grad():
        for fn in legs.values():                                  # untimed: both lengths of every leg (graphs captured, torch ops warm)
            fn()
        times = {k: [] for k in legs}
        for rnd in range(a.rounds):
            for k, fn in legs.items():
                times[k].append(fn())
                print(f"round {rnd} {k}: {times[k][-1]:.3f} ms/step", flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    cell = lambda k: f"{med[k]:.3f} ({min(times[k]):.3f} .. {max(times[k]):.3f})"
    lines = [f"## Constrained decoding, {a.layers} layers at the LLaMA-33B shape, TP = 1, prompt {a.prompt}, one prompt", "",
             f"ms per step: (a call of {LONG} new tokens - a call of {SHORT}) / {LONG - SHORT}; median of {a.rounds} alternating rounds "
             "(min .. max).  Every trie is 8 tokens deep, so no call reaches an EOS.", "",
             f"### {NB} beams", "",
             "| trie | device loop, hipGraph replay | host loop, same trie | mask cost: device constrained - unconstrained | "
             "gain: host - device constrained | largest spread of the windows involved |", "|---|---|---|---|---|---|",
             f"| none | {cell(('beam', 'device', None))} | | | | |"]
    for name in tt:
        d, h, u = ("beam", "device", name), ("beam", "host", name), ("beam", "device", None)
        lines.append(f"| {name} | {cell(d)} | {cell(h)} | {med[d] - med[u]:+.3f} | {med[h] - med[d]:+.3f} | "
                     f"{max(spread[d], spread[h], spread[u]):.3f} |")
    lines += ["", "### One beam (greedy through the sample kernel)", "",
              "| trie | device loop, hipGraph replay | mask cost: constrained - unconstrained | largest spread of the windows involved |",
              "|---|---|---|---|", f"| none | {cell(('one', 'device', None))} | | |"]
    for name in tt:
        d, u = ("one", "device", name), ("one", "device", None)
        lines.append(f"| {name} | {cell(d)} | {med[d] - med[u]:+.3f} | {max(spread[d], spread[u]):.3f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
