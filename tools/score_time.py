#!/usr/bin/env python
"""Time of ranking candidate continuations with a shared prefix (needs a GPU):

    python tools/score_time.py [--layers 60] [--cands 64] [--cand-len 8] [--prefix 64] [--iters 5]

``LlamaEngine.score_continuations`` (one prefill of the prefix, its K / V copied to the candidates' rows, the candidates scored on
top) against ``prefill`` of the ``cands`` concatenated rows prefix + candidate -- what recomputing the prompt for every candidate,
as the reference does, costs on this engine (its head and loss are not even counted).  Synthetic weights at the 33B widths; host
clock between device synchronisations, best of ``--iters`` after one warm-up.  Prints one line per leg.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emu_amd import synth  # noqa: E402
from emu_amd.conf.emu_conf import LlamaCfg  # noqa: E402
from emu_amd.constants import VOCAB_EMU2_CHAT  # noqa: E402
from emu_amd.llama import EmuHipContext, LlamaEngine  # noqa: E402

BF16 = torch.bfloat16


def best_of(fn, iters):
    fn()
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return min(times), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--cands", type=int, default=64)
    ap.add_argument("--cand-len", type=int, default=8)
    ap.add_argument("--prefix", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("score_time.py measures on a GPU; none found")
    dev = torch.device("cuda", torch.cuda.current_device())
    lcfg = LlamaCfg(num_hidden_layers=a.layers)
    lm = LlamaEngine(lcfg, VOCAB_EMU2_CHAT, EmuHipContext(dev))
    lm.load_weights(synth.iter_synth(synth.llama_param_shapes(lcfg, VOCAB_EMU2_CHAT), seed=0, device=dev, dtype=BF16))
    g = torch.Generator().manual_seed(3)
    N, Tc, S = a.cands, a.cand_len, a.prefix
    prefix = torch.randint(3, 32000, (1, S), generator=g)
    cands = torch.randint(3, 32000, (N, Tc), generator=g)
    cmask = torch.ones(N, Tc, dtype=torch.bool)
    x = lm.embed_tokens(prefix)
    pmask = torch.ones(1, S, dtype=torch.int64)
    print(f"{torch.cuda.get_device_name(0)}: {a.layers} layers, {N} candidates of {Tc} tokens behind a {S}-token prefix", flush=True)
    for via in ("prefill", "decode"):
        ms, all_ms = best_of(lambda: lm.score_continuations(x, pmask, cands, cmask, via=via), a.iters)
        print(f"score_continuations via={via}: {ms:.2f} ms (runs: {', '.join('%.2f' % t for t in all_ms)})", flush=True)
    full = lm.embed_tokens(torch.cat([prefix.expand(N, -1), cands], dim=1))
    fmask = torch.ones(N, S + Tc, dtype=torch.int64)
    s_max = lm.kv_capacity(S + Tc)
    ms, all_ms = best_of(lambda: lm.prefill(full, fmask, s_max), a.iters)
    print(f"prefill of the {N} concatenated rows of {S + Tc}: {ms:.2f} ms (runs: {', '.join('%.2f' % t for t in all_ms)})", flush=True)


if __name__ == "__main__":
    main()
