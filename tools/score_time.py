#!/usr/bin/env python
"""Time of ranking candidate continuations with a shared prefix (needs a GPU):

    python tools/score_time.py [--layers 60] [--cands 64 ...] [--cand-len 8] [--prefix 64 ...] [--iters 5] [--share-prefix {0,1,both}]

``--share-prefix 0`` (default): ``LlamaEngine.score_continuations`` (one prefill of the prefix, its K / V copied to the candidates'
rows, the candidates scored on top) against ``prefill`` of the ``cands`` concatenated rows prefix + candidate -- what recomputing the
prompt for every candidate, as the reference does, costs on this engine (its head and loss are not even counted).

``--share-prefix 1`` / ``both``: the route that keeps the prompt's cache in one place (``share_prefix=True``: a small suffix cache per
candidate, the two-segment flash kernel), alone or against the copying route in ALTERNATING windows of the same process -- per
(prefix, cands) pair: ms per call (median, min .. max of ``--iters`` windows after a warm-up of both), the bytes of the KV caches each
route holds (checked against ``scoring.shared_prefix_plan``: they are exact), the peak of ``torch.cuda.max_memory_allocated`` above
the resident weights, and the attention of ONE layer alone (device events): the V transposes plus the flash launch of each route.

Synthetic weights at the 33B widths; host clock between device synchronisations.  Prints one line per leg.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emu_amd import ops, scoring, synth  # noqa: E402
from emu_amd.conf.emu_conf import LlamaCfg  # noqa: E402
from emu_amd.constants import VOCAB_EMU2_CHAT  # noqa: E402
from emu_amd.llama import EmuHipContext, LlamaEngine  # noqa: E402

BF16 = torch.bfloat16


def window(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def best_of(fn, iters):
    fn()
    times = [window(fn) for _ in range(iters)]
    return min(times), times


def spread(times):
    return f"{statistics.median(times):.2f} ms (min {min(times):.2f} .. max {max(times):.2f}, {len(times)} windows)"


def event_ms(fn, reps=20):
    """Device time of one ``fn()``: events around ``reps`` back-to-back calls after a warm-up."""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def kv_bytes(lm):
    return {k: 2 * v[0].numel() * 2 for k, v in lm.__dict__.get("_kv_slots", {}).items() if v is not None}


def attention_alone(lm, N, S, n):
    """One layer's attention of N rows of n queries behind S prompt slots, as each route launches it: (shared ms, unshared ms)."""
    Hl, D, dev = lm.plan.heads_local, lm.cfg.head_dim, lm.device
    g = torch.Generator().manual_seed(5)
    mk = lambda *s: torch.randn(*s, generator=g).to(BF16).to(dev)
    q, kp, vp, ko, vo = mk(N, n, Hl, D), mk(S, Hl, D), mk(S, Hl, D), mk(N, n, Hl, D), mk(N, n, Hl, D)
    scale = 1.0 / D ** 0.5
    shared = event_ms(lambda: ops.flash_attn_prefix(q, kp, vp, ko, vo, 0, scale))
    kcat = torch.cat([kp[None].expand(N, -1, -1, -1), ko], dim=1).contiguous()
    vcat = torch.cat([vp[None].expand(N, -1, -1, -1), vo], dim=1).contiguous()
    unshared = event_ms(lambda: ops.flash_attn(q, kcat, vcat, True, scale))
    return shared, unshared


def legacy_legs(lm, x, pmask, prefix, cands, cmask, iters):
    N, Tc, S = cands.shape[0], cands.shape[1], prefix.shape[1]
    for via in ("prefill", "decode"):
        ms, all_ms = best_of(lambda: lm.score_continuations(x, pmask, cands, cmask, via=via), iters)
        print(f"score_continuations via={via}: {ms:.2f} ms (runs: {', '.join('%.2f' % t for t in all_ms)})", flush=True)
    full = lm.embed_tokens(torch.cat([prefix.expand(N, -1), cands], dim=1))
    fmask = torch.ones(N, S + Tc, dtype=torch.int64)
    s_max = lm.kv_capacity(S + Tc)
    ms, all_ms = best_of(lambda: lm.prefill(full, fmask, s_max), iters)
    print(f"prefill of the {N} concatenated rows of {S + Tc}: {ms:.2f} ms (runs: {', '.join('%.2f' % t for t in all_ms)})", flush=True)


def shared_legs(lm, x, pmask, cands, cmask, iters, routes):
    N, Tc, S = cands.shape[0], cands.shape[1], x.shape[1]
    plan = scoring.shared_prefix_plan(N, S, [Tc], lm.cfg.num_hidden_layers, lm.plan.heads_local, lm.cfg.head_dim, lm.kv_capacity)
    seg = plan["segments"][0]
    want = {True: {"main": plan["prefix_bytes"], "suffix": seg["shared_bytes"]},
            False: {"main": plan["prefix_bytes"], "beam": seg["unshared_bytes"]}}
    calls = {r: (lambda r=r: lm.score_continuations(x, pmask, cands, cmask, share_prefix=r)) for r in routes}
    name = {True: "shared", False: "unshared"}
    for r in routes:                                       # memory, each route from an engine without caches (also the warm-up)
        lm.release_kv()
        lm._ws = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        rest = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        calls[r]()
        torch.cuda.synchronize()
        got = kv_bytes(lm)
        assert got == want[r], (got, want[r])
        print(f"  {name[r]:8s} KV caches {sum(got.values()) / 1e9:8.3f} GB = plan ({', '.join(f'{k} {v / 1e9:.3f}' for k, v in got.items())}); "
              f"peak above the weights {(torch.cuda.max_memory_allocated() - rest) / 1e9:8.3f} GB", flush=True)
    lm.release_kv()
    for r in routes:
        calls[r]()                                         # both routes' caches resident and warm before the timed windows
    times = {r: [] for r in routes}
    for _ in range(iters):                                 # alternating windows
        for r in routes:
            times[r].append(window(calls[r]))
    for r in routes:
        print(f"  {name[r]:8s} score_continuations via=prefill: {spread(times[r])}", flush=True)
    if len(routes) == 2:
        d = statistics.median(times[False]) - statistics.median(times[True])
        noise = max(max(t) - min(t) for t in times.values())
        print(f"  shared is {d:+.2f} ms ahead (medians); largest window spread {noise:.2f} ms -> "
              f"{'a difference' if abs(d) > noise else 'NO difference beyond the spread'}", flush=True)
        same = torch.equal(calls[True]()[0], calls[False]()[0])
        print(f"  lp of the two routes bit-identical: {same} (expected for a prefix that is a multiple of 64: {S % 64 == 0})", flush=True)
    a_s, a_u = attention_alone(lm, N, S, max(Tc - 1, 2))
    print(f"  attention of one layer alone (V transposes + flash launch): shared {a_s * 1e3:.1f} us, unshared {a_u * 1e3:.1f} us", flush=True)
    lm.release_kv()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--cands", type=int, nargs="+", default=[64])
    ap.add_argument("--cand-len", type=int, default=8)
    ap.add_argument("--prefix", type=int, nargs="+", default=[64])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--share-prefix", choices=("0", "1", "both"), default="0")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("score_time.py measures on a GPU; none found")
    dev = torch.device("cuda", torch.cuda.current_device())
    lcfg = LlamaCfg(num_hidden_layers=a.layers)
    lm = LlamaEngine(lcfg, VOCAB_EMU2_CHAT, EmuHipContext(dev))
    lm.load_weights(synth.iter_synth(synth.llama_param_shapes(lcfg, VOCAB_EMU2_CHAT), seed=0, device=dev, dtype=BF16))
    g = torch.Generator().manual_seed(3)
    Tc = a.cand_len
    for S in a.prefix:
        for N in a.cands:
            prefix = torch.randint(3, 32000, (1, S), generator=g)
            cands = torch.randint(3, 32000, (N, Tc), generator=g)
            cmask = torch.ones(N, Tc, dtype=torch.bool)
            x = lm.embed_tokens(prefix)
            pmask = torch.ones(1, S, dtype=torch.int64)
            print(f"{torch.cuda.get_device_name(0)}: {a.layers} layers, {N} candidates of {Tc} tokens behind a {S}-token prefix", flush=True)
            if a.share_prefix == "0":
                legacy_legs(lm, x, pmask, prefix, cands, cmask, a.iters)
            else:
                shared_legs(lm, x, pmask, cands, cmask, a.iters, (True, False) if a.share_prefix == "both" else (True,))


if __name__ == "__main__":
    main()
