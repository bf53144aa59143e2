#!/usr/bin/env python
"""Prompt-lookup speculative decoding against the one-row greedy step, one process, same box (needs a GPU):

    python tools/lookup_time.py [--layers 60] [--steps 48] [--warmup 8] [--rounds 2] [--out profiles/lookup_decode.md]

1. ms per chunk step at T = 2, 3, 5, 8 rows (``LlamaEngine.lookup_generate`` with a table of drafts, hipGraph-replayed, the loop
   alone between two device synchronisations) against ms per one-row greedy step (``GreedyState.step_graph``, the behaviour
   without the option, with the 13-bit packed one-row stream a model's loader switches on) at the LLaMA-33B shape behind a 770-row
   prompt, synthetic weights, TP = 1; bf16, fp8-wide and MXFP4-wide;
   the windows alternate, every window is reported.
2. The chunk attention launch alone (HIP events) against T one-row launches and against the transposing flash path, 52 heads of
   128, contexts 770, 1544 and 2304.
3. Tokens/s with ``drafts`` that are right for 0, half and all of their k entries, and from 1. the break-even acceptance per mode:
   a chunk step of T rows pays off once it emits more than (chunk step time / one-row step time) ids.

    python tools/lookup_time.py --sampling [--out profiles/lookup_sampling.md]

The sampling legs (prompt lookup together with ``do_sample`` or a repetition penalty, bf16, the same shape and prompt), in one run:

4. ms per chunk step with the sampler's selection at T = 2, 3, 5, 8 rows (the demo's temperature 0.7 / top_p 0.9, and penalty 1.2
   + top_k 50 + top_p 0.9), per chunk step with the greedy selection and per one-row ``emu_llama_sample_step``; windows alternate.
5. Tokens/s with drafts right for none, half and all of their entries, and the break-even acceptance.
6. The selection launches alone at V = 32 274 (HIP events): the sampler's selection + select against arg-maxes + select, and the
   one-row ``emu_sample_bf16``.

Acceptance on real text needs the real checkpoint and is not measured here (synthetic weights: the greedy ids are noise, which is
also why the forced acceptance is reported as counted by the device, not as intended).
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
from emu_amd.llama import EmuHipContext, GreedyState, LlamaEngine, SampleState, rope_tables, sample_params  # noqa: E402

BF16 = torch.bfloat16
MODES = ("bf16", "fp8-wide", "fp4-wide")
TS = (2, 3, 5, 8)


def set_mode(lm, mode):
    if getattr(lm, "fp8_decode", False):
        lm.use_fp8(False)
    if getattr(lm, "fp4_decode", False):
        lm.use_fp4(False)
    if mode == "fp8-wide":
        lm.use_fp8(True, wide=True)
    elif mode == "fp4-wide":
        lm.use_fp4(True, wide=True)


def forced_drafts(g, k, max_new, right, vocab):
    """Row s guesses g[s], g[s + 1], ..: right for its first ``right`` entries, wrong (the id plus one) from there on."""
    d = torch.zeros(max_new, k, dtype=torch.int32)
    for s in range(max_new):
        for j in range(k):
            gid = g[s + j] if s + j < len(g) else 0
            d[s, j] = gid if j < right and s + j < len(g) else (gid + 1) % vocab
    return d


def spread(v):
    return f"{min(v):.3f} (" + ", ".join(f"{t:.3f}" for t in v) + ")"


def engine_legs(a, dev):
    lcfg = LlamaCfg(num_hidden_layers=a.layers)
    V = VOCAB_EMU2_CHAT
    lm = LlamaEngine(lcfg, V, EmuHipContext(dev))
    t0 = time.time()
    lm.load_weights(synth.iter_synth(synth.llama_param_shapes(lcfg, V), seed=0, device=dev, dtype=BF16))
    lm.pack_bf16_default()                                        # as a model's loader does: the one-row bf16 step is the product's default
    lm.quantize_fp8()
    lm.quantize_fp4()
    torch.cuda.synchronize()
    print(f"weights + fp8 + fp4 copies ready in {time.time() - t0:.0f}s, {torch.cuda.memory_allocated() / 2**30:.1f} GiB", flush=True)
    S = a.prompt
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(1, S, lcfg.hidden_size, generator=g) * 0.02).to(BF16).to(dev)
    mask = torch.ones(1, S, dtype=torch.long)
    ids = torch.randint(3, V, (1, S), generator=g)
    n = a.steps + 1
    s_max = lm.kv_capacity(S + a.warmup + n + 16)
    hidden, kstart, next_pos = lm.prefill(x, mask, s_max)         # (the largest workspace the run needs: it is not re-allocated later)
    cur = ops.argmax(lm.logits(hidden[:, -1, :]), suppress_id=2)
    out_ids = torch.zeros(a.warmup + n + 8, 1, device=dev, dtype=torch.int32)
    one_row = {m: [] for m in MODES}
    chunk = {(m, T): [] for m in MODES for T in TS}
    wrong = {T: torch.full((n, T - 1), 5, dtype=torch.int32) for T in TS}       # (an id the random model does not emit)
    for rnd in range(a.rounds):
        for mode in MODES:
            set_mode(lm, mode)
            lm.prefill(x, mask, s_max)
            st = GreedyState(lm, 1, cur, next_pos, S, kstart, out_ids)
            for _ in range(a.warmup):
                st.step_graph()
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.steps):
                st.step_graph()
            torch.cuda.synchronize()
            one_row[mode].append((time.perf_counter() - t) / a.steps * 1e3)
            print(f"round {rnd} {mode}: one-row step {one_row[mode][-1]:.3f} ms", flush=True)
            del st
            for T in TS:
                for timed in (False, True):                       # the first call captures the step's graph
                    stats = dict(timing=True)
                    lm.lookup_generate(x, mask, ids, n, T - 1, use_graph=True, stop_on_eos=False, drafts=wrong[T], stats=stats)
                chunk[mode, T].append(stats["loop_seconds"] / stats["steps_launched"] * 1e3)
                print(f"round {rnd} {mode}: chunk step T={T} {chunk[mode, T][-1]:.3f} ms "
                      f"({stats['steps_launched']} steps, {stats['tokens_emitted']} ids)", flush=True)
    # ---- forced acceptance
    forced = []
    for mode in MODES:
        set_mode(lm, mode)
        one = lm.greedy_generate(x, mask, n, use_graph=True, stop_on_eos=False)[0].tolist()
        for k in (4, 7):
            # the ids the drafts are measured against are the chunk path's own: one id per step through the (1 + k)-row streams
            gids = lm.lookup_generate(x, mask, ids, n, k, use_graph=True, stop_on_eos=False, drafts=wrong[k + 1])[0].tolist()
            agree = sum(int(p == q) for p, q in zip(gids, one))
            for right in (0, k // 2, k):
                d = forced_drafts(gids, k, n, right, V)
                for timed in (False, True):
                    stats = dict(timing=True)
                    out = lm.lookup_generate(x, mask, ids, n, k, use_graph=True, stop_on_eos=False, drafts=d, stats=stats)
                same = sum(int(p == q) for p, q in zip(out[0].tolist(), gids))
                forced.append((mode, k, right, stats["steps_run"], stats["steps_launched"], stats["tokens_emitted"],
                               stats["loop_seconds"] * 1e3, same, agree))
                print("forced", forced[-1], flush=True)
    set_mode(lm, "bf16")
    return one_row, chunk, forced, S, n


SETTINGS = (("demo", dict(do_sample=True, temperature=0.7, top_p=0.9)),
            ("pen+k+p", dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9, repetition_penalty=1.2)))


def sampling_engine_legs(a, dev):
    lcfg = LlamaCfg(num_hidden_layers=a.layers)
    V = VOCAB_EMU2_CHAT
    lm = LlamaEngine(lcfg, V, EmuHipContext(dev))
    lm.load_weights(synth.iter_synth(synth.llama_param_shapes(lcfg, V), seed=0, device=dev, dtype=BF16))
    lm.pack_bf16_default()
    torch.cuda.synchronize()
    S = a.prompt
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(1, S, lcfg.hidden_size, generator=g) * 0.02).to(BF16).to(dev)
    mask = torch.ones(1, S, dtype=torch.long)
    ids = torch.randint(3, V, (1, S), generator=g)
    n = a.steps + 1
    uni = torch.rand(n, generator=g, dtype=torch.float32)
    s_max = lm.kv_capacity(S + a.warmup + n + 16)
    hidden, kstart, next_pos = lm.prefill(x, mask, s_max)
    n1 = a.warmup + n + 8
    uni1 = torch.rand(n1, 1, generator=g, dtype=torch.float32).to(dev)
    names = [name for name, _ in SETTINGS]
    one_row = {name: [] for name in names}
    chunk = {(sel, T): [] for sel in ["greedy"] + names for T in TS}
    wrong = {T: torch.full((n, T - 1), 5, dtype=torch.int32) for T in TS}
    for rnd in range(a.rounds):
        for name, o in SETTINGS:
            hidden, kstart, next_pos = lm.prefill(x, mask, s_max)
            out_ids = torch.zeros(n1, 1, device=dev, dtype=torch.int32)
            st = SampleState(lm, 1, next_pos, S, kstart, out_ids, uni1,
                             sample_params(True, o.get("temperature"), o.get("top_k"), o.get("top_p"), o.get("repetition_penalty", 1.0),
                                           2, 1, 2, 32000))
            lm.logits(hidden[:, -1, :], out=st.logits)
            st.first()
            for _ in range(a.warmup):
                st.step_graph()
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.steps):
                st.step_graph()
            torch.cuda.synchronize()
            one_row[name].append((time.perf_counter() - t) / a.steps * 1e3)
            print(f"round {rnd} one-row sample step ({name}) {one_row[name][-1]:.3f} ms", flush=True)
            del st
        for T in TS:
            for sel, o in [("greedy", {})] + list(SETTINGS):
                for timed in (False, True):                       # the first call captures the step's graph
                    stats = dict(timing=True)
                    lm.lookup_generate(x, mask, ids, n, T - 1, use_graph=True, stop_on_eos=False, drafts=wrong[T], stats=stats,
                                       uniforms=uni if o else None, **o)
                chunk[sel, T].append(stats["loop_seconds"] / stats["steps_launched"] * 1e3)
                print(f"round {rnd} chunk step T={T} {sel} {chunk[sel, T][-1]:.3f} ms ({stats['steps_launched']} steps)", flush=True)
    forced = []
    for name, o in SETTINGS:
        for k in (4, 7):
            gids = lm.lookup_generate(x, mask, ids, n, k, use_graph=True, stop_on_eos=False, drafts=wrong[k + 1], uniforms=uni, **o)[0].tolist()
            for right in (0, k // 2, k):
                d = forced_drafts(gids, k, n, right, V)
                for timed in (False, True):
                    stats = dict(timing=True)
                    out = lm.lookup_generate(x, mask, ids, n, k, use_graph=True, stop_on_eos=False, drafts=d, stats=stats, uniforms=uni, **o)
                same = sum(int(p == q) for p, q in zip(out[0].tolist(), gids))
                forced.append((name, k, right, stats["steps_run"], stats["steps_launched"], stats["tokens_emitted"],
                               stats["loop_seconds"] * 1e3, same))
                print("forced", forced[-1], flush=True)
    return one_row, chunk, forced, S, n


def selection_leg(a, dev):
    """The selection launches alone at V = 32 274: every call emits one id (a table of drafts that are never right), so the state
    advances as in the loop and the penalty's history grows by one id per call."""
    V = VOCAB_EMU2_CHAT
    g = torch.Generator().manual_seed(4)
    max_new = a.iters + 16
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    uni = torch.rand(max_new, 1, generator=g, dtype=torch.float32).to(dev)
    rows = []
    for T in TS:
        logits = (torch.randn(T, V, generator=g) * 3).to(BF16).to(dev)
        drafts = torch.full((max_new, T - 1), V - 1, dtype=torch.int32, device=dev)
        logits[:, V - 1] = -50.0

        def state():
            return (i32([7] + [V - 1] * (T - 1)), i32([1, 0, T - 1, 4, 0, 0, 0, 0]), i32([4]), i32([4]), i32([5]),
                    torch.zeros(max_new, dtype=torch.int32, device=dev), torch.zeros(max_new + 8, dtype=torch.int32, device=dev))
        amax = torch.zeros(T, dtype=torch.int32, device=dev)
        s = state()
        t_greedy = timeit(lambda: ops.lookup_select(logits, *s, 2, max_new, 1, 2, False, drafts=drafts, amax=amax), a.iters)
        assert int(s[1][0]) == a.iters + 4, "every timed call advanced the state by one id"
        row = [T, t_greedy]
        for name, o in SETTINGS:
            p = sample_params(True, o.get("temperature"), o.get("top_k"), o.get("top_p"), o.get("repetition_penalty", 1.0), 2, 1, 2, 32000)
            s = state()
            row.append(timeit(lambda: ops.lookup_sample(logits, *s, 2, max_new, 1, 2, p, uniforms=uni, stop_on_eos=False, drafts=drafts,
                                                        amax=amax), a.iters))
            assert int(s[1][0]) == a.iters + 4
            step = i32([a.iters // 2])
            hist = torch.zeros(max_new, 1, dtype=torch.int32, device=dev)
            out = torch.zeros(1, dtype=torch.int32, device=dev)
            row.append(timeit(lambda: ops.sample(logits[:1], step, p, out, hist=hist, uniforms=uni), a.iters))
        rows.append(row)
        print("selection", rows[-1], flush=True)
    return rows


def sampling_report(a, dev):
    names = [name for name, _ in SETTINGS]
    out = ["# Prompt-lookup speculation for sampling and penalised greedy decoding: measured", "",
           f"Written by `tools/lookup_time.py --sampling` ({torch.cuda.get_device_name(0)}; one process, so every comparison is same-run,",
           "same-box).  Synthetic weights: **acceptance on real text is not measured** -- it needs the real checkpoint.  The option is",
           "off by default (`EmuModel(device_sampler=True).generate(do_sample=True, ..., prompt_lookup_num_tokens=k)`).",
           "Settings: `demo` = temperature 0.7, top_p 0.9 (the chat demo's); `pen+k+p` = temperature 0.7, top_k 50, top_p 0.9, repetition",
           "penalty 1.2.", ""]
    rows = selection_leg(a, dev)
    out += ["## The selection launches alone, V = 32 274", "",
            f"HIP events around {a.iters} calls of the Python wrappers; every call emits one id, so the state advances as in the loop.",
            "`arg-max + select`: emu_lookup_select_bf16; `sample + select`: emu_lookup_sample_bf16 (T sampler workgroups side by side,",
            "then the select workgroup); `one-row sampler`: emu_sample_bf16 on one row.", "",
            "| T | arg-max + select us | " + " | ".join(f"sample + select us ({n}) | one-row sampler us ({n})" for n in names) + " |",
            "|---|---|" + "---|---|" * len(names)]
    for r in rows:
        out.append("| " + " | ".join([str(r[0])] + [f"{v:.1f}" for v in r[1:]]) + " |")
    out.append("")
    one_row, chunk, forced, S, n = sampling_engine_legs(a, dev)
    out += [f"## Step time, {a.layers} layers at the LLaMA-33B shape, bf16, TP = 1, behind a {S}-row prompt", "",
            f"hipGraph-replayed steps, a host clock between device synchronisations; one-row: `emu_llama_sample_step`, {a.warmup} warm-up +",
            f"{a.steps} timed steps; chunk: a warm-up call, then {a.steps} timed steps of `lookup_generate`'s loop (its prefill excluded);",
            f"{a.rounds} windows each, alternating; best window, all windows in brackets.  `over greedy` = the sampling selection's chunk",
            "step minus the greedy selection's, best windows.  Break-even = ids a chunk step must emit to match the one-row sample step",
            "per id (of which one is free: the step's own draw).", "",
            "| selection | one-row sample step ms | " + " | ".join(f"T={T} ms" for T in TS) + " | " +
            " | ".join(f"over greedy T={T} ms" for T in TS) + " | " + " | ".join(f"break-even T={T}" for T in TS) + " |",
            "|---|---|" + "---|" * (3 * len(TS))]
    out.append("| greedy (arg-max) | - | " + " | ".join(spread(chunk["greedy", T]) for T in TS) + " | " + " | ".join("-" for _ in TS) + " | " +
               " | ".join("-" for _ in TS) + " |")
    for name in names:
        o = min(one_row[name])
        out.append(f"| {name} | {spread(one_row[name])} | " + " | ".join(spread(chunk[name, T]) for T in TS) + " | " +
                   " | ".join(f"{min(chunk[name, T]) - min(chunk['greedy', T]):+.3f}" for T in TS) + " | " +
                   " | ".join(f"{min(chunk[name, T]) / o:.2f} ids" for T in TS) + " |")
    sp = max(max(v) - min(v) for v in chunk.values())
    out += ["", f"Largest spread between the windows of one chunk-step cell: {sp:.3f} ms.", "",
            "## Tokens/s at forced acceptance", "",
            "`drafts` right for their first `right` of k entries, against the ids the (1 + k)-row steps emit one at a time with the same",
            "uniforms (a run with drafts that are all wrong).  `steps run`, `ids emitted`: what the device counted; `same ids` = positions at",
            "which the output equals that run's.  Time: the loop alone, no-op replays behind the end included.", "",
            "| selection | k | right | steps run | launched | ids emitted | loop ms | tokens/s | one-row tokens/s | same ids |",
            "|---|---|---|---|---|---|---|---|---|---|"]
    best = {}
    for name, k, right, run, launched, emitted, ms, same in forced:
        tps, one = emitted / ms * 1e3, 1e3 / min(one_row[name])
        best[name] = max(best.get(name, 0.0), tps / one)
        out.append(f"| {name} | {k} | {right} | {run} | {launched} | {emitted} | {ms:.1f} | {tps:.1f} | {one:.1f} | {same}/{n} |")
    out += ["", "Best tokens/s over the one-row sample loop's: " + ", ".join(f"{m} {v:.2f}x" for m, v in best.items()) + ".", ""]
    return out


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
    return s.elapsed_time(e) / iters * 1e3          # us


def attention_leg(a, dev):
    H, D, S_max = 52, 128, 2304
    g = torch.Generator().manual_seed(3)
    kc = torch.randn(1, H, S_max, D, generator=g).to(BF16).to(dev)
    vc = torch.randn(1, H, S_max, D, generator=g).to(BF16).to(dev)
    cos, sin = rope_tables(D, S_max, 10000.0, dev)
    scale = D ** -0.5
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    rows = []
    for ctx in (770, 1544, 2304):
        for T in TS:
            slot0 = ctx - T
            qkv = torch.randn(T, 3 * H * D, generator=g).to(BF16).to(dev)
            p0, s0 = i32([slot0]), i32([slot0])
            ws = torch.empty(ops.lib().emu_decode_chunk_ws_bytes(1, T, H, D, ctx) // 4, device=dev, dtype=torch.float32)
            t_chunk = timeit(lambda: ops.decode_chunk(qkv, cos, sin, p0, s0, kc, vc, H, T, ctx, scale, ws=ws), a.iters)
            one = [(qkv[i:i + 1].contiguous(), i32([slot0 + i])) for i in range(T)]
            ws1 = torch.empty(ops.lib().emu_decode_fused_ws_bytes(1, H, D, ctx) // 4, device=dev, dtype=torch.float32)

            def seq():
                for q1, sl in one:
                    ops.decode_fused(q1, cos, sin, sl, sl, kc, vc, H, ctx, scale, ws=ws1)
            t_seq = timeit(seq, a.iters)
            q = qkv.view(1, T, 3, H, D)[:, :, 0]
            k4, v4 = kc.transpose(1, 2)[:, :ctx], vc.transpose(1, 2)[:, :ctx]
            t_flash = timeit(lambda: ops.flash_attn(q, k4, v4, True, scale), a.iters)
            rows.append((ctx, T, t_chunk, t_seq, t_flash))
            print("attention", rows[-1], flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--prompt", type=int, default=770)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sampling", action="store_true", help="the sampling legs alone -> profiles/lookup_sampling.md")
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip", default="", help="comma list of legs to leave out: engine, attention")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lookup_time.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "lookup_sampling.md" if a.sampling else "lookup_decode.md")
    if a.sampling:
        with torch.no_grad():
            out = sampling_report(a, dev)
        with open(a.out, "w") as f:
            f.write("\n".join(out))
        print("\n".join(out))
        return
    skip = set(a.skip.split(","))
    out = ["# Prompt-lookup speculative decoding: chunk steps measured against the one-row greedy step", "",
           f"Written by `tools/lookup_time.py` ({torch.cuda.get_device_name(0)}; one process, so every comparison is same-run, same-box).",
           "Synthetic weights: **acceptance on real text is not measured** -- it needs the real checkpoint.  The option is off by default",
           "(`generate(prompt_lookup_num_tokens=k)`).", ""]
    with torch.no_grad():
        if "attention" not in skip:
            rows = attention_leg(a, dev)
            out += ["## The chunk attention launch alone", "",
                    f"52 heads of 128, one sequence, the chunk's last row at the given context; HIP events around {a.iters} calls of the Python",
                    "wrapper (each allocates its output; the same for all three).  `T one-row launches`: emu_decode_fused_bf16 T times.",
                    "`flash path`: V transposed for the whole context, then the flash kernel on T query rows -- what a T-row forward",
                    "on top of a cache runs today (without its RoPE / append launch).", "",
                    "| context | T | chunk launch us | T one-row launches us | flash path us | chunk / one-row | chunk / flash |", "|---|---|---|---|---|---|---|"]
            for ctx, T, tc, ts, tf in rows:
                out.append(f"| {ctx} | {T} | {tc:.1f} | {ts:.1f} | {tf:.1f} | {tc / ts:.2f} | {tc / tf:.2f} |")
            out.append("")
        if "engine" not in skip:
            one_row, chunk, forced, S, n = engine_legs(a, dev)
            out += [f"## Step time, {a.layers} layers at the LLaMA-33B shape, TP = 1, behind a {S}-row prompt", "",
                    f"hipGraph-replayed steps, a host clock between device synchronisations; one-row: {a.warmup} warm-up + {a.steps} timed steps;",
                    f"chunk: a warm-up call, then {a.steps} timed steps of `lookup_generate`'s loop (its prefill excluded); {a.rounds} windows each,",
                    "alternating per mode; best window, all windows in brackets.  Break-even = ids a chunk step must emit to match the",
                    "one-row step per id = chunk step / one-row step (of which one is free: the step's own arg-max).", "",
                    "| mode | one-row step ms | " + " | ".join(f"T={T} ms" for T in TS) + " | " + " | ".join(f"break-even T={T}" for T in TS) + " |",
                    "|---|---|" + "---|" * (2 * len(TS))]
            for m in MODES:
                o = min(one_row[m])
                out.append(f"| {m} | {spread(one_row[m])} | " + " | ".join(spread(chunk[m, T]) for T in TS) + " | " +
                           " | ".join(f"{min(chunk[m, T]) / o:.2f} ids" for T in TS) + " |")
            out += ["", "## Tokens/s at forced acceptance", "",
                    "`drafts` right for their first `right` of k entries, against the ids the (1 + k)-row steps emit one at a time (a run",
                    "with drafts that are all wrong).  `steps run`, `ids emitted`: what the device counted.  `same ids` = positions at which",
                    "the output equals that run's; `as one-row` = positions at which that run equals the one-row greedy loop's (synthetic",
                    "weights have top-2 margins inside bf16 rounding, so the few-row and the one-row streams need not agree).  Time: the",
                    "loop alone, no-op replays behind the end included.", "",
                    "| mode | k | right | steps run | launched | ids emitted | loop ms | tokens/s | one-row tokens/s | same ids | as one-row |",
                    "|---|---|---|---|---|---|---|---|---|---|---|"]
            best = {}
            for m, k, right, run, launched, emitted, ms, same, agree in forced:
                tps, one = emitted / ms * 1e3, 1e3 / min(one_row[m])
                best[m] = max(best.get(m, 0.0), tps / one)
                out.append(f"| {m} | {k} | {right} | {run} | {launched} | {emitted} | {ms:.1f} | {tps:.1f} | {one:.1f} | {same}/{n} | {agree}/{n} |")
            out += ["", "Best tokens/s over the one-row loop's, per mode: " + ", ".join(f"{m} {v:.2f}x" for m, v in best.items()) + ".", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print("\n".join(out))


if __name__ == "__main__":
    main()
