#!/usr/bin/env python
"""The few-row stream over the 13-bit packed bf16 sets (csrc/gemv_pack_thin.hip) against the bf16 few-row stream it would replace
(csrc/gemv_thin.hip), one process (needs a GPU):

    python tools/pack_wide_time.py [--layers 60] [--iters 30] [--rounds 3] [--out profiles/bf16_pack_wide.md]
    python tools/pack_wide_time.py --ab         # 16 / 32 weight rows per workgroup (emu_gemm_tune bits 28-29); prints only
    python tools/pack_wide_time.py --bits both [--out profiles/bf16_pack12_wide.md]     # the 12-bit twin against the 13-bit one

1. Every projection on its own at the LLaMA-33B shapes, TP = 1 and the TP = 2 shards, at 4 / 5 / 8 / 16 rows: HIP events, the
   weights rotating through more copies than the infinity cache holds, the two contenders alternating in windows of one run.
2. A 5-beam step at --layers layers behind a 770-row prompt, ``use_bf16_pack_wide`` off against on: ms per step from the difference
   of two beam searches of different lengths (the prefill and the set-up cancel), windows alternating.
3. The chunk step of prompt-lookup speculation at 5 and 8 rows (k = 4 / 7, every draft forced and rejected, so a step emits one id),
   off against on, the same way.

--bits 13 (the default) is the above.  --bits 12 / both measure the twin over the 12-bit sets (legs 1b, 2b below the code of 1-3):
every TP = 1 projection under bf16 / the 13-bit twin / the 12-bit twin, and the engine in three states -- the switch off on 12-bit
sets (the default), on with the repack to 13 bits, on with ``keep12`` -- each with the 5-beam step, the two lookup chunk steps and the
one-row greedy step, the device memory of the sets, and the GEMV profiler's bytes of a 5-row and a one-row step as the witness of
which kernels ran.

Off is the path of a build without the switch: the comparison is same-run, same-box.  Writes the tables to --out, every window next
to the best one.  The results are the same bits either way (tests/test_gpu_bf16_pack_wide.py); only time is measured here.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emu_amd import ops, synth  # noqa: E402
from emu_amd._lib import lib  # noqa: E402
from emu_amd.conf.emu_conf import LlamaCfg  # noqa: E402
from emu_amd.constants import VOCAB_EMU2_CHAT  # noqa: E402
from emu_amd.llama import EmuHipContext, LlamaEngine  # noqa: E402

BF16 = torch.bfloat16
HBM = 8.0e12
# (name, N, K, epilogue, rows per group of the set the one-row stream of the matrix reads)
SHAPES = [("qkv", 19968, 6656, 0, 4), ("o+res", 6656, 6656, 1, 2), ("gateup+swiglu", 35840, 6656, 2, 4), ("down+res", 6656, 17920, 1, 2),
          ("lm_head", 32274, 6656, 0, 4),
          ("qkv tp2", 9984, 6656, 0, 4), ("o+res tp2", 6656, 3328, 1, 2), ("gateup+swiglu tp2", 17920, 6656, 2, 4), ("down+res tp2", 6656, 8960, 1, 2)]


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


def weight_sets(N, K, R, dev):
    """> 600 MB of bf16 copies of an [N, K] matrix, each with its packed set"""
    out = []
    for _ in range(max(1, int(600e6 // (N * K * 2)) + 1)):
        w = (torch.randn(N, K, device=dev) * 0.02).to(BF16)
        out.append((w, ops.pack_bf16_rows(w, R)))
    return out


def stream_leg(a, dev, rows_list, pins=(0,)):
    """rows: [name, N, K, M, {contender: [window seconds]}]; the contenders' windows alternate"""
    out = []
    for name, N, K, epi, R in SHAPES:
        sets = weight_sets(N, K, R, dev)
        for M in rows_list:
            xv = torch.randn(M, K, device=dev).to(BF16)
            res = torch.randn(M, N, device=dev).to(BF16) if epi == 1 else None
            i = [0]

            def bf16():
                i[0] += 1
                ops.linear(xv, sets[i[0] % len(sets)][0], res=res, epi=epi)

            def pack():
                i[0] += 1
                w, p = sets[i[0] % len(sets)]
                ops.linear_bf16pack_thin(xv, w, p, res=res, epi=epi)
            contenders = {"bf16": (bf16, 0)}
            contenders.update({"pack" + (f" {8 << pin}" if pin else ""): (pack, pin << 28) for pin in pins})
            t = {c: [] for c in contenders}
            for _ in range(a.rounds):
                for c, (fn, tune) in contenders.items():
                    lib().emu_gemm_tune(tune)
                    t[c].append(timeit(fn, a.iters))
                    lib().emu_gemm_tune(0)
            print("stream", name, N, K, M, {c: [round(v * 1e6, 1) for v in ts] for c, ts in t.items()}, flush=True)
            out.append([name, N, K, M, t])
        del sets
        torch.cuda.empty_cache()
    return out


def engine_leg(a, dev):
    lcfg = LlamaCfg(num_hidden_layers=a.layers)
    lm = LlamaEngine(lcfg, VOCAB_EMU2_CHAT, EmuHipContext(dev))
    t0 = time.time()
    lm.load_weights(synth.iter_synth(synth.llama_param_shapes(lcfg, VOCAB_EMU2_CHAT), seed=0, device=dev, dtype=BF16))
    rule = lm.pack_bf16_default()
    torch.cuda.synchronize()
    print(f"weights + packed sets ({rule}: {len(lm._pack)} matrices) ready in {time.time() - t0:.0f}s, "
          f"{torch.cuda.memory_allocated() / 2**30:.1f} GiB", flush=True)
    assert lm.bf16_pack_on and len(lm._pack) == 4 * a.layers + 1, "every projection and the head need a packed set for this comparison"
    S = a.prompt
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(1, S, lcfg.hidden_size, generator=g) * 0.02).to(BF16).to(dev)
    mask = torch.ones(1, S, dtype=torch.long)
    ids = torch.randint(3, 30000, (1, S), generator=g)
    n0, n1 = a.short, a.long

    def beam(n):
        lm.beam_search_generate(x, mask, 5, n, min_len=n)
        torch.cuda.synchronize()
        return n - 1

    def lookup(k):
        def call(n):
            stats = {}
            drafts = torch.full((n, k), 1, dtype=torch.int32)           # id 1 is never the arg-max of these weights' rows: all rejected
            lm.lookup_generate(x, mask, ids, n, k, min_len=n, use_graph=True, stop_on_eos=False, drafts=drafts, stats=stats)
            torch.cuda.synchronize()
            return stats["steps_run"]
        return call

    def per_step(call):
        ts, steps = {}, {}
        for n in (n0, n1):
            call(n)                                      # warm-up: graph capture of this length
            t = time.perf_counter()
            steps[n] = call(n)
            ts[n] = time.perf_counter() - t
        return (ts[n1] - ts[n0]) / max(1, steps[n1] - steps[n0]) * 1e3
    result = {}
    for what, call in (("5-beam step (5 rows)", beam), ("lookup chunk step, k = 4 (5 rows)", lookup(4)), ("lookup chunk step, k = 7 (8 rows)", lookup(7))):
        times = {"off": [], "on": []}
        for rnd in range(a.rounds):
            for mode in ("off", "on"):
                lm.use_bf16_pack_wide(mode == "on")
                times[mode].append(per_step(call))
                print(f"{what}, round {rnd} {mode}: {times[mode][-1]:.3f} ms per step", flush=True)
        lm.use_bf16_pack_wide(False)
        result[what] = times
    return result, S


# ---- --bits 12 / both: the 12-bit twin.  13 = the yardstick, bf16 beside it
def stream_leg12(a, dev, rows_list, bits):
    """rows: [name, N, K, M, {contender: [window seconds]}] over the TP = 1 shapes; contenders bf16, pack13, pack12, alternating"""
    out = []
    for name, N, K, epi, R in SHAPES[:5]:
        copies = []
        for _ in range(max(1, int(600e6 // (N * K * 2)) + 1)):
            w = (torch.randn(N, K, device=dev) * 0.02).to(BF16)
            copies.append((w, ops.pack_bf16_rows(w, R) if 13 in bits else None, ops.pack12_bf16_rows(w, R)))
        flagged = sum(c[2]["flagged"] for c in copies) / len(copies)
        for M in rows_list:
            xv = torch.randn(M, K, device=dev).to(BF16)
            res = torch.randn(M, N, device=dev).to(BF16) if epi == 1 else None
            i = [0]

            def run(which):
                def fn():
                    i[0] += 1
                    c = copies[i[0] % len(copies)]
                    if which == 0:
                        ops.linear(xv, c[0], res=res, epi=epi)
                    else:
                        ops.linear_bf16pack_thin(xv, c[0], c[which], res=res, epi=epi)
                return fn
            contenders = {"bf16": run(0)}
            if 13 in bits:
                contenders["pack13"] = run(1)
            contenders["pack12"] = run(2)
            t = {c: [] for c in contenders}
            for _ in range(a.rounds):
                for c, fn in contenders.items():
                    t[c].append(timeit(fn, a.iters))
            print("stream12", name, N, K, M, {c: [round(v * 1e6, 1) for v in ts] for c, ts in t.items()}, f"flagged groups per copy {flagged:.1f}", flush=True)
            out.append([name, N, K, M, t, flagged, R])
        del copies
        torch.cuda.empty_cache()
    return out


def engine_leg12(a, dev, bits):
    """{state: {step: [ms windows]}}, {state: witness}, prompt rows.  States: the switch off on 12-bit sets, on with the repack to 13
    bits, on with keep12; their windows alternate, so the sets are packed again between them (to 13 bits and back to 12)."""
    import ctypes as C
    lcfg = LlamaCfg(num_hidden_layers=a.layers)
    lm = LlamaEngine(lcfg, VOCAB_EMU2_CHAT, EmuHipContext(dev))
    t0 = time.time()
    lm.load_weights(synth.iter_synth(synth.llama_param_shapes(lcfg, VOCAB_EMU2_CHAT), seed=0, device=dev, dtype=BF16))
    rule = lm.pack_bf16_default()
    torch.cuda.synchronize()
    n12 = sum("patch" in v for v in lm._pack.values())
    print(f"weights + packed sets ({rule}: {len(lm._pack)} matrices, {n12} at 12 bits) ready in {time.time() - t0:.0f}s, "
          f"{torch.cuda.memory_allocated() / 2**30:.1f} GiB", flush=True)
    assert lm.bf16_pack_on and len(lm._pack) == 4 * a.layers + 1 and n12 == len(lm._pack), "every projection and the head need a 12-bit set for this comparison"
    S = a.prompt
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(1, S, lcfg.hidden_size, generator=g) * 0.02).to(BF16).to(dev)
    mask = torch.ones(1, S, dtype=torch.long)
    ids = torch.randint(3, 30000, (1, S), generator=g)
    n0, n1 = a.short, a.long

    def beam(n):
        lm.beam_search_generate(x, mask, 5, n, min_len=n)
        torch.cuda.synchronize()
        return n - 1

    def greedy(n):
        lm.greedy_generate(x, mask, n, min_len=n, use_graph=True, stop_on_eos=False)
        torch.cuda.synchronize()
        return n - 1

    def lookup(k):
        def call(n):
            stats = {}
            drafts = torch.full((n, k), 1, dtype=torch.int32)           # id 1 is never the arg-max of these weights' rows: all rejected
            lm.lookup_generate(x, mask, ids, n, k, min_len=n, use_graph=True, stop_on_eos=False, drafts=drafts, stats=stats)
            torch.cuda.synchronize()
            return stats["steps_run"]
        return call

    def per_step(call):
        ts, steps = {}, {}
        for n in (n0, n1):
            call(n)                                      # warm-up: graph capture of this length
            t = time.perf_counter()
            steps[n] = call(n)
            ts[n] = time.perf_counter() - t
        return (ts[n1] - ts[n0]) / max(1, steps[n1] - steps[n0]) * 1e3

    def profiled_bytes(rows):
        """(bytes, launches) the GEMV profiler prices over one eager cached step of `rows` rows + its logits"""
        xs = (torch.randn(rows, 25, lcfg.hidden_size, generator=g) * 0.02).to(BF16).to(dev)
        _, kstart, pos = lm.prefill(xs[:, :24].contiguous(), torch.ones(rows, 24, dtype=torch.long), lm.kv_capacity(40))
        lib().emu_profile_gemv(1)
        try:
            lm.logits(lm.decode_embeds(xs[:, 24].contiguous(), pos, 24, kstart))
            torch.cuda.synchronize()
            ms, wb, nl = C.c_double(), C.c_double(), C.c_long()
            lib().emu_profile_gemv_read(C.byref(ms), C.byref(wb), C.byref(nl))
        finally:
            lib().emu_profile_gemv(0)
        return wb.value, nl.value

    def enter(state):
        lm.use_bf16_pack_wide(False)
        if state != "on, repacked to 13 bits" and not all("patch" in v for v in lm._pack.values()):
            lm._drop_bf16_pack(list(lm._pack))           # back to 12-bit sets
            lm.pack_bf16(head_form=True, bits12=True)
            torch.cuda.synchronize()
        if state == "on, repacked to 13 bits":
            lm.use_bf16_pack_wide(True)
        elif state == "on, keep12":
            lm.use_bf16_pack_wide(True, keep12=True)
        torch.cuda.synchronize()

    states = ["off, 12-bit sets"] + (["on, repacked to 13 bits"] if 13 in bits else []) + ["on, keep12"]
    steps = (("5-beam step (5 rows)", beam), ("lookup chunk step, k = 4 (5 rows)", lookup(4)), ("lookup chunk step, k = 7 (8 rows)", lookup(7)),
             ("greedy step (1 row)", greedy))
    result = {st: {what: [] for what, _ in steps} for st in states}
    witness = {}
    profiled_bytes(5), profiled_bytes(1)                 # (their KV caches exist in every state's memory figure alike)
    for st in states:                                    # before any generation: the memory is the weights, those caches and the sets
        enter(st)
        torch.cuda.empty_cache()
        witness[st] = dict(sets=sum(lm._set_bytes(v) for v in lm._pack.values()), bits12=sum("patch" in v for v in lm._pack.values()),
                           allocated=torch.cuda.memory_allocated(), five=profiled_bytes(5), one=profiled_bytes(1))
        print(f"state {st}: {witness[st]}", flush=True)
    for rnd in range(a.rounds):
        for st in states:
            enter(st)
            for what, call in steps:
                result[st][what].append(per_step(call))
                print(f"{what}, round {rnd}, {st}: {result[st][what][-1]:.3f} ms per step", flush=True)
    lm.use_bf16_pack_wide(False)
    bf16_bytes = sum(2 * v["shape"][0] * v["shape"][1] for v in lm._pack.values())
    return result, witness, S, bf16_bytes


def report12(a, dev, bits, skip):
    both = 13 in bits
    out = ["# 12-bit packed bf16 weights for 4..16-row steps: the 12-bit twin of the few-row stream, measured", "",
           f"Written by `tools/pack_wide_time.py --bits {'both' if both else '12'}` ({torch.cuda.get_device_name(0)}; one process, alternating windows, so every",
           "comparison is same-run, same-box).  The outputs are the same bits on every path (`tests/test_gpu_bf16_pack12_wide.py`), so time",
           "and memory are the only questions.  Opt-in: `LlamaEngine.use_bf16_pack_wide(True, keep12=True)`, `EMU_BF16_PACK_WIDE=12`.",
           "Synthetic weights, N(0, 0.02^2): the miss and flag rates of a real checkpoint are unknown and nothing here speaks for them.", ""]
    if "stream" not in skip:
        rows = stream_leg12(a, dev, (4, 5, 8, 16), bits)
        out += ["## Every projection on its own, 4 / 5 / 8 / 16 rows", "",
                f"HIP events around {a.iters} launches, weights rotating through > 600 MB of copies, {a.rounds} windows per contender alternating; us per",
                "launch: best window, all windows in brackets (their spread is the noise of the run).  bf16 = what `ops.linear` launches",
                "(`gemv_thin.hip`); 13 / 12 = `gemv_pack_thin.hip` over the 13-bit / the 12-bit set of the same matrix.  A verdict is `yes` when the",
                "12-bit twin's best window is below the other's by more than the larger spread of the two.", "",
                "| stream | N | K | rows | bf16 us | 13-bit us | 12-bit us | 12 / 13 | 12 / bf16 | below 13-bit | below bf16 | flagged groups |",
                "|---|---|---|---|---|---|---|---|---|---|---|---|"]
        lose13, lose16 = [], []
        for name, N, K, M, t, flagged, R in rows:
            p12 = min(t["pack12"])
            w16, _ = verdict(t["bf16"], t["pack12"])
            if not w16:
                lose16.append(f"{name} at {M} rows")
            if both:
                w13, _ = verdict(t["pack13"], t["pack12"])
                if not w13:
                    lose13.append(f"{name} at {M} rows")
            out.append(f"| {name} | {N} | {K} | {M} | {windows(t['bf16'])} | {windows(t['pack13']) if both else '-'} | {windows(t['pack12'])} | "
                       f"{p12 / min(t['pack13']) if both else float('nan'):.3f} | {p12 / min(t['bf16']):.3f} | "
                       f"{('yes' if w13 else '**no**') if both else '-'} | {'yes' if w16 else '**no**'} | {flagged:.1f} of {(N + R - 1) // R} |")
        out += [""]
        if both:
            out += ["The 12-bit twin is NOT below the 13-bit twin by more than the windows' spread at: " + (", ".join(lose13) if lose13 else "none of these cases") + ".", ""]
        out += ["The 12-bit twin is NOT below the bf16 stream by more than the windows' spread at: " + (", ".join(lose16) if lose16 else "none of these cases") + ".", ""]
    if "engine" not in skip:
        result, witness, S, bf16_bytes = engine_leg12(a, dev, bits)
        states = list(result)
        out += [f"## Whole steps, {a.layers} layers at the LLaMA-33B shape, TP = 1, every projection and the head packed", "",
                f"A prompt of {S} rows; ms per step = (time of a {a.long}-token run - time of a {a.short}-token run) / the steps between them, each run",
                f"once to warm up (graph capture) and once timed, host clock between device synchronisations, {a.rounds} windows per state, the states",
                "alternating (the sets are packed again between them); best window, all windows in brackets.  The lookup steps run forced",
                "drafts that are all rejected: one id per step.", "",
                "| step | " + " | ".join(f"{st}, ms" for st in states) + " |", "|---|" + "---|" * len(states)]
        for what in result[states[0]]:
            out.append(f"| {what} | " + " | ".join(windows(result[st][what], 1.0, "{:.3f}") for st in states) + " |")
        out += ["", "Which kernels ran, from the GEMV profiler over one eager step plus its logits (bytes priced, launches), and the memory:", "",
                "| state | sets at 12 bits | bytes of all sets, GiB | device memory allocated, GiB | 5-row step: bytes priced, GiB (launches) | 1-row step: bytes priced, GiB (launches) |",
                "|---|---|---|---|---|---|"]
        for st in states:
            w = witness[st]
            out.append(f"| {st} | {w['bits12']} | {w['sets'] / 2**30:.3f} | {w['allocated'] / 2**30:.2f} | {w['five'][0] / 2**30:.3f} ({w['five'][1]}) | "
                       f"{w['one'][0] / 2**30:.3f} ({w['one'][1]}) |")
        out += ["", f"The same matrices as bf16 are {bf16_bytes / 2**30:.3f} GiB: a step priced at that ran the bf16 kernels, one priced at a state's set bytes ran the",
                "packed twins of those sets.", ""]
        k12, off = "on, keep12", "off, 12-bit sets"
        lines = []
        one = "greedy step (1 row)"
        d = min(result[k12][one]) - min(result[off][one])
        sp = max(max(result[s][one]) - min(result[s][one]) for s in (k12, off))
        lines.append(f"- one-row step, keep12 against the switch off: {min(result[k12][one]):.3f} vs {min(result[off][one]):.3f} ms (difference {d:+.3f}, spread {sp:.3f}): "
                     + ("equal within the spread" if abs(d) <= sp else "**NOT equal within the spread**"))
        if both:
            r13 = "on, repacked to 13 bits"
            for what in result[off]:
                if what == one:
                    continue
                d = min(result[k12][what]) - min(result[r13][what])
                sp = max(max(result[s][what]) - min(result[s][what]) for s in (k12, r13))
                lines.append(f"- {what}, keep12 against the repack: {min(result[k12][what]):.3f} vs {min(result[r13][what]):.3f} ms (difference {d:+.3f}, spread {sp:.3f}): "
                             + ("no slower by more than the spread" if d <= sp else "**slower by more than the spread**"))
        out += ["The claim -- with keep12 the one-row step is the switch-off one, and the few-row steps are no slower than after the repack:", ""] + lines + [""]
    return out


def windows(ts, scale=1e6, fmt="{:.1f}"):
    return fmt.format(min(ts) * scale) + " (" + " ".join(fmt.format(v * scale) for v in ts) + ")"


def verdict(off, on):
    """(on is below off by more than the windows' spread, the spread)"""
    spread = max(max(off) - min(off), max(on) - min(on))
    return min(off) - min(on) > spread, spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=770)
    ap.add_argument("--short", type=int, default=8)
    ap.add_argument("--long", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_pack_wide.md"))
    ap.add_argument("--ab", action="store_true", help="only the rows-per-workgroup A/B at 5 and 16 rows (prints, writes nothing)")
    ap.add_argument("--skip", default="", help="comma list of legs to leave out: stream, engine")
    ap.add_argument("--bits", default="13", choices=["13", "12", "both"], help="13: the 13-bit twin against bf16 (the default); 12 / both: the 12-bit twin "
                    "against bf16 / and the 13-bit twin, the engine in its states (write to --out profiles/bf16_pack12_wide.md)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pack_wide_time.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    if a.ab:
        with torch.no_grad():
            stream_leg(a, dev, (5, 16), pins=(0, 1, 2))
        return
    skip = set(a.skip.split(","))
    if a.bits != "13":
        with torch.no_grad():
            out = report12(a, dev, (13, 12) if a.bits == "both" else (12,), skip)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(out) + "\n")
        print("\n".join(out))
        return
    out = ["# 13-bit packed bf16 weights for 4..16-row steps: measured against the bf16 few-row stream", "",
           f"Written by `tools/pack_wide_time.py` ({torch.cuda.get_device_name(0)}; one process, so every comparison is same-run, same-box).",
           "The outputs are the same bits either way (`tests/test_gpu_bf16_pack_wide.py`), so time is the only question.  The mode is",
           "opt-in (`LlamaEngine.use_bf16_pack_wide()`, `EMU_BF16_PACK_WIDE=1`); off is the path of a build without it.", ""]
    with torch.no_grad():
        if "stream" not in skip:
            rows = stream_leg(a, dev, (4, 5, 8, 16))
            out += ["## Every projection on its own, 4 / 5 / 8 / 16 rows", "",
                    f"HIP events around {a.iters} launches, weights rotating through > 600 MB of copies, {a.rounds} windows per contender",
                    "alternating; us per launch: best window, all windows in brackets (their spread is the noise of the run).  bf16 = what",
                    "`ops.linear` launches (`gemv_thin.hip`), pack = `gemv_pack_thin.hip` over the set of the same matrix.  HBM share = the",
                    "packed stream's plane bytes (13 / 8 x N x K) / its best time / 8 TB/s.", "",
                    "| stream | N | K | rows | bf16 us | pack us | pack / bf16 | pack HBM share | below bf16 by more than the spread |",
                    "|---|---|---|---|---|---|---|---|---|"]
            lose = []
            for name, N, K, M, t in rows:
                b, p = min(t["bf16"]), min(t["pack"])
                won, _ = verdict(t["bf16"], t["pack"])
                if not won:
                    lose.append(f"{name} at {M} rows")
                out.append(f"| {name} | {N} | {K} | {M} | {windows(t['bf16'])} | {windows(t['pack'])} | {p / b:.3f} | {N * K * 13 / 8 / p / HBM:.3f} | "
                           f"{'yes' if won else '**no**'} |")
            out += ["", "The packed stream is NOT below the bf16 stream by more than the windows' spread at: " + (", ".join(lose) if lose else "none of these cases") + ".", ""]
        if "engine" not in skip:
            result, S = engine_leg(a, dev)
            out += [f"## Whole steps, {a.layers} layers at the LLaMA-33B shape, TP = 1, every projection and the head packed", "",
                    f"A prompt of {S} rows; ms per step = (time of a {a.long}-token run - time of a {a.short}-token run) / the steps between them, each",
                    f"run once to warm up (graph capture) and once timed, host clock between device synchronisations, {a.rounds} windows per mode",
                    "alternating; best window, all windows in brackets.  The lookup steps run forced drafts that are all rejected: one id per step.", "",
                    "| step | switch off, ms | switch on, ms | on / off | below off by more than the spread |", "|---|---|---|---|---|"]
            for what, times in result.items():
                won, spread = verdict(times["off"], times["on"])
                out.append(f"| {what} | {windows(times['off'], 1.0, '{:.3f}')} | {windows(times['on'], 1.0, '{:.3f}')} | "
                           f"{min(times['on']) / min(times['off']):.3f} | {'yes' if won else f'**no** (spread {spread:.3f} ms)'} |")
            out.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
    print("\n".join(out))


if __name__ == "__main__":
    main()
