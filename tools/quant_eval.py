#!/usr/bin/env python
"""What the quantised weight streams do to next-token distributions: teacher-forced scoring of given continuations through the
decode kernels (``LlamaEngine.score(via="decode")``), bf16 first, then each mode asked for with the bf16 logits as the reference
(needs a GPU):

    python tools/quant_eval.py [--checkpoint PATH] [--prompts FILE.jsonl] [--modes fp8,fp8-wide,fp4,fp4-wide,fp8-all] [--out profiles/quant_eval.md]

Per mode: mean NLL per scored token and its difference from bf16, mean and max KL(bf16 || mode), top-1 agreement with bf16, and
ms per scored token (hipGraph-replayed steps, host clock between device synchronisations, the second of two runs).

``--checkpoint``: the LLaMA of an Emu checkpoint (a file or a sharded directory, ``emu_amd.checkpoint``; keys ``decoder.lm.*``) at
the 33B shape.  Without one: synthetic weights at ``--layers`` / the 33B widths -- such figures show that the tool runs and how much
a mode moves random-init logits; they say NOTHING about a trained checkpoint.
``--prompts``: JSON lines of ``{"prompt_ids": [...], "cont_ids": [...]}`` (token ids, so no tokenizer is needed here); without it
``--n`` synthetic prompts of ``--prompt-len`` random ids with ``--cont-len`` continuation ids: half of each continuation is the
bf16 run's own greedy choice (tokens a model finds likely), half random ids (tokens it finds unlikely).

Rows per step follow the stream under test: fp8 and fp4 stream one-row steps (``use_fp8`` / ``use_fp4(True)``: 1-2 rows), fp8-wide
and fp4-wide the 3-16-row steps (``use_fp8(True, wide=True)`` / ``use_fp4(True, wide=True)``), so those modes score ``--wide-rows``
prompts at a time; bf16 is run at the same row count for each.  fp8-all (``use_fp8(True, wide=True, mid=True, all_rows=True)``)
scores ``via="prefill"``, every prompt in one batch: prefix and continuation rows run through the 65-rows-and-up form of the W8A16
GEMM (csrc/gemm_fp8.hip) where the batch has 65 rows or more, against bf16 scored the same way.
"""
import argparse
import json
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


def set_mode(lm, mode):
    if getattr(lm, "fp8_decode", False):
        lm.use_fp8(False)
    if getattr(lm, "fp4_decode", False):
        lm.use_fp4(False)
    if mode == "fp8":
        lm.use_fp8(True)
    elif mode == "fp8-wide":
        lm.use_fp8(True, wide=True)
    elif mode == "fp4":
        lm.use_fp4(True)
    elif mode == "fp4-wide":
        lm.use_fp4(True, wide=True)
    elif mode == "fp8-all":
        lm.use_fp8(True, wide=True, mid=True, all_rows=True)
    elif mode != "bf16":
        raise SystemExit(f"unknown mode {mode!r}: fp8, fp8-wide, fp4, fp4-wide, fp8-all")


def batches(items, rows):
    """Left-padded prompts and right-padded continuations, ``rows`` at a time: (ids, mask, cont, cmask) CPU tensors."""
    for i in range(0, len(items), rows):
        part = items[i:i + rows]
        S, T = max(len(p) for p, _ in part), max(len(c) for _, c in part)
        ids, mask = torch.zeros(len(part), S, dtype=torch.int64), torch.zeros(len(part), S, dtype=torch.int64)
        cont, cmask = torch.zeros(len(part), T, dtype=torch.int64), torch.zeros(len(part), T, dtype=torch.bool)
        for b, (p, c) in enumerate(part):
            ids[b, S - len(p):], mask[b, S - len(p):] = torch.tensor(p), 1
            cont[b, :len(c)], cmask[b, :len(c)] = torch.tensor(c), True
        yield ids, mask, cont, cmask


def run(lm, items, rows, refs=None, keep_logits=False, via="decode"):
    """Scores every batch twice (the first run warms up and captures); returns the per-batch dicts and ms per scored token."""
    out, tokens, secs = [], 0, 0.0
    for n, (ids, mask, cont, cmask) in enumerate(batches(items, rows)):
        x = lm.embed_tokens(ids)
        for attempt in range(2):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = lm.score(x, mask, cont, cmask, via=via, use_graph=via == "decode", reference_logits=None if refs is None else refs[n],
                         return_logits=keep_logits)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
        secs += dt
        tokens += int(cmask.sum())
        out.append(r)
    return out, secs / max(tokens, 1) * 1e3


def summarise(res, base=None):
    lp = torch.cat([r["lp"][r["counted"]] for r in res]).double()
    row = {"nll": float(-lp.mean()), "tokens": lp.numel()}
    if base is not None:
        row["kl_mean"] = float(torch.cat([r["kl"][r["counted"]] for r in res]).double().mean())
        row["kl_max"] = float(torch.cat([r["kl"][r["counted"]] for r in res]).max())
        row["agree"] = float(torch.cat([r["agree"][r["counted"]] for r in res]).double().mean())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--prompts", default=None)
    ap.add_argument("--modes", default="fp8,fp8-wide,fp4,fp4-wide")
    ap.add_argument("--layers", type=int, default=8, help="synthetic weights only: decoder layers at the 33B widths")
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--prompt-len", type=int, default=48)
    ap.add_argument("--cont-len", type=int, default=16)
    ap.add_argument("--wide-rows", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("quant_eval.py measures on a GPU; none found")
    if not 3 <= a.wide_rows <= 16:
        sys.exit("--wide-rows must be in 3..16 (the row counts the wide fp8 and MXFP4 streams serve)")
    modes = [m for m in a.modes.split(",") if m]
    dev = torch.device("cuda", torch.cuda.current_device())
    lcfg = LlamaCfg() if a.checkpoint else LlamaCfg(num_hidden_layers=a.layers)
    lm = LlamaEngine(lcfg, VOCAB_EMU2_CHAT, EmuHipContext(dev))
    if a.checkpoint:
        from emu_amd.checkpoint import iter_checkpoint
        lm.load_weights(iter_checkpoint(a.checkpoint))
        weights = f"checkpoint {a.checkpoint}"
    else:
        lm.load_weights(synth.iter_synth(synth.llama_param_shapes(lcfg, VOCAB_EMU2_CHAT), seed=0, device=dev, dtype=BF16))
        weights = f"SYNTHETIC weights (seed 0), {a.layers} layers at the 33B widths"
    if not lm.ready:
        sys.exit("the LLaMA weights are incomplete")
    if "fp8" in modes or "fp8-wide" in modes or "fp8-all" in modes:
        lm.quantize_fp8()

    if a.prompts:
        items = [(d["prompt_ids"], d["cont_ids"]) for d in map(json.loads, open(a.prompts)) if d]
        what = f"{len(items)} prompts of {a.prompts}"
    else:
        g = torch.Generator().manual_seed(1)
        items = []
        for i in range(a.n):
            p = [1] + torch.randint(3, 32000, (a.prompt_len - 1,), generator=g).tolist()
            half = a.cont_len // 2
            own = lm.greedy_generate(lm.embed_tokens(torch.tensor([p])), torch.ones(1, len(p), dtype=torch.int64), max(half, 1),
                                     min_len=0, stop_on_eos=False)[0].tolist()
            items.append((p, own[:half] + torch.randint(3, 32000, (a.cont_len - half,), generator=g).tolist()))
        what = (f"{a.n} synthetic prompts of {a.prompt_len} random ids, continuations of {a.cont_len}: {a.cont_len // 2} greedy ids "
                f"of the bf16 run, then random ids")

    lines = ["# Quantised weight streams against bf16: teacher-forced scoring through the decode kernels", ""]
    if not a.checkpoint:
        lines += ["**Synthetic weights: these figures say nothing about the real checkpoint.**  Random-init logits are nearly flat, so",
                  "NLL sits near log(vocab) and KL / agreement show only how far a mode moves such logits.  Evaluate a trained",
                  "checkpoint with `--checkpoint` before relying on a mode.", ""]
    lines += [f"Command: `python tools/quant_eval.py {' '.join(sys.argv[1:])}` ({torch.cuda.get_device_name(0)}).",
              f"Weights: {weights}.  Text: {what}.", "",
              "| mode | rows/step | tokens | mean NLL | dNLL vs bf16 | mean KL | max KL | top-1 agreement | ms/token |",
              "|---|---|---|---|---|---|---|---|---|"]
    base = {}
    for mode in modes:
        via = "prefill" if mode == "fp8-all" else "decode"
        rows = len(items) if via == "prefill" else a.wide_rows if mode in ("fp8-wide", "fp4-wide") else 1
        if (rows, via) not in base:
            set_mode(lm, "bf16")
            res, ms = run(lm, items, rows, keep_logits=True, via=via)
            base[(rows, via)] = ([r.pop("logits") for r in res], summarise(res), ms)
            b = base[(rows, via)][1]
            lines.append(f"| bf16{' (prefill)' if via == 'prefill' else ''} | {rows} | {b['tokens']} | {b['nll']:.4f} | | | | | {ms:.3f} |")
            print(lines[-1], flush=True)
        refs, b, _ = base[(rows, via)]
        set_mode(lm, mode)
        try:
            res, ms = run(lm, items, rows, refs=refs, via=via)
        finally:
            set_mode(lm, "bf16")
        s = summarise(res, b)
        lines.append(f"| {mode} | {rows} | {s['tokens']} | {s['nll']:.4f} | {s['nll'] - b['nll']:+.4f} | {s['kl_mean']:.3e} | "
                     f"{s['kl_max']:.3e} | {s['agree']:.3f} | {ms:.3f} |")
        print(lines[-1], flush=True)
    lines += ["", "KL is KL(bf16 || mode) per scored token; ms/token is per scored token of the second of two runs of each batch (graph replay),",
              "prefill and the first token's logits included.  fp8-all and its bf16 row score via=\"prefill\": rows/step is the batch, every",
              "prefix and continuation row of it in one forward."]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
