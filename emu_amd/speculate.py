"""Prompt-lookup speculative greedy decoding, specified in pure torch / Python: what ``csrc/lookup.hip`` computes on the device.

The option is the library's ``lm.generate(prompt_lookup_num_tokens=k, max_matching_ngram_size=n)``, which the reference reaches
through the ``**kwargs`` of ``Emu2/emu/emu.py:175,228``.  A step feeds the last emitted id and up to k guessed ids through the model
at once (one few-row step costs about one token's time), and keeps the guessed ids for as long as each equals the arg-max of the
row before it -- so every emitted id is the arg-max of the model's own logits, and the output is the greedy one.

``lookup_draft`` restates ``PromptLookupCandidateGenerator.get_candidates`` (checked against the installed library in
``tests/test_speculate_host.py``); ``accept`` is the verification; ``simulate`` runs the whole loop on a table of arg-maxes, which
is how the tests predict ``steps_run``.

Together with ``do_sample`` or a repetition penalty (``row_select``, ``simulate_select``; ``csrc/sample.hip``: lookup_sample_kernel) the
library's ``_assisted_decoding`` runs the processors and warpers on every row, with the history extended by the draft ids before that
row, draws one token per row and keeps the draft for as long as each drawn token equals the next draft id.  Here the draw of output
index j always uses ``uniforms[j]``, whichever row of whichever step makes it, so with the same uniforms the speculative loop emits
the ids the one-token-at-a-time device sampler emits: speculation changes the speed, not the sample.

Imports nothing from the engine."""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import sampling

MAX_DRAFT = 7                  # k: a chunk step has 1 + k <= 8 rows (DECODE_CHUNK_MAX of the chunk attention kernel)


def lookup_draft(history: Sequence[int], k: int, max_ngram: int) -> List[int]:
    """The ids guessed to follow ``history``: for n from min(max_ngram, L - 1) down to 1, the first window (left to right) that
    equals the last n ids and is followed by at least one id gives up to k ids behind it, cut at the end of the history.  No
    such window: no draft."""
    h = [int(t) for t in history]
    L = len(h)
    for n in range(min(max_ngram, L - 1), 0, -1):
        tail = h[L - n:]
        for i in range(0, L - n):                          # i + n < L: the window is followed by at least one id
            if h[i:i + n] == tail:
                return h[i + n:min(i + n + k, L)]
    return []


def row_argmax(logits: torch.Tensor, step: int, min_len: int, eos: int) -> List[int]:
    """a[i]: the arg-max of row i of ``logits`` [T, V] (lowest index on ties), EOS suppressed while step + i < min_len."""
    x = logits.float().clone()
    for i in range(x.shape[0]):
        if step + i < min_len and 0 <= eos < x.shape[1]:
            x[i, eos] = float("-inf")
    best = x.max(dim=-1, keepdim=True).values
    idx = torch.arange(x.shape[1])[None].expand_as(x)
    return [int(v) for v in torch.where(x == best, idx, x.shape[1]).min(dim=-1).values]


def accept(draft: Sequence[int], n_draft: int, argmax_rows: Sequence[int], step: int, max_new: int, min_len: int, eos: int,
           stop_on_eos: bool = True) -> Tuple[int, bool]:
    """Row 0 was fed the last emitted id and rows 1.. the draft; ``argmax_rows`` = a (``row_argmax``).  n = the number of leading
    j < n_draft with draft[j] == a[j]; a[0..n] are emitted at indices step.., cut at max_new and behind the first EOS (an EOS at an
    index below min_len does not end anything: a suppressed arg-max never is one).  -> (n_emit, finished)."""
    n = 0
    while n < n_draft and n < len(draft) and int(draft[n]) == int(argmax_rows[n]):
        n += 1
    n_emit = min(n + 1, max_new - step)
    finished = False
    if stop_on_eos:
        for i in range(n_emit):
            if int(argmax_rows[i]) == eos and step + i >= min_len:
                n_emit, finished = i + 1, True
                break
    return n_emit, finished or step + n_emit >= max_new


def simulate(rows: Callable[[List[int], int], List[int]], first: int, prompt_ids: Sequence[int], k: int, max_ngram: int, max_new: int,
             min_len: int, eos: int, drafts: Optional[torch.Tensor] = None, stop_on_eos: bool = True) -> Tuple[List[int], int]:
    """The loop behind the first token: ``rows(fed, step)`` -> the arg-maxes of the 1 + k rows fed ``fed`` on top of the ids emitted
    so far.  ``drafts`` [max_new, k]: row ``step`` in place of the lookup.  -> (emitted ids, steps run)."""
    out, hist = [int(first)], [int(t) for t in prompt_ids] + [int(first)]
    steps, finished = 0, max_new <= 1 or (stop_on_eos and int(first) == eos and min_len <= 0)
    while not finished:
        step = len(out)
        d = [int(t) for t in drafts[step]] if drafts is not None else lookup_draft(hist, k, max_ngram)
        fed = [out[-1]] + d + [0] * (k - len(d))
        a = rows(fed, step)
        n_emit, finished = accept(d, len(d), a, step, max_new, min_len, eos, stop_on_eos)
        out += [int(t) for t in a[:n_emit]]
        hist += [int(t) for t in a[:n_emit]]
        steps += 1
    return out, steps


def row_select(logits: torch.Tensor, out_hist: Sequence[int], cur: Sequence[int], step: int, params: dict,
               uniforms: Optional[torch.Tensor] = None) -> List[int]:
    """The ids the T rows of a chunk step pick when the loop samples or penalises: row i exactly as ``emu_sample_bf16`` picks output
    index ``step + i`` (``emu_amd/sampling.py``).  ``logits`` [T, V]; ``out_hist``: the generated ids (the first ``step`` are read: with
    ``inputs_embeds`` the prompt contributes none); ``cur`` [T]: the fed ids, cur[0] the last emitted one, cur[1:] the draft padded with
    0.  Row i's history is out_hist[:step] + cur[1:1 + i]; ``params['suppress_id']`` is suppressed while step + i <
    ``params['min_len']``; its uniform is uniforms[min(step + i, rows - 1)] (``uniforms`` fp32 [rows] or [rows, 1]).  ``params``:
    ``repetition_penalty``, ``suppress_id``, ``min_len``, ``do_sample``, ``temperature``, ``top_k``, ``top_p``, ``min_keep`` (each
    optional: off)."""
    T = logits.shape[0]
    gen = [int(t) for t in out_hist[:step]]
    pen = float(params.get("repetition_penalty", 1.0))
    u = None if uniforms is None else uniforms.reshape(-1).to(torch.float32)
    picked = []
    for i in range(T):
        hist = [gen + [int(t) for t in cur[1:1 + i]]]
        sup = params.get("suppress_id") if step + i < int(params.get("min_len", 0)) else None
        row = logits[i:i + 1]
        if not params.get("do_sample"):
            picked.append(int(sampling.reference_greedy(row, hist, pen, sup)[0]))
            continue
        probs = sampling.reference_probs(row, hist, pen, sup, True, params.get("temperature"), params.get("top_k"), params.get("top_p"),
                                         int(params.get("min_keep", 1)))
        picked.append(int(sampling.reference_draw(probs, u[min(step + i, u.numel() - 1)].reshape(1).to(probs.device))[0]))
    return picked


def simulate_select(rows: Callable[[List[int], int, List[int]], List[int]], first: int, prompt_ids: Sequence[int], k: int, max_ngram: int,
                    max_new: int, min_len: int, eos: int, drafts: Optional[torch.Tensor] = None,
                    stop_on_eos: bool = True) -> Tuple[List[int], int]:
    """``simulate`` for a selection that depends on the history: ``rows(fed, step, out)`` -> the ids the 1 + k rows pick, ``out`` the ids
    emitted so far (``row_select``'s ``out_hist``).  -> (emitted ids, steps run)."""
    out, hist = [int(first)], [int(t) for t in prompt_ids] + [int(first)]
    steps, finished = 0, max_new <= 1 or (stop_on_eos and int(first) == eos and min_len <= 0)
    while not finished:
        step = len(out)
        d = [int(t) for t in drafts[step]] if drafts is not None else lookup_draft(hist, k, max_ngram)
        fed = [out[-1]] + d + [0] * (k - len(d))
        a = rows(fed, step, list(out))
        n_emit, finished = accept(d, len(d), a, step, max_new, min_len, eos, stop_on_eos)
        out += [int(t) for t in a[:n_emit]]
        hist += [int(t) for t in a[:n_emit]]
        steps += 1
    return out, steps
