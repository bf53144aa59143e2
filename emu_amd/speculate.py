"""Prompt-lookup speculative greedy decoding, specified in pure torch / Python: what ``csrc/lookup.hip`` computes on the device.

The option is the library's ``lm.generate(prompt_lookup_num_tokens=k, max_matching_ngram_size=n)``, which the reference reaches
through the ``**kwargs`` of ``Emu2/emu/emu.py:175,228``.  A step feeds the last emitted id and up to k guessed ids through the model
at once (one few-row step costs about one token's time), and keeps the guessed ids for as long as each equals the arg-max of the
row before it -- so every emitted id is the arg-max of the model's own logits, and the output is the greedy one.

``lookup_draft`` restates ``PromptLookupCandidateGenerator.get_candidates`` (checked against the installed library in
``tests/test_speculate_host.py``); ``accept`` is the verification; ``simulate`` runs the whole loop on a table of arg-maxes, which
is how the tests predict ``steps_run``.  Imports nothing from the engine."""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import torch

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
