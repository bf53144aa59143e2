"""Inputs shared by tests/test_ngram_host.py (CPU) and tests/test_gpu_ngram.py: histories with planted repetitions for the sample
kernel, the multi-step beam scenarios with their torch reference (computed once per case and never modified), and the n-gram
property check of generated ids."""
import functools

import torch

from emu_amd import sampling
from emu_amd.llama import beam_host_scores

EOS, PAD = 2, 32000
BF16 = torch.bfloat16
THREADS = 1024                                        # the sample kernel's workgroup
CHAT = dict(temperature=0.7, top_p=0.9)               # the chat demo's options
PEN = dict(repetition_penalty=1.3, top_k=50, top_p=0.9)


def alphabet_history(rows, cur, g):
    """ids from a 6-symbol alphabet: repeats are everywhere (the construction of tests/test_host_logic.py:513)."""
    return torch.randint(3, 9, (rows, cur), generator=g)


def planted_targets(V):
    """The ids a planted ban is aimed at: the first id, the last, and the first id of the last owning thread's chunk (a partial chunk
    wherever V is no multiple of the chunk; chunks are odd: sample_common.h)."""
    C = ((V + THREADS - 1) // THREADS) | 1
    last_chunk = ((V - 1) // C) * C
    out = [0, V - 1, last_chunk if last_chunk not in (0, V - 1) else V // 2]
    assert len(set(out)) == 3
    return out


def planted_row(V, n, nh, f, g):
    """(history of nh ids, planted?): the last n - 1 ids occur earlier followed by ``f`` and nowhere else, so ``f`` is banned by
    construction -- wherever nh leaves room for a repetition at all (nh >= n); otherwise nh distinct ids and no ban."""
    pool = [t for t in (torch.randperm(V - 3, generator=g) + 3).tolist() if t != f]
    if nh < n:
        return pool[:nh], False
    if nh < 2 * n - 1:                                # the occurrence and the tail overlap: a run of one id is the only shape
        return [f] * nh, True
    gram, fill = pool[:n - 1], pool[n - 1:]
    p = int(torch.randint(0, nh - (2 * n - 1) + 1, (1,), generator=g))
    h = fill[:p] + gram + [f] + fill[p:nh - (2 * n - 1)] + gram
    assert len(h) == nh
    return h, True


def planted_case(V, rows, n, step, k, hist_rows=None, seed=0):
    """Logits [rows, V] bf16 and a history per row with a planted ban on ``planted_targets(V)[(row + k) % 3]``, whose logit is raised
    to the row maximum: the unbanned arg-max is banned by construction.  The history is ``min(step, hist_rows)`` long, as the kernel
    reads it.  Returns (x, hist int64 [rows, nh], targets, planted flags)."""
    g = torch.Generator().manual_seed(seed * 7919 + V * 31 + n * 7 + step + k)
    nh = step if hist_rows is None else min(step, hist_rows)
    x = (torch.randn(rows, V, generator=g) * 3.0).to(BF16)
    tg = planted_targets(V)
    hist, targets, flags = [], [], []
    for r in range(rows):
        f = tg[(r + k) % 3]
        h, planted = planted_row(V, n, nh, f, g)
        x[r, f] = x[r].float().max() + 1.0
        hist.append(h); targets.append(f); flags.append(planted)
    return x, torch.tensor(hist, dtype=torch.int64).reshape(rows, nh), targets, flags


def has_repeated_ngram(row, n, pad=PAD):
    """Does the row hold one n-gram twice among its ids ahead of the padding?"""
    ids = [t for t in row if t != pad]
    grams = [tuple(ids[i:i + n]) for i in range(len(ids) - n + 1)]
    return len(grams) != len(set(grams))


# ------------------------------------------------------------------------------------------------ beam scenarios
BEAM_SHAPES = [(1, 5, 32274, 12), (2, 3, 64, 24), (2, 8, 4096, 10)]


def magnets(V):
    """Three ids every row favours, so that beams repeat n-grams: first chunk, a middle chunk, the (partial) last chunk."""
    return [5, 17000, 32270] if V == 32274 else [5, V // 2, V - 4]


def torch_step(st, lp_rows, cur, min_len, max_len, length_penalty, eos_id, v431=False, ngram=0):
    """tests/test_gpu_beam.py::torch_step (one iteration of the host loop of emu_amd/llama.py::beam_search_generate, the stable
    top-2N) with the host loop's ``process_logits(..., no_repeat_ngram_size=ngram)`` on the log-probabilities."""
    B, nb, V = lp_rows.shape
    acc = beam_host_scores(lp_rows, st["running_scores"], st["running_seq"], cur, min_len, eos_id, ngram=ngram)
    top_lp, top_idx = sampling.beam_reference_select(acc, nb, None, False)
    return sampling.beam_scorer_step(st, top_lp, top_idx, V, cur, max_len, length_penalty, eos_id, v431)[:2]


# shape -> seed, screened with the torch pipeline on the CPU (the first of 0, 1, 2, ... to qualify): for n = 1, 2, 3 and both scorer
# conventions some beam row has a non-empty banned set at EVERY step from n on (tests/test_ngram_host.py asserts it)
BEAM_SEEDS = {(1, 5, 32274, 12): 3, (2, 3, 64, 24): 20, (2, 8, 4096, 10): 0}


def beam_logits(B, nb, V, L):
    """The bf16 logits of every step ([B, V] at step 0, where the beams share the prompt's row, then [B * nb, V]): unit normal
    (the largest of 32 274 draws is about 4), the magnets raised by 8 on every row."""
    g = torch.Generator().manual_seed(BEAM_SEEDS[(B, nb, V, L)] * 7919 + B * 1000 + nb * 10 + L)
    out = []
    for cur in range(L):
        x = torch.randn(B if cur == 0 else B * nb, V, generator=g)
        x[:, magnets(V)] += 8.0
        out.append(x.to(BF16))
    return out


# length_penalty 0: Emu1's own caption setting, the reference's user of the ban (Emu1/models/modeling_emu.py:110).  (Under -1 a kept
# score is the sum TIMES the length: at 24 tokens one fp32 ulp of such a score is already above the 1e-4 the kernel tests compare to.)
BEAM_MIN_LEN, BEAM_LP = 1, 0.0


@functools.lru_cache(maxsize=None)
def beam_scenario(B, nb, V, L, n, v431):
    """The deterministic search of ``beam_logits`` under the ban n, by the torch pipeline on the CPU: per step (logits, state after
    it, tokens to feed, cache rows, number of beam rows with a non-empty banned set), computed once and shared."""
    st = sampling.beam_start_state(B, nb, L, PAD)
    steps = []
    for cur, lg in enumerate(beam_logits(B, nb, V, L)):
        rows = lg.float()[:, None, :].expand(B, nb, V) if cur == 0 else lg.float().view(B, nb, V)
        banned = sampling.banned_ngram_mask(st["running_seq"][:, :, :cur].reshape(B * nb, cur), n, V)
        toks, flat = torch_step(st, rows, cur, BEAM_MIN_LEN, L, BEAM_LP, EOS, v431, ngram=n)
        steps.append(dict(lg=lg, state={k: v.clone() for k, v in st.items()}, toks=toks.clone(), flat=flat.clone(),
                          banned_rows=int(banned.any(dim=1).sum())))
    return steps
