"""Specification of the device sampler (emu_amd/csrc/sample.hip, ``emu_sample_bf16``) in pure torch: what the kernel computes for
one row of bf16 logits, the ids generated so far, the sampling options and one uniform ``u`` in [0, 1).  It plays the role
``emu_amd/mxfp4.py`` plays for the 4-bit format: the kernel is tested against this file, and this file against the host pipeline
(``emu_amd.llama.process_logits``, itself pinned to transformers' processors).

The order is transformers' order:

1. ``s = float32(logit)``.
2. Repetition penalty: for every DISTINCT history id in [0, vocab): ``s = s * pen if s < 0 else s / pen`` (IEEE fp32 multiply and
   divide), once per id however often it occurs; ids outside [0, vocab) are ignored.
3. Minimum-length suppress: ``s[suppress_id] = -inf`` (``suppress_id`` None or < 0: not applied).
4. ``do_sample`` false ends here: the token is the first index of the maximum (``argmax_kernel``'s rule).
5. Temperature: ``s = s / temperature`` (IEEE fp32 division), skipped for None or 1.
6. Top-k: with k' = min(max(top_k, min_keep), vocab), drop ``s < (k'-th largest value)``; ties with that value stay.
7. Top-p: with p = softmax(s), token i stays iff the mass of {j : s_j <= s_i} exceeds 1 - top_p, or s_i >= the min_keep-th largest
   value.  This is transformers' ascending-sort rule whenever the group of tokens AT the threshold value has one member.  With ties
   at the threshold -- bf16 logits make them real: a vocabulary of 32 274 drawn from a few thousand distinct bf16 values -- this
   rule keeps the whole tied group where the library's sort keeps whatever part of it the sort happened to place last, so the kept
   set here is a superset of the library's that differs from it only inside that one group (and does not depend on a sort's tie
   order).
8. Draw: q = softmax over the kept tokens; the token is the lowest id whose inclusive cumulative q in ASCENDING ID order exceeds u;
   if rounding leaves u at or beyond the total, the highest kept id.

Steps 1-6 are always done in fp32, so the scores -- and with them every comparison between scores -- are the kernel's bit for bit.
``dtype=torch.float64`` widens only the softmax, the masses of step 7 and the sums of step 8: the tests' yardstick for the kernel's
fp32 sums.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import torch

History = Union[None, torch.Tensor, Sequence[Sequence[int]]]


def _history_rows(history: History, B: int):
    if history is None:
        return [[] for _ in range(B)]
    if isinstance(history, torch.Tensor):
        return [[int(v) for v in r] for r in history.reshape(B, -1).tolist()]
    return [list(map(int, r)) for r in history]


def reference_scores(logits: torch.Tensor, history: History = None, repetition_penalty: float = 1.0,
                     suppress_id: Optional[int] = None) -> torch.Tensor:
    """Steps 1-3: [B, vocab] fp32 scores of bf16 (or fp32-held bf16) logit rows."""
    s = logits.float().clone()
    B, V = s.shape
    if repetition_penalty != 1.0:
        pen = torch.tensor(float(repetition_penalty), dtype=torch.float32)
        for b, row in enumerate(_history_rows(history, B)):
            ids = sorted({i for i in row if 0 <= i < V})
            if ids:
                idx = torch.tensor(ids, dtype=torch.int64, device=s.device)
                g = s[b, idx]
                s[b, idx] = torch.where(g < 0, g * pen.to(s.device), g / pen.to(s.device))
    if suppress_id is not None and 0 <= suppress_id < V:
        s[:, suppress_id] = -float("inf")
    return s


def reference_greedy(logits: torch.Tensor, history: History = None, repetition_penalty: float = 1.0,
                     suppress_id: Optional[int] = None) -> torch.Tensor:
    """Step 4: first index of the maximum of the penalised, suppressed scores, [B] int64."""
    s = reference_scores(logits, history, repetition_penalty, suppress_id)
    first = (s == s.max(dim=-1, keepdim=True)[0]).float().argmax(dim=-1)       # argmax of a 0/1 row: the first 1
    return first


def reference_warped(logits: torch.Tensor, history: History = None, repetition_penalty: float = 1.0,
                     suppress_id: Optional[int] = None, temperature: Optional[float] = None, top_k: Optional[int] = None,
                     top_p: Optional[float] = None, min_keep: int = 1, dtype: torch.dtype = torch.float32
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Steps 1-7: (scores [B, vocab] fp32 after temperature, kept [B, vocab] bool)."""
    s = reference_scores(logits, history, repetition_penalty, suppress_id)
    B, V = s.shape
    if temperature is not None and temperature != 1.0:
        s = s / torch.tensor(float(temperature), dtype=torch.float32, device=s.device)
    kept = torch.ones_like(s, dtype=torch.bool)
    if top_k is not None and top_k > 0:
        kk = min(max(int(top_k), int(min_keep)), V)
        kth = torch.topk(s, kk, dim=-1)[0][:, -1:]
        kept = s >= kth
    if top_p is not None and top_p < 1.0:
        sk = s.masked_fill(~kept, -float("inf"))
        p = torch.softmax(sk.to(dtype), dim=-1)
        # mass of {j : s_j <= s_i}: cumulative mass in ascending score order, taken at the END of every group of equal scores
        srt, idx = torch.sort(sk, dim=-1, descending=False, stable=True)
        cum = torch.gather(p, 1, idx).cumsum(dim=-1)
        last_of_group = torch.ones_like(srt, dtype=torch.bool)
        last_of_group[:, :-1] = srt[:, :-1] != srt[:, 1:]
        pos = torch.arange(V, device=s.device).expand(B, V)
        end = torch.where(last_of_group, pos, torch.full_like(pos, V)).flip(-1).cummin(dim=-1)[0].flip(-1)   # group end per position
        mass_sorted = torch.gather(cum, 1, end)
        thr = torch.tensor(1.0 - float(top_p), dtype=torch.float32).to(dtype)      # the host path compares in fp32 with this value
        keep_sorted = mass_sorted > thr
        keep_p = torch.zeros_like(kept).scatter(1, idx, keep_sorted)
        mk = min(int(min_keep), V)
        keep_p |= sk >= torch.topk(sk, mk, dim=-1)[0][:, -1:]
        kept = kept & keep_p
    return s, kept


def reference_probs(logits: torch.Tensor, history: History = None, repetition_penalty: float = 1.0,
                    suppress_id: Optional[int] = None, do_sample: bool = True, temperature: Optional[float] = None,
                    top_k: Optional[int] = None, top_p: Optional[float] = None, min_keep: int = 1,
                    dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """[B, vocab] probabilities the draw is made from (``dtype``), exactly 0 for removed tokens.  ``do_sample`` false: the one-hot
    row of the greedy token."""
    if not do_sample:
        g = reference_greedy(logits, history, repetition_penalty, suppress_id)
        return torch.zeros(logits.shape, dtype=dtype, device=logits.device).scatter_(1, g[:, None], 1.0)
    s, kept = reference_warped(logits, history, repetition_penalty, suppress_id, temperature, top_k, top_p, min_keep, dtype)
    q = torch.softmax(s.masked_fill(~kept, -float("inf")).to(dtype), dim=-1)
    return q.masked_fill(~kept, 0.0)


def reference_intervals(probs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lo, hi) [B, vocab]: token i is drawn for u in [lo_i, hi_i) -- the cumulative probability in ascending id order before and
    after it.  A removed token has an empty interval."""
    hi = probs.cumsum(dim=-1)
    return hi - probs, hi


def reference_draw(probs: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """Step 8: [B] int64, the lowest id whose inclusive cumulative probability exceeds u [B]; the highest kept id when rounding
    leaves u at or beyond the total."""
    V = probs.shape[-1]
    hi = probs.cumsum(dim=-1)
    over = (hi > u.to(hi.dtype)[:, None]) & (probs > 0)
    pos = torch.arange(V, device=probs.device).expand_as(probs)
    first = torch.where(over, pos, torch.full_like(pos, V)).min(dim=-1)[0]
    last_kept = torch.where(probs > 0, pos, torch.full_like(pos, -1)).max(dim=-1)[0]
    return torch.where(first < V, first, last_kept)


def top_p_threshold_group(logits: torch.Tensor, **opts) -> Tuple[torch.Tensor, torch.Tensor]:
    """For the tests' screening of their inputs: per row (the number of tokens that share the lowest kept score, the distance of
    the top-p decision from its bound: min over the distinct scores of |mass{s_j <= s} - (1 - top_p)|).  Same options as
    ``reference_warped``; rows without a top-p cut report (1, inf)."""
    top_p = opts.get("top_p")
    s, kept = reference_warped(logits, **opts)
    B, V = s.shape
    if top_p is None or top_p >= 1.0:
        return torch.ones(B, dtype=torch.int64), torch.full((B,), float("inf"), dtype=torch.float64)
    low = s.masked_fill(~kept, float("inf")).min(dim=-1, keepdim=True)[0]
    group = (s == low).sum(dim=-1)
    o64 = dict(opts, top_p=None, dtype=torch.float64)
    s2, kept_k = reference_warped(logits, **o64)                       # the set top-p acts on
    sk = s2.masked_fill(~kept_k, -float("inf"))
    p = torch.softmax(sk.double(), dim=-1)
    srt, idx = torch.sort(sk, dim=-1)
    cum = torch.gather(p, 1, idx).cumsum(dim=-1)
    margin = (cum - float(torch.tensor(1.0 - float(top_p), dtype=torch.float32))).abs()
    last = torch.ones_like(srt, dtype=torch.bool)
    last[:, :-1] = srt[:, :-1] != srt[:, 1:]
    margin = margin.masked_fill(~last | torch.isinf(srt), float("inf")).min(dim=-1)[0]
    return group, margin
