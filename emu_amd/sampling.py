"""Specification of the device sampler (emu_amd/csrc/sample.hip, ``emu_sample_bf16``) in pure torch: what the kernel computes for
one row of bf16 logits, the ids generated so far, the sampling options and one uniform ``u`` in [0, 1).  It plays the role
``emu_amd/mxfp4.py`` plays for the 4-bit format: the kernel is tested against this file, and this file against the host pipeline
(``emu_amd.llama.process_logits``, itself pinned to transformers' processors).

The order is transformers' order:

1. ``s = float32(logit)``.
2. Repetition penalty: for every DISTINCT history id in [0, vocab): ``s = s * pen if s < 0 else s / pen`` (IEEE fp32 multiply and
   divide), once per id however often it occurs; ids outside [0, vocab) are ignored.
2a. No-repeat n-gram ban (``banned`` bool [rows, vocab], None = none: ``banned_ngram_mask`` of the ids generated so far; the place
   of the library's NoRepeatNGramLogitsProcessor, after the penalty and ahead of the suppress): ``s[banned] = -inf``.  This, the
   suppress and the constraint are masks: after the penalty their order does not matter.
3. Minimum-length suppress: ``s[suppress_id] = -inf`` (``suppress_id`` None or < 0: not applied).
3a. Constraint (``allowed`` bool [rows, vocab], None = none; the place of the library's PrefixConstrainedLogitsProcessor):
   ``s[~allowed] = -inf``, so everything below -- the arg-max, the thresholds, the softmax -- runs over the allowed ids.
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


def banned_ngram_mask(history: History, n: int, vocab: int) -> torch.Tensor:
    """Step 2a's mask, bool [rows, vocab] (``history`` [rows, nh] or a list of rows: the ids each row has generated so far; with
    ``inputs_embeds`` the prompt contributes none).  With h[0 .. nh) a row's ids, ``banned[v]`` holds iff nh + 1 >= n and there is
    an i in [0, nh - n + 1) with h[i .. i + n - 1) == h[nh - n + 1 .. nh) (an empty comparison for n = 1) and h[i + n - 1] == v:
    v would complete an n-gram the row already holds.  A would-be banned id outside [0, vocab) is ignored; n < 1 means off."""
    if isinstance(history, torch.Tensor):              # (a [rows, 0] tensor -- nothing generated yet -- has no -1 to reshape to)
        rows = [[int(v) for v in r] for r in history.tolist()]
    else:
        rows = _history_rows(history, len(history))
    mask = torch.zeros(len(rows), int(vocab), dtype=torch.bool)
    n = int(n)
    if n < 1:
        return mask
    for r, h in enumerate(rows):
        nh = len(h)
        if nh + 1 < n:
            continue
        tail = h[nh - n + 1:]
        for i in range(nh - n + 1):
            if h[i:i + n - 1] == tail and 0 <= h[i + n - 1] < vocab:
                mask[r, h[i + n - 1]] = True
    return mask


def reference_scores(logits: torch.Tensor, history: History = None, repetition_penalty: float = 1.0,
                     suppress_id: Optional[int] = None, allowed: Optional[torch.Tensor] = None,
                     banned: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Steps 1-3a: [B, vocab] fp32 scores of bf16 (or fp32-held bf16) logit rows."""
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
    if banned is not None:
        s = s.masked_fill(banned.to(device=s.device, dtype=torch.bool), -float("inf"))
    if suppress_id is not None and 0 <= suppress_id < V:
        s[:, suppress_id] = -float("inf")
    if allowed is not None:
        s = s.masked_fill(~allowed.to(device=s.device, dtype=torch.bool), -float("inf"))
    return s


def reference_greedy(logits: torch.Tensor, history: History = None, repetition_penalty: float = 1.0,
                     suppress_id: Optional[int] = None, allowed: Optional[torch.Tensor] = None,
                     banned: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Step 4: first index of the maximum of the penalised, suppressed scores, [B] int64."""
    s = reference_scores(logits, history, repetition_penalty, suppress_id, allowed, banned)
    first = (s == s.max(dim=-1, keepdim=True)[0]).float().argmax(dim=-1)       # argmax of a 0/1 row: the first 1
    return first


def reference_warped(logits: torch.Tensor, history: History = None, repetition_penalty: float = 1.0,
                     suppress_id: Optional[int] = None, temperature: Optional[float] = None, top_k: Optional[int] = None,
                     top_p: Optional[float] = None, min_keep: int = 1, dtype: torch.dtype = torch.float32,
                     allowed: Optional[torch.Tensor] = None,
                     banned: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Steps 1-7: (scores [B, vocab] fp32 after temperature, kept [B, vocab] bool)."""
    s = reference_scores(logits, history, repetition_penalty, suppress_id, allowed, banned)
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
                    dtype: torch.dtype = torch.float32, allowed: Optional[torch.Tensor] = None,
                    banned: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B, vocab] probabilities the draw is made from (``dtype``), exactly 0 for removed tokens.  ``do_sample`` false: the one-hot
    row of the greedy token."""
    if not do_sample:
        g = reference_greedy(logits, history, repetition_penalty, suppress_id, allowed, banned)
        return torch.zeros(logits.shape, dtype=dtype, device=logits.device).scatter_(1, g[:, None], 1.0)
    s, kept = reference_warped(logits, history, repetition_penalty, suppress_id, temperature, top_k, top_p, min_keep, dtype, allowed,
                               banned)
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


# ---------------------------------------------------------------------------------------------------------------------------------
# Beam-search sampling and penalised beam search (emu_amd/csrc/beam_sample.hip, ``emu_beam_sample_step_bf16``): what the two kernels
# compute for the nb beam rows of every prompt.  Tested against the host pipeline of ``LlamaEngine.beam_search_generate``
# (``log_softmax`` -> ``process_logits(min_keep=2)`` / ``warp_logits`` in the order's sequence), which with a table of uniforms draws by
# ``beam_reference_select``.
#
# Per beam row (b, j), from its bf16 logits, the ids the beam has generated, its running score rs_j and the options:
#
# 1. ``lp = x - (m + log sum exp(x - m))`` with ``x = float32(logit)`` and m the row maximum; the subtraction is fp32, the sum is taken
#    in ``dtype``.
# 2. The processors act on lp: the repetition penalty of step 2 above (``lp < 0`` multiplies, otherwise divides; once per distinct
#    history id; ids outside the vocabulary are ignored), then the n-gram ban ``lp[banned] = -inf`` (step 2a above, over the beam's own
#    ids), then ``lp[eos] = -inf`` while ``cur < min_len``, then the constraint: ``lp[~allowed] = -inf`` (the log-sum-exp of step 1 is
#    over the whole, unmasked row for all three).
# 3. The warpers are steps 5-7 above with ``min_keep = 2``.  ``order="5.x"``: they act on lp, and ``acc = warped + rs_j``;
#    ``order="4.31"``: they act on ``lp + rs_j`` and acc is that warped row; ``do_sample=False`` (penalised beam search): no warpers,
#    ``acc = lp + rs_j``.  All these sums are fp32; removed entries are -inf.
#
# Per prompt, over the flattened [nb * V] scores (flat index = j * V + id):
#
# * ``do_sample=False``: the 2N best; ties go to the lower flat index (beam.hip's rule).
# * ``do_sample=True``: 2N draws without replacement, one uniform u_k each.  ``p = softmax(acc)`` in ``dtype``.  Draw k takes the
#   lowest flat index not yet drawn whose inclusive cumulative mass -- over the not-yet-drawn entries only, in ascending flat index --
#   exceeds ``u_k * R_k``, R_k the mass that remains; if rounding leaves ``u_k * R_k`` at or beyond the total, the highest remaining
#   entry of positive mass.  When no positive mass remains (the "5.x" start: beams 1..N-1 carry -1e9, and with top_k = 3 beam 0 alone
#   cannot supply ten tokens) the draw takes the lowest not-yet-drawn flat index whose acc is finite; removed entries are never drawn
#   (with ``min_keep = 2`` there are always at least 2N finite entries).  Under ``order="4.31"`` the 2N draws are then sorted by score,
#   descending, stably: equal scores keep draw order.
# * The results are ``top_idx`` and ``top_lp = acc[top_idx]``, which the scorer's bookkeeping (``beam_scorer_step`` below) consumes
#   unchanged.

BEAM_MIN_KEEP = 2          # the library's min_tokens_to_keep under beam search: one EOS id + 1


def _check_order(order: str) -> bool:
    if order not in ("4.31", "5.x"):
        raise ValueError("order must be '4.31' or '5.x'")
    return order == "4.31"


def _beam_processed(logits, history, repetition_penalty, eos_id, suppress_eos, dtype, allowed=None, banned=None):
    """Steps 1-2: the penalised, n-gram-banned, EOS-suppressed, constrained log-probabilities [R, vocab] fp32."""
    x = logits.float()
    m = x.max(dim=-1, keepdim=True)[0]
    lse = m + torch.log(torch.exp((x - m).to(dtype)).sum(dim=-1, keepdim=True)).float()
    return reference_scores(x - lse, history, repetition_penalty, eos_id if suppress_eos else None, allowed, banned)


def beam_reference_warp_input(logits: torch.Tensor, running_scores: torch.Tensor, history: History = None,
                              repetition_penalty: float = 1.0, eos_id: Optional[int] = None, suppress_eos: bool = False,
                              order: str = "5.x", dtype: torch.dtype = torch.float32,
                              allowed: Optional[torch.Tensor] = None, banned: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The fp32 rows [R, vocab] the warpers act on (ahead of the temperature): steps 1-2, under ``order="4.31"`` with the running
    score added."""
    lp = _beam_processed(logits, history, repetition_penalty, eos_id, suppress_eos, dtype, allowed, banned)
    return lp + running_scores.reshape(-1, 1).float().to(lp.device) if _check_order(order) else lp


def beam_reference_rows(logits: torch.Tensor, running_scores: torch.Tensor, history: History = None,
                        repetition_penalty: float = 1.0, eos_id: Optional[int] = None, suppress_eos: bool = False,
                        do_sample: bool = True, temperature: Optional[float] = None, top_k: Optional[int] = None,
                        top_p: Optional[float] = None, order: str = "5.x", dtype: torch.dtype = torch.float32,
                        allowed: Optional[torch.Tensor] = None, banned: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Steps 1-3: acc [R, vocab] fp32 of R beam rows (bf16 or fp32-held bf16 logits [R, vocab], running scores [R] or [B, nb], one
    history per row), -inf for removed entries."""
    accumulated = _check_order(order)
    rs = running_scores.reshape(-1, 1).float().to(logits.device)
    if not do_sample:
        return _beam_processed(logits, history, repetition_penalty, eos_id, suppress_eos, dtype, allowed, banned) + rs
    w = beam_reference_warp_input(logits, running_scores, history, repetition_penalty, eos_id, suppress_eos, order, dtype, allowed,
                                  banned)
    s, kept = reference_warped(w, None, 1.0, None, temperature, top_k, top_p, BEAM_MIN_KEEP, dtype)
    return (s if accumulated else s + rs).masked_fill(~kept, -float("inf"))


def beam_reference_probs(acc: torch.Tensor, nb: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """[B, nb * vocab] probabilities the draws are made from (``dtype``): softmax over the flattened rows of every prompt, exactly
    0 for removed entries.  ``acc`` [B * nb, vocab] or [B, nb, vocab]."""
    flat = acc.reshape(-1, nb * acc.shape[-1])
    p = torch.softmax(flat.to(dtype), dim=-1)
    return p.masked_fill(torch.isinf(flat) & (flat < 0), 0.0)


def _draw_state(p_row: torch.Tensor, drawn):
    rem = p_row.clone()
    if drawn:
        rem[torch.tensor(list(drawn), dtype=torch.int64, device=p_row.device)] = 0
    return rem


def _draw_one(rem: torch.Tensor, finite: torch.Tensor, u) -> int:
    """One draw from the remaining masses ``rem`` (drawn entries zeroed; ``finite`` marks the not-yet-drawn entries of finite acc)."""
    R = rem.sum()
    if not bool(R > 0):
        return int(torch.nonzero(finite)[0])
    target = torch.as_tensor(u, dtype=rem.dtype, device=rem.device) * R
    over = (rem.cumsum(dim=0) > target) & (rem > 0)
    hit = torch.nonzero(over)
    if hit.numel():
        return int(hit[0])
    return int(torch.nonzero(rem > 0)[-1])


def beam_reference_select(acc: torch.Tensor, nb: int, uniforms: Optional[torch.Tensor] = None, do_sample: bool = True,
                          order: str = "5.x", dtype: torch.dtype = torch.float32, return_draws: bool = False):
    """The selection per prompt: (top_lp [B, 2 nb] fp32, top_idx [B, 2 nb] int64) of ``acc`` [B * nb, vocab] or [B, nb, vocab];
    ``uniforms`` [B, 2 nb] when sampling.  ``return_draws`` adds the flat indices in draw order (before the "4.31" sort)."""
    accumulated = _check_order(order)
    flat = acc.reshape(-1, nb * acc.shape[-1])
    B, n2 = flat.shape[0], 2 * nb
    if not do_sample:
        # stable descending order: equal scores keep ascending flat index
        idx = torch.sort(flat, dim=-1, descending=True, stable=True)[1][:, :n2]
        return (torch.gather(flat, 1, idx), idx, idx) if return_draws else (torch.gather(flat, 1, idx), idx)
    p = beam_reference_probs(acc, nb, dtype)
    u = uniforms.to(torch.float32).cpu()
    draws = torch.empty(B, n2, dtype=torch.int64)
    for b in range(B):
        rem = p[b].clone()
        finite = ~(torch.isinf(flat[b]) & (flat[b] < 0))
        for k in range(n2):
            i = _draw_one(rem, finite, float(u[b, k]))
            draws[b, k] = i
            rem[i] = 0
            finite[i] = False
    draws = draws.to(flat.device)
    top_idx = draws
    top_lp = torch.gather(flat, 1, top_idx)
    if accumulated:
        top_lp, o = torch.sort(top_lp, descending=True, dim=1, stable=True)
        top_idx = torch.gather(top_idx, 1, o)
    return (top_lp, top_idx, draws) if return_draws else (top_lp, top_idx)


def beam_draw_intervals(acc_flat: torch.Tensor, drawn) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """For one prompt's flattened acc [nb * vocab] with the flat indices ``drawn`` already taken: (lo, hi, R) in fp64 and in units of
    the INITIAL total mass (softmax(acc) sums to 1): entry i is drawn for ``u * R`` in [lo_i, hi_i), R the mass that remains."""
    p = beam_reference_probs(acc_flat[None], 1, torch.float64)[0]
    rem = _draw_state(p, drawn)
    hi = rem.cumsum(dim=0)
    return hi - rem, hi, rem.sum()


def beam_draw_margin(acc: torch.Tensor, nb: int, uniforms: torch.Tensor, draws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """For the tests' screening of their inputs, per prompt and draw [B, 2 nb] fp64: the distance of ``u_k * R_k`` from the nearest
    boundary between two remaining entries of positive mass, in units of the initial total mass (the draws 0..k-1 removed: those
    of ``draws``, default the fp64 spec's own).  The two ends of the remaining mass, 0 and R_k, are not decisions (below the first
    entry's end or beyond the total the rule names one entry whatever the rounding), so a draw with a single entry of positive mass
    left, and a draw by the zero-mass rule, report inf."""
    flat = acc.reshape(-1, nb * acc.shape[-1])
    B, n2 = uniforms.shape
    if draws is None:
        draws = beam_reference_select(acc, nb, uniforms, True, "5.x", torch.float64, return_draws=True)[2]
    out = torch.full((B, n2), float("inf"), dtype=torch.float64)
    for b in range(B):
        for k in range(n2):
            lo, hi, R = beam_draw_intervals(flat[b], [int(v) for v in draws[b, :k]])
            pos = hi[(hi - lo) > 0]
            if pos.numel() < 2:
                continue
            t = float(torch.tensor(float(uniforms[b, k]), dtype=torch.float64) * R)
            out[b, k] = float((pos[:-1] - t).abs().min())
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# The beam scorer's bookkeeping (the second half of ``emu_beam_step_bf16`` / ``emu_beam_sample_step_bf16`` and of their trie and
# n-gram variants): what one step does with the 2N candidates ``top_lp`` / ``top_idx`` of every prompt, whichever selection made them.
# ``beam_scorer_step`` IS the host loop's step (``LlamaEngine.beam_search_generate`` calls it) and the kernels are tested against it;
# tests/golden/beam_scorer_steps.npz pins it bit for bit to the statements as they stood inline in that loop.
#
# State per prompt (``beam_start_state``): N running beams (ids ``running_seq``, summed log-probabilities ``running_scores``), N kept
# results (``sequences``, ``beam_scores`` = score / len ** length_penalty, ``finished``, ``seq_len``), and ``open``: may a running beam
# still beat the worst kept result?  -1e9 (``BEAM_NEG``) marks an empty slot; it is ADDED to a score to take a candidate out.
#
# 1. Candidate k continues beam ``top_idx // V`` with token ``top_idx % V``.  It is a hit if the token is EOS or -- 5.x only -- the step
#    is the last one.
# 2. The N best non-hits, in candidate order among equals, are the running beams of the next step.
# 3. A hit among the FIRST N candidates competes with the kept results at ``top_lp / n ** length_penalty``, n = cur + 1 tokens (4.31:
#    the cur tokens ahead of the EOS, 1 at step 0), unless the prompt is closed; the N best of kept + new stay.
# 4. ``open`` stays set while a kept slot is still empty or ``best / (cur + 1) ** length_penalty`` beats the worst kept result, best =
#    the first running beam (4.31: the first candidate, an EOS one included).
# 5. 4.31, last step: the running beams join the kept results at ``score / L ** length_penalty`` unless the prompt is closed (``finalize``).
#
# Every top-k is over at most 3N entries; ``stable`` settles its ties by position (the kernels' rule), otherwise ``torch.topk`` does.

BEAM_NEG = -1.0e9


def beam_start_state(B: int, nb: int, L: int, pad_id: int, device=None, equal_start: bool = False) -> dict:
    """The state a search of B prompts x nb beams over at most L tokens starts from.  Beam 0 alone carries score 0 (at step 0 every
    beam holds the same hypothesis); ``equal_start``: all do (4.31's ``beam_sample``: the draws tell them apart).  ``top_mask`` is the
    constant "only the first N candidates may finish" of step 3."""
    st = dict(running_seq=torch.full((B, nb, L), pad_id, dtype=torch.int64, device=device),
              running_scores=torch.zeros(B, nb, device=device), beam_scores=torch.full((B, nb), BEAM_NEG, device=device),
              finished=torch.zeros(B, nb, dtype=torch.bool, device=device), seq_len=torch.zeros(B, nb, dtype=torch.int64, device=device),
              open=torch.ones(B, 1, dtype=torch.bool, device=device))
    st["sequences"] = st["running_seq"].clone()
    if not equal_start:
        st["running_scores"][:, 1:] = BEAM_NEG
    st["top_mask"] = torch.cat([torch.ones(nb, dtype=torch.bool, device=device), torch.zeros(nb, dtype=torch.bool, device=device)])
    return st


def beam_topk(t: torch.Tensor, k: int, stable: bool = True):
    """(values, indices) [B, k] of the k largest per row of ``t`` [B, n], descending.  ``stable``: equal values keep ascending index (the
    kernels' rule); otherwise ``torch.topk``, which leaves ties open."""
    if not stable:
        return torch.topk(t, k)
    return tuple(r[:, :k] for r in torch.sort(t, dim=1, descending=True, stable=True))


def beam_scorer_step(st: dict, top_lp: torch.Tensor, top_idx: torch.Tensor, V: int, cur: int, max_len: int, length_penalty: float,
                     eos_id: int, v431: bool, stable: bool = True):
    """Steps 1-5 for step ``cur`` on the candidates ``top_lp`` / ``top_idx`` [B, 2 nb]; updates ``st`` in place.  Returns (the tokens to
    feed [B * nb] int64, the cache rows they continue [B * nb], the beam each new beam continues [B, nb], the candidates' scores with
    the hits taken out [B, 2 nb]).  No host read."""
    B, nb = st["running_scores"].shape
    dev, NEG = top_lp.device, BEAM_NEG
    running_seq, sequences, beam_scores, finished, seq_len, heuristic_open = (
        st["running_seq"], st["sequences"], st["beam_scores"], st["finished"], st["seq_len"], st["open"])
    topk = lambda t, k: beam_topk(t, k, stable)
    gather = lambda t, idx: torch.gather(t, 1, idx.reshape(B, -1, *([1] * (t.dim() - 2))).expand(-1, -1, *t.shape[2:]))
    src_beam = top_idx // V
    tok = top_idx % V
    cand_seq = gather(running_seq, src_beam)
    cand_seq[:, :, cur] = tok
    at_limit = cur + 1 >= max_len
    # 4.31: at the length limit the non-EOS candidates still become running beams (finalize adds them below)
    hits = (tok == eos_id) if v431 else (tok == eos_id) | at_limit
    # running beams for the next step: best N non-finished candidates
    run_lp = top_lp + hits.float() * NEG
    nxt = topk(run_lp, k=nb)[1]
    running_seq = gather(cand_seq, nxt)
    running_scores = torch.gather(run_lp, 1, nxt)
    beam_idx = torch.gather(src_beam, 1, nxt)                                   # which old beam each new beam extends
    # finished results: only the top-N candidates may finish; merge with the kept ones
    # 4.31 BeamHypotheses.add: an EOS hypothesis is scored over the cur tokens ahead of the EOS
    fin_lp = top_lp / float((cur if (v431 and cur > 0) else cur + 1) ** length_penalty)
    fin_lp = fin_lp + (~heuristic_open).float() * NEG
    just = hits & st["top_mask"][None, :]
    fin_lp = fin_lp + (~just).float() * NEG
    m_seq = torch.cat((sequences, cand_seq), dim=1)
    m_sc = torch.cat((beam_scores, fin_lp), dim=1)
    m_fin = torch.cat((finished, just), dim=1)
    m_len = torch.cat((seq_len, torch.full((B, 2 * nb), cur + 1, dtype=torch.int64, device=dev)), dim=1)
    keep = topk(m_sc, k=nb)[1]
    sequences = gather(m_seq, keep)
    beam_scores = torch.gather(m_sc, 1, keep)
    finished = torch.gather(m_fin, 1, keep)
    seq_len = torch.gather(m_len, 1, keep)
    cur += 1
    # early-stop heuristic (early_stopping=False): can the best running beam still beat the worst kept result?
    # (4.31 is_done: the best of all 2N candidates, an EOS one included)
    best_run = (top_lp[:, :1] if v431 else running_scores[:, :1]) / float(cur ** length_penalty)
    worst_fin = torch.where(finished, beam_scores.min(dim=1, keepdim=True)[0], torch.full_like(beam_scores, NEG))
    heuristic_open = heuristic_open & (best_run > worst_fin).any(dim=-1, keepdim=True)
    if v431 and cur >= max_len:
        # 4.31 finalize: the running beams (now L tokens) join the kept results at L ** length_penalty unless done
        fin2 = running_scores / float(cur ** length_penalty) + (~heuristic_open).float() * NEG
        m_sc = torch.cat((beam_scores, fin2), dim=1)
        keep = topk(m_sc, k=nb)[1]
        sequences = gather(torch.cat((sequences, running_seq), dim=1), keep)
        beam_scores = torch.gather(m_sc, 1, keep)
        finished = torch.gather(torch.cat((finished, torch.ones_like(finished)), dim=1), 1, keep)
        seq_len = torch.gather(torch.cat((seq_len, torch.full((B, nb), cur, dtype=torch.int64, device=dev)), dim=1), 1, keep)
    st.update(running_seq=running_seq, running_scores=running_scores, sequences=sequences, beam_scores=beam_scores, finished=finished,
              seq_len=seq_len, open=heuristic_open)
    flat = (beam_idx + torch.arange(B, device=dev)[:, None] * nb).reshape(-1)
    toks = running_seq[:, :, cur - 1].reshape(-1)
    return toks, flat, beam_idx, run_lp


# ---------------------------------------------------------------------------------------------------------------------------------
# Contrastive search (emu_amd/csrc/contrastive.hip: ``emu_contrastive_pick_bf16`` and ``emu_contrastive_score``): what the kernels
# compute per prompt and step.  It restates the arithmetic of the host loop ``LlamaEngine.contrastive_generate`` and is tested against it.
#
# Candidates, from the logit row the previous step kept: steps 1-3 above (repetition penalty once per distinct id of the prompt's
# history, EOS at -inf while ``step < min_len``), ``p = softmax(s)`` in ``dtype``, and the k largest in descending order of s (p is
# monotone in s), ties to the lower id.
#
# Selection: ``pen[b, j]`` = the largest cosine between candidate j's final-normed hidden row and the VALID context rows of prompt b
# (the prompt from its first real token, then every kept token: left padding is left out); ``score = (1 - alpha) * p - alpha * pen``;
# the first index of the maximum is kept.  Both depend on a candidate only through its row and its p, never through j: two identical
# candidates tie and the lower index wins.

def contrastive_reference_candidates(logits: torch.Tensor, history: History = None, repetition_penalty: float = 1.0,
                                     eos_id: Optional[int] = None, suppress_eos: bool = False, k: int = 1,
                                     dtype: torch.dtype = torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
    """(ids [B, k] int64, p [B, k] ``dtype``) of bf16 (or fp32-held) logit rows [B, vocab]."""
    s = reference_scores(logits, history, repetition_penalty, eos_id if suppress_eos else None)
    p = torch.softmax(s.to(dtype), dim=-1)
    ids = torch.sort(s, dim=-1, descending=True, stable=True)[1][:, :int(k)]         # stable: equal scores keep ascending id
    return ids, torch.gather(p, 1, ids)


def contrastive_reference_select(ctx: torch.Tensor, ctx_valid: torch.Tensor, cand_h: torch.Tensor, p: torch.Tensor, alpha: float,
                                 dtype: torch.dtype = torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
    """(pen [B, k] ``dtype``, sel [B] int64): ``ctx`` [B, L, H] hidden rows (any scale: they are normalised here), ``ctx_valid``
    [B, L] bool, ``cand_h`` [B, k, H], ``p`` [B, k]."""
    c, n = ctx.to(dtype), cand_h.to(dtype)
    cn = c / c.norm(dim=2, keepdim=True)
    nn_ = n / n.norm(dim=2, keepdim=True)
    cos = torch.einsum("bld,bkd->bkl", cn, nn_).masked_fill(~ctx_valid.to(torch.bool)[:, None, :], -float("inf"))
    pen = cos.max(dim=-1)[0]
    score = (1.0 - alpha) * p.to(dtype) - alpha * pen
    first = (score == score.max(dim=-1, keepdim=True)[0]).float().argmax(dim=-1)    # argmax of a 0/1 row: the first 1
    return pen, first


# ---------------------------------------------------------------------------------------------------------------------------------
# Constrained decoding (emu_amd/constrain.py: ``TokenTrie``; the "trie" variants of ``ops.SELECT_ENTRY``).  The kernels keep
# one trie node per row on the device and advance it by the id they select; what that state must equal is the stateless walk of the
# row's generated ids through the trie, and what the mask must equal is the trie's answer for those ids.

def constraint_allowed(trie, history: History) -> torch.Tensor:
    """[rows, vocab] bool: the ids that may follow each row's generated ids (``history`` [rows, n] or a list of rows)."""
    rows = _history_rows(history, len(history))
    mask = torch.zeros(len(rows), trie.vocab, dtype=torch.bool)
    for r, ids in enumerate(rows):
        mask[r, torch.tensor(trie.allowed(ids), dtype=torch.int64)] = True
    return mask


def trie_nodes(trie, history: History) -> torch.Tensor:
    """[rows] int32: the trie node of each row after its generated ids; -1 = off the trie or past its EOS."""
    return torch.tensor([trie.walk(ids) for ids in _history_rows(history, len(history))], dtype=torch.int32)
