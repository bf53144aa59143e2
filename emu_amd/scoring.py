"""Specification of the scoring kernel (emu_amd/csrc/score.hip, ``emu_token_logprob_bf16``) in pure torch: what it computes for one
row of bf16 logits ``x[0..V)``, a forced target id ``t`` and optionally a reference row ``r[0..V)`` of bf16 logits.  It plays the role
``emu_amd/sampling.py`` plays for the sampler: the kernel is tested against this file, and this file against
``torch.log_softmax`` and ``torch.nn.CrossEntropyLoss``.

* ``m = max x``; ``lse = m + log(sum exp(x - m))``: the subtraction and the exponential are fp32, the sum is taken in ``dtype``.
* ``lp = float32(x[t]) - lse``.  A target outside [0, V) is IGNORED (the reference's ignore value is -100): ``lp = 0`` and
  ``counted = False``.  ``x[t] = -inf`` gives ``lp = -inf``, not NaN.
* ``top1`` is the first index of the maximum (``argmax_kernel``'s tie rule).
* ``kl = sum_j p_r[j] * (logp_r[j] - logp_x[j])`` with ``logp = x - lse`` (fp32) of both rows as above and ``p_r = exp(logp_r)``;
  terms with ``p_r[j] == 0`` contribute 0; ``logp_x[j] = -inf`` where ``p_r[j] > 0`` gives ``kl = +inf``.  The sum is taken in ``dtype``.
* ``agree = (top1(x) == top1(r))``.

``dtype=torch.float64`` widens only the sums (and the logarithm of them): the tests' yardstick for the kernel's fp32 sums, whose
order -- per thread sequential in ascending id order, then a fixed tree -- is the kernel's own.

``reference_candidate_losses`` restates the loss the reference ranks candidate answers by (Emu1/models/prediction_mixin.py:36-131 on
the loss of Emu1/models/modeling_llama.py:110-116).

``two_segment_attention`` is the specification of the two-segment flash kernel (emu_amd/csrc/attention_prefix.hip) and
``shared_prefix_plan`` the host arithmetic of ``LlamaEngine.score_continuations(share_prefix=True)``: the caches it allocates and
what they and the unshared route's cost in bytes.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Sequence

import torch

IGNORE_INDEX = -100        # the reference's label for a position that does not count (prediction_mixin.py:66-70)


def _first_argmax(s: torch.Tensor) -> torch.Tensor:
    return (s == s.max(dim=-1, keepdim=True)[0]).float().argmax(dim=-1)       # argmax of a 0/1 row: the first 1


def _lse(s: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """s [..., V] fp32 -> lse [..., 1] in ``dtype``."""
    m = s.max(dim=-1, keepdim=True)[0]
    z = torch.exp(s - m).to(dtype).sum(dim=-1, keepdim=True)
    return m.to(dtype) + torch.log(z)


def reference_logprob(logits: torch.Tensor, targets: torch.Tensor, ref_logits: Optional[torch.Tensor] = None,
                      dtype: torch.dtype = torch.float32) -> Dict[str, torch.Tensor]:
    """``logits`` [..., V] bf16 (or fp32-held bf16), ``targets`` [...] integer -> dict of ``lp`` and ``lse`` (``dtype``), ``counted``
    (bool), ``top1`` (int64), and with ``ref_logits`` [..., V]: ``kl`` (``dtype``), ``agree`` (bool)."""
    s = logits.float()
    V = s.shape[-1]
    t = targets.to(device=s.device, dtype=torch.int64)
    lse = _lse(s, dtype)
    counted = (t >= 0) & (t < V)
    xt = s.gather(-1, t.clamp(0, V - 1).unsqueeze(-1)).squeeze(-1)
    lp = xt.to(dtype) - lse.squeeze(-1)
    lp = torch.where(counted, lp, torch.zeros_like(lp))
    out = {"lp": lp, "lse": lse.squeeze(-1), "counted": counted, "top1": _first_argmax(s)}
    if ref_logits is not None:
        r = ref_logits.float()
        lser = _lse(r, dtype)
        # the kernel's log-probabilities are fp32 differences from its fp32 lse; in fp64 they are differences from the fp64 lse
        logp_x = s.to(dtype) - lse
        logp_r = r.to(dtype) - lser
        p_r = torch.exp(logp_r)
        term = torch.where(p_r == 0, torch.zeros_like(p_r), p_r * (logp_r - logp_x))
        out["kl"] = term.sum(dim=-1)
        out["agree"] = out["top1"] == _first_argmax(r)
    return out


def reference_candidate_losses(lp: torch.Tensor, counted: torch.Tensor, S: int, Tmax: int) -> torch.Tensor:
    """The reference's per-candidate loss from the candidates' per-token log-probabilities ``lp`` [N, T] and ``counted`` [N, T].

    The reference concatenates prompt (S tokens, labels ignored) and candidate (padded to the longest of its SEGMENT, ``Tmax``; padding
    ignored), shifts logits and labels by one, takes ``CrossEntropyLoss(reduction="none")`` over all S + Tmax - 1 shifted positions
    and then ``.view(B, -1).mean(1)`` (prediction_mixin.py:112-115): an ignored position is a zero in that mean, so
    ``loss_c = -(sum of the candidate's counted lp) / (S + Tmax - 1)`` -- a denominator that differs between segments with
    different longest candidates.  That quirk is kept."""
    lp = torch.where(counted, lp, torch.zeros_like(lp))
    return -lp.sum(dim=-1) / float(S + Tmax - 1)


def split_segments(n_cands: int, n_segments: int):
    """The (start, end) candidate ranges of prediction_mixin.py:84-90: ``n_cands // n_segments`` per segment, the last one takes the
    remainder."""
    if n_segments < 1 or n_segments > max(n_cands, 1):
        raise ValueError(f"n_segments must be in [1, {n_cands}], got {n_segments}")
    per = n_cands // n_segments
    return [(i * per, n_cands if i == n_segments - 1 else (i + 1) * per) for i in range(n_segments)]


def two_segment_attention(q: torch.Tensor, kp: torch.Tensor, vp: torch.Tensor, ko: torch.Tensor, vo: torch.Tensor, kstart: int,
                          scale: float) -> torch.Tensor:
    """Attention of B rows behind ONE shared prefix, in the dtype it is given: ``q`` [B, Sq, H, D]; the prefix ``kp`` / ``vp``
    [P, H, D], common to all rows, of which keys [kstart, P) count (left padding); the rows' own ``ko`` / ``vo`` [B, Sk, H, D], of
    which query i sees keys j <= i + (Sk - Sq).  Each segment is reduced on its own -- maximum, sum of exponentials, weighted values --
    and the two states are merged as an online softmax merges tiles.  This is the specification of the kernel's MASKING, not of its
    rounding (the kernel keeps fp32 sums and rounds the probabilities to bf16)."""
    B, Sq, H, D = q.shape
    P, Sk = kp.shape[0], ko.shape[1]
    if not 0 <= kstart < P or Sk < Sq:
        raise ValueError(f"two_segment_attention: 0 <= kstart < P and Sk >= Sq, got kstart = {kstart}, P = {P}, Sq = {Sq}, Sk = {Sk}")
    neg = float("-inf")
    sp = torch.einsum("bqhd,phd->bhqp", q, kp) * scale                                  # [B, H, Sq, P]
    sp = sp.masked_fill(torch.arange(P, device=q.device)[None, None, None, :] < kstart, neg)
    so = torch.einsum("bqhd,bkhd->bhqk", q, ko) * scale                                 # [B, H, Sq, Sk]
    i = torch.arange(Sq, device=q.device)[:, None]
    j = torch.arange(Sk, device=q.device)[None, :]
    so = so.masked_fill((j > i + (Sk - Sq))[None, None], neg)
    mp, mo = sp.amax(dim=-1, keepdim=True), so.amax(dim=-1, keepdim=True)               # kstart < P, own key 0 visible: both finite
    ep, eo = torch.exp(sp - mp), torch.exp(so - mo)
    op = torch.einsum("bhqp,phd->bhqd", ep, vp)
    oo = torch.einsum("bhqk,bkhd->bhqd", eo, vo)
    m = torch.maximum(mp, mo)
    wp, wo = torch.exp(mp - m), torch.exp(mo - m)
    num = op * wp + oo * wo
    den = ep.sum(dim=-1, keepdim=True) * wp + eo.sum(dim=-1, keepdim=True) * wo
    return (num / den).permute(0, 2, 1, 3).contiguous()                                 # [B, Sq, H, D]


SUFFIX_MIN_SLOTS = 16      # smallest suffix cache of the shared-prefix route: candidates of up to 16 tokens share one allocation


def suffix_capacity(width: int) -> int:
    """Slots of a segment's suffix cache: the next power of two >= max(16, width), so segments of similar width reuse one allocation."""
    cap = SUFFIX_MIN_SLOTS
    while cap < width:
        cap *= 2
    return cap


def shared_prefix_plan(N: int, S: int, widths: Sequence[int], layers: int, heads_local: int, head_dim: int,
                       kv_capacity: Callable[[int], int]) -> Dict:
    """What ``score_continuations`` allocates for N candidates behind an S-slot prompt, scored in ``len(widths)`` segments
    (``split_segments``) of the given widths (the longest candidate of each): pure host arithmetic.  ``kv_capacity``: the engine's
    bucket rule (``LlamaEngine.kv_capacity``).  Both routes prefill the prompt into a cache of 1 x ``prefix_capacity`` slots
    (``prefix_shape`` / ``prefix_bytes``, K and V together).  Per segment of ``rows`` candidates:

    * shared route: a suffix cache of rows x ``suffix_capacity`` slots (``suffix_shape``, ``shared_bytes``) and no copy;
    * unshared route: ``fan_out_kv``'s cache of rows x ``prefix_capacity`` slots (``unshared_shape``, ``unshared_bytes``) into which
      rows x S slots of the prompt are copied (``copy_bytes``).

    One cache of each kind is alive at a time: the routes' peaks are ``prefix_bytes`` plus the largest segment's bytes
    (``shared_peak_bytes`` / ``unshared_peak_bytes``)."""
    if N < 1 or S < 1 or not widths or min(widths) < 1:
        raise ValueError(f"shared_prefix_plan: N, S and every width >= 1, got N = {N}, S = {S}, widths = {list(widths)}")
    slot_bytes = 2 * layers * heads_local * head_dim * 2                 # K and V of one slot of one row, bf16
    s_max = kv_capacity(S + max(widths))
    segs = []
    for (a, b), w in zip(split_segments(N, len(widths)), widths):
        rows, cap = b - a, suffix_capacity(w)
        segs.append({"rows": rows, "width": w, "suffix_capacity": cap,
                     "suffix_shape": (layers, rows, heads_local, cap, head_dim), "shared_bytes": rows * cap * slot_bytes,
                     "unshared_shape": (layers, rows, heads_local, s_max, head_dim), "unshared_bytes": rows * s_max * slot_bytes,
                     "copy_bytes": rows * S * slot_bytes})
    prefix_bytes = s_max * slot_bytes
    return {"slot_bytes": slot_bytes, "prefix_capacity": s_max, "prefix_shape": (layers, 1, heads_local, s_max, head_dim),
            "prefix_bytes": prefix_bytes, "segments": segs,
            "shared_peak_bytes": prefix_bytes + max(g["shared_bytes"] for g in segs),
            "unshared_peak_bytes": prefix_bytes + max(g["unshared_bytes"] for g in segs)}
