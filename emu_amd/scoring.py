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
"""
from __future__ import annotations

from typing import Dict, Optional

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
