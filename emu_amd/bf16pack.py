"""The 13-bit lossless packing of bf16 weights that the one-row decode streams read (csrc/gemv_pack.hip), and the 12-bit one behind it
(``pack12``, stated where its functions begin), restated with torch on the CPU.  csrc/bf16_pack.h states the same layout for the device packer and the kernels; the GPU tests hold the two against each other
byte for byte.

A bf16 weight spends 8 of its 16 bits on an exponent and a weight matrix uses only a handful of binades, so the top 7 bits of the
exponent field are stored as a 4-bit offset from a per-matrix base ``hb``.  A weight ``w`` (16 bits: s, e8, m7) becomes

* the low byte ``w & 0xff`` (e8's lowest bit and the mantissa), verbatim,
* the nibble ``((w >> 8) & 0x7f) - hb``, which must lie in 0..15,
* the sign bit,

13 bits instead of 16.  ``hb`` follows from the largest exponent field ``emax`` of the matrix's finite weights (``hb_rule``): the window
is the 32 binades ``[2 hb, 2 hb + 31]`` whose top pair holds ``emax``.  A weight outside the window -- a zero or a tiny value beside
large ones, Inf, NaN -- flags its row group (``flag_rule``); a flagged group is read from the bf16 matrix, so the planes carry no
patches.

Layout, for row groups of ``R`` (2 or 4: the rows one workgroup of the planned bf16 kernel owns) consecutive rows, the last group padded
with zero weights, ``KV = K / 8`` 16-byte vectors per row, ``G = ceil(N / R)``:

* ``lo``    uint8 [G, R/2, KV, 16]: unit (g, h, vi) = the 8 low bytes of vector vi of row 2h of the group, then those of row 2h + 1
* ``nib``   uint8 [G, KV, R, 4]: byte b of row r = nibble of weight b | nibble of weight b + 4 << 4
* ``sign``  uint8 [G, KV, R].  R = 2: byte r, bit j = sign of weight j of row r's vector vi.  R = 4: the bytes are one little-endian
  32-bit word whose bit ``8 b + 7 - q`` holds the sign of weight ``4 hf + b`` of row ``r``, ``q = 2 r + hf`` (the four signs that belong
  to one dword of high bytes sit one byte apart: one shift and one mask on the device)
* ``flags`` int32 [ceil(G / 32)]: bit g % 32 of word g / 32 = row group g is flagged
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch


def _bits(w: torch.Tensor) -> torch.Tensor:
    assert w.dtype == torch.bfloat16 and w.dim() == 2, (w.dtype, w.shape)
    return w.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def hb_rule(emax: int) -> int:
    """The exponent base of a matrix whose largest finite exponent field is ``emax``: top binade pair ``emax | 1``, 32 binades down."""
    top = int(emax) | 1
    return max(0, (top - 31) >> 1)


def matrix_hb(w: torch.Tensor) -> int:
    b = _bits(w)
    e8 = (b >> 7) & 0xFF
    finite = e8[e8 != 0xFF]
    return hb_rule(int(finite.max()) if finite.numel() else 0)


def flag_rule(w: torch.Tensor, hb: int) -> torch.Tensor:
    """bool [N, K]: the weights that cannot be stored (nibble outside 0..15, or an Inf / NaN)."""
    b = _bits(w)
    d = ((b >> 8) & 0x7F) - hb
    return (d < 0) | (d > 15) | (((b >> 7) & 0xFF) == 0xFF)


def packed_bytes(N: int, K: int, rows: int) -> int:
    """Bytes of the set of an [N, K] matrix: the three planes (13 bits per weight of the padded groups) and the flag words."""
    G = (N + rows - 1) // rows
    return G * rows * K * 13 // 8 + 4 * ((G + 31) // 32)


def pack(w: torch.Tensor, rows: int) -> Dict[str, object]:
    """bf16 [N, K] (K % 32 == 0) -> {"lo", "nib", "sign", "flags", "hb", "rows", "shape"} (see the module docstring)."""
    assert rows in (2, 4)
    N, K = w.shape
    assert K >= 32 and K % 32 == 0, K
    hb = matrix_hb(w)
    G, KV = (N + rows - 1) // rows, K // 8
    bad = flag_rule(w, hb)
    b = torch.zeros(G * rows, K, dtype=torch.int32)
    b[:N] = _bits(w)
    badg = torch.zeros(G * rows, dtype=torch.bool)
    badg[:N] = bad.any(dim=1)
    v = b.view(G, rows, KV, 8)                                       # [g, r, vi, j]
    lo = (v & 0xFF).view(G, rows // 2, 2, KV, 8).permute(0, 1, 3, 2, 4).reshape(G, rows // 2, KV, 16)
    d = (((v >> 8) & 0x7F) - hb) & 15
    nib = (d[..., :4] | (d[..., 4:] << 4)).permute(0, 2, 1, 3)       # [g, vi, r, b]
    if rows == 2:
        sign = ((v >> 15) << torch.arange(8, dtype=torch.int32)).sum(dim=-1).permute(0, 2, 1)
    else:                                                            # [g, r, vi, hf, b] -> [g, vi, b, q = 2 r + hf], bit 7 - q of byte b
        sq = (v >> 15).view(G, 4, KV, 2, 4).permute(0, 2, 4, 1, 3).reshape(G, KV, 4, 8)
        sign = (sq << (7 - torch.arange(8, dtype=torch.int32))).sum(dim=-1)
    fg = badg.view(G, rows).any(dim=1)
    words = torch.zeros(((G + 31) // 32) * 32, dtype=torch.int64)
    words[:G] = fg.to(torch.int64)
    flags = (words.view(-1, 32) << torch.arange(32, dtype=torch.int64)).sum(dim=1)
    flags = torch.where(flags >= 2 ** 31, flags - 2 ** 32, flags).to(torch.int32)
    return {"lo": lo.to(torch.uint8).contiguous(), "nib": nib.to(torch.uint8).contiguous(), "sign": sign.to(torch.uint8).contiguous(),
            "flags": flags, "hb": hb, "rows": rows, "shape": (N, K)}


def flagged_groups(p: Dict[str, object]) -> torch.Tensor:
    """bool [G]: the flagged row groups of a packed set."""
    N, _ = p["shape"]
    G = (N + p["rows"] - 1) // p["rows"]
    f = p["flags"].to(torch.int64) & 0xFFFFFFFF
    return (((f[:, None] >> torch.arange(32, dtype=torch.int64)) & 1).reshape(-1)[:G]).bool()


def unpack(p: Dict[str, object]) -> Tuple[torch.Tensor, torch.Tensor]:
    """(bf16 [N, K] decoded from the planes, bool [N]: the rows of flagged groups, whose decoded values are not to be used)."""
    N, K = p["shape"]
    R, hb = p["rows"], p["hb"]
    G, KV = (N + R - 1) // R, K // 8
    lo = p["lo"].to(torch.int32).view(G, R // 2, KV, 2, 8).permute(0, 1, 3, 2, 4).reshape(G, R, KV, 8)
    nb = p["nib"].to(torch.int32).permute(0, 2, 1, 3)                # [g, r, vi, b]
    d = torch.cat([nb & 15, nb >> 4], dim=-1)
    if R == 2:
        sg = (p["sign"].to(torch.int32).permute(0, 2, 1)[..., None] >> torch.arange(8, dtype=torch.int32)) & 1
    else:                                                            # [g, vi, b, q] -> [g, r, vi, hf, b] -> [g, r, vi, j = 4 hf + b]
        sq = (p["sign"].to(torch.int32)[..., None] >> (7 - torch.arange(8, dtype=torch.int32))) & 1
        sg = sq.view(G, KV, 4, 4, 2).permute(0, 3, 1, 4, 2).reshape(G, 4, KV, 8)
    bits = (sg << 15) | ((d + hb) << 8) | lo
    bits = bits.reshape(G * R, K)[:N]
    w = torch.where(bits >= 2 ** 15, bits - 2 ** 16, bits).to(torch.int16).view(torch.bfloat16)
    return w, flagged_groups(p).repeat_interleave(R)[:N]


# ---------------------------------------------------------------------------------------------------- the 12-bit format
# The sign moves into the nibble beside a 3-bit exponent code, so the sign plane goes: ``n(w) = sign << 3 | code`` with
# ``code = ((w >> 8) & 0x7f) - hb`` in 0..7, laid out as the 13-bit nibbles are.  ``hb`` is the base of the window of 8 codes that
# covers the most weights (``window_rule``).  A weight outside the window -- any bit pattern: zeros, denormals, Inf and NaN are not
# special -- is a miss: its low byte stays in ``lo``, its nibble is 0 and one slot of its row group's patch record carries its high byte:
#
# * ``patch`` int32 [G, 8]: slot = ``vi << 13 | r << 11 | j << 8 | (w >> 8)`` (vector index, row in the group, element 0..7, high byte);
#   the slots in use sorted ascending as unsigned words, the empty ones (0xffffffff, i.e. -1) behind them
# * a row group with more than 8 misses is flagged (it is read from the bf16 matrix, as in the 13-bit format) and its record is empty
# * rows that pad the last group are no misses (nibble 0, low byte 0)
PACK12_SLOTS = 8
# the kinds of matrix whose 12-bit twin beat the 13-bit one on the device (profiles/bf16_pack12.md): only these take a 12-bit set
PACK12_KINDS = ("wqkv", "wo", "wgu", "wdown", "lm_head")


def window_rule(hist) -> int:
    """The base ``hb`` (0..120) of the 8-code window [hb, hb + 7] that covers the most weights, from the 128 counts of
    ``(w >> 8) & 0x7f``; ties go to the lower base (an empty histogram: 0).  A pure function of the counts."""
    h = [int(c) for c in hist]
    assert len(h) == 128
    best, hb = -1, 0
    for b in range(121):
        c = sum(h[b:b + 8])
        if c > best:
            best, hb = c, b
    return hb


def histogram12(w: torch.Tensor) -> torch.Tensor:
    """int64 [128]: the counts of ``(w >> 8) & 0x7f`` over the matrix."""
    return torch.bincount(((_bits(w) >> 8) & 0x7F).reshape(-1).to(torch.int64), minlength=128)


def miss_rule12(w: torch.Tensor, hb: int) -> torch.Tensor:
    """bool [N, K]: the weights whose code is outside 0..7."""
    d = ((_bits(w) >> 8) & 0x7F) - hb
    return (d < 0) | (d > 7)


def packed_bytes12(N: int, K: int, rows: int) -> int:
    """Bytes of the 12-bit set of an [N, K] matrix: the two planes (12 bits per weight of the padded groups), the patch records (32
    bytes per row group) and the flag words."""
    G = (N + rows - 1) // rows
    return G * rows * K * 12 // 8 + 4 * PACK12_SLOTS * G + 4 * ((G + 31) // 32)


def set_bits(flagged_12: int, groups: int, rows: int, K: int, enabled_12: bool = True) -> int:
    """Which format a matrix's set takes -> 12 | 13, from what its 12-bit pack reported: ``flagged_12`` of its ``groups`` row groups of
    ``rows`` rows by ``K`` weights are flagged.  12 bits while the 12-bit stream is the smaller one: a group streams ``12 rows K`` bits
    of planes and a 256-bit patch record, a flagged group ``16 rows K`` bits of bf16 rows on top, against ``13 rows K`` bits per group
    of the 13-bit set.  Break-even: ``flagged_12 / groups = (1 - 256 / (rows K)) / 16``, just under one group in 16; at or above it, 13
    bits.  ``enabled_12`` False (EMU_BF16_PACK12=0, a tensor-parallel shard, a kind of matrix whose 12-bit twin is not faster): 13."""
    if not enabled_12 or groups < 1:
        return 13
    w = rows * K
    return 12 if (12 * w + 256) * groups + 16 * w * flagged_12 < 13 * w * groups else 13


def pack12(w: torch.Tensor, rows: int) -> Dict[str, object]:
    """bf16 [N, K] (K % 32 == 0) -> {"lo", "nib", "patch", "flags", "hb", "rows", "shape", "bits": 12, "flagged"} (see above)."""
    assert rows in (2, 4)
    N, K = w.shape
    assert K >= 32 and K % 32 == 0 and K // 8 < 2 ** 18, K
    hb = window_rule(histogram12(w))
    G, KV = (N + rows - 1) // rows, K // 8
    b = torch.zeros(G * rows, K, dtype=torch.int32)
    b[:N] = _bits(w)
    miss = torch.zeros(G * rows, K, dtype=torch.bool)
    miss[:N] = miss_rule12(w, hb)
    v = b.view(G, rows, KV, 8)                                       # [g, r, vi, j]
    mv = miss.view(G, rows, KV, 8)
    lo = (v & 0xFF).view(G, rows // 2, 2, KV, 8).permute(0, 1, 3, 2, 4).reshape(G, rows // 2, KV, 16)
    n = ((v >> 15) << 3) | (((v >> 8) & 0x7F) - hb)
    n = torch.where(mv, torch.zeros_like(n), n)
    n.view(G * rows, K)[N:] = 0                                      # padding rows
    nib = (n[..., :4] | (n[..., 4:] << 4)).permute(0, 2, 1, 3)       # [g, vi, r, b]
    g, r, vi, j = mv.nonzero(as_tuple=True)
    slot = (vi << 13) | (r << 11) | (j << 8) | (v[g, r, vi, j].to(torch.int64) >> 8)
    order = torch.argsort(g * 2 ** 32 + slot)
    g, slot = g[order], slot[order]
    count = torch.bincount(g, minlength=G)
    fg = count > PACK12_SLOTS
    start = torch.cumsum(count, 0) - count
    keep = ~fg[g]
    patch = torch.full((G, PACK12_SLOTS), 0xFFFFFFFF, dtype=torch.int64)
    patch[g[keep], (torch.arange(g.numel()) - start[g])[keep]] = slot[keep]
    patch = torch.where(patch >= 2 ** 31, patch - 2 ** 32, patch).to(torch.int32)
    words = torch.zeros(((G + 31) // 32) * 32, dtype=torch.int64)
    words[:G] = fg.to(torch.int64)
    flags = (words.view(-1, 32) << torch.arange(32, dtype=torch.int64)).sum(dim=1)
    flags = torch.where(flags >= 2 ** 31, flags - 2 ** 32, flags).to(torch.int32)
    return {"lo": lo.to(torch.uint8).contiguous(), "nib": nib.to(torch.uint8).contiguous(), "patch": patch.contiguous(), "flags": flags,
            "hb": hb, "rows": rows, "shape": (N, K), "bits": 12, "flagged": int(fg.sum())}


def slots_used(p: Dict[str, object]) -> torch.Tensor:
    """int64 [G]: the patch slots in use per row group of a 12-bit set (0 for a flagged group: its record is empty)."""
    return (p["patch"] != -1).sum(dim=1)


def unpack12(p: Dict[str, object]) -> Tuple[torch.Tensor, torch.Tensor]:
    """(bf16 [N, K] decoded from the planes and the patch records, bool [N]: the rows of flagged groups, whose decoded values are not
    to be used)."""
    N, K = p["shape"]
    R, hb = p["rows"], p["hb"]
    G, KV = (N + R - 1) // R, K // 8
    lo = p["lo"].to(torch.int32).view(G, R // 2, KV, 2, 8).permute(0, 1, 3, 2, 4).reshape(G, R, KV, 8)
    nb = p["nib"].to(torch.int32).permute(0, 2, 1, 3)                # [g, r, vi, b]
    n = torch.cat([nb & 15, nb >> 4], dim=-1)
    high = ((n >> 3) << 7) | ((n & 7) + hb)
    pt = p["patch"].to(torch.int64) & 0xFFFFFFFF
    g, s = (pt != 0xFFFFFFFF).nonzero(as_tuple=True)
    sl = pt[g, s]
    high[g, (sl >> 11) & 3, sl >> 13, (sl >> 8) & 7] = (sl & 0xFF).to(torch.int32)
    bits = ((high << 8) | lo).reshape(G * R, K)[:N]
    w = torch.where(bits >= 2 ** 15, bits - 2 ** 16, bits).to(torch.int16).view(torch.bfloat16)
    return w, flagged_groups(p).repeat_interleave(R)[:N]


def default_pack(env, world_size: int, bf16_released: bool, need: int, free: int) -> str:
    """Which matrices of a loaded model get a packed set by default -> "off" | "plain" | "all".  "plain": o_proj and down (the two-row
    streams, what ``LlamaEngine`` packs by itself at load); "all": qkv, gate/up and lm_head too (the head form, 8 rows per workgroup:
    profiles/bf16_pack_head8.md).  A pure function of scalars, so a CPU test can enumerate it (tests/test_pack_default_rule.py).

    ``env``: the value of EMU_BF16_PACK or None ("0" = off, "plain", "all" or unset = all; anything else is read as unset);
    ``world_size``: tensor-parallel ranks -- more than one stays plain: a shard's qkv and gate/up do take the head form, but nothing at
    TP has been timed on hardware; ``bf16_released``: flagged row groups read the bf16 matrices, so nothing is packed without them;
    ``need`` / ``free``: bytes of the head-form sets still missing and free device bytes -- sets that would take more than half of what
    is free are not added (the KV cache and the workspaces need the rest), which leaves what the engine's own rule, the same one over
    the plain sets, decided at load."""
    if env == "0" or bf16_released:
        return "off"
    if env == "plain" or world_size > 1:
        return "plain"
    if 2 * int(need) > int(free):
        return "plain"
    return "all"
