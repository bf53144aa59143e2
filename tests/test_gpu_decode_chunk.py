"""GPU: the chunk step's attention launch (launch_decode_chunk, csrc/attention.hip, through emu_decode_chunk_bf16) on its own.

One launch = RoPE of the T queries and the T new keys of every sequence, append of the T new K / V rows at slots ``slot0 + i``,
attention of query i over the keys ``kstart <= key <= slot0 + i`` in 128-key splits, merge of the splits.  Checked

  (a) bit for bit (integer views) against T successive one-row launches (emu_decode_fused_bf16, ``slot = slot0 + i``): o and both
      caches -- the chunk form promises the one-row path's arithmetic and summation order;
  (b) against a float64 reference written from the operation's definition, with the bound of tests/test_gpu_decode_fused_kernel.py,
      |got - ref| <= 2^-7 |ref| + 1e-3 max|V|, on the same input distribution (randn rounded to bf16).  The bound is justified
      there by a plain fp32 restatement of split attention; the same restatement (that file's ``_restate_fp32``) is run on every
      row of every case here and asserted below 1/4 of the bound, scores within +-8;
  (c) NaN bit patterns in every dead cache slot (below kstart, at and above slot0: the chunk's own slots are written before they
      could be read) and in the whole workspace change no bit;
  (d) every cache element outside the T appended rows keeps its bits, the appended rows are the oracle-rotated keys and the values;
  (e) a repeated launch gives the same bits;
  (f) the refusals answer -22.

Helpers are imported from tests/test_gpu_decode_fused_kernel.py.  The operation is the attention of transformers' LlamaAttention
with a KV cache fed T tokens at once (assisted decoding's verify forward; Emu2/emu/emu.py:175,228 forwards the option)."""
import functools
from types import SimpleNamespace
from typing import NamedTuple, Optional, Tuple

import pytest
import torch

from tests import test_gpu_decode_fused_kernel as F

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
TS = [2, 3, 5, 8]


class Chunk(NamedTuple):
    D: int
    T: int
    S_max: int
    ctx_max: int
    slot0: Tuple[int, ...]                     # per sequence
    kstart: Optional[Tuple[int, ...]]          # per sequence, or None: the launch gets a null pointer
    H: int = 2
    seed: int = 0


def _ks_pos(c: Chunk):
    ks = c.kstart if c.kstart is not None else (0,) * len(c.slot0)
    return ks, tuple(s - k for s, k in zip(c.slot0, ks))


@functools.lru_cache(maxsize=4)
def _data(c: Chunk):
    """Inputs (CPU), the float64 reference of every row and its bound; computed once per case, shared, never modified."""
    from oracle import emu2_ref as R
    B, H, D, T = len(c.slot0), c.H, c.D, c.T
    ks, pos0 = _ks_pos(c)
    assert all(0 <= k <= s and s + T <= c.ctx_max <= c.S_max and p + T <= F.MAX_POS for k, s, p in zip(ks, c.slot0, pos0)), c
    g = torch.Generator().manual_seed(5200 + c.seed)
    qkv = torch.randn(B * T, 3 * H * D, generator=g).to(BF16)
    kc = torch.randn(B, H, c.S_max, D, generator=g).to(BF16)
    vc = torch.randn(B, H, c.S_max, D, generator=g).to(BF16)
    q4 = qkv.view(B, T, 3, H, D)
    pos = torch.tensor(pos0, dtype=torch.long)[:, None] + torch.arange(T)[None]                     # [B, T]
    cos, sin = R.rope_cos_sin(pos, D, 10000.0, BF16)                                                # [B, T, D]
    qr, kr = R.apply_rope(q4[:, :, 0].transpose(1, 2), q4[:, :, 1].transpose(1, 2), cos, sin)       # bf16 ops, [B, H, T, D]
    vn = q4[:, :, 2].transpose(1, 2).contiguous()                                                   # [B, H, T, D]
    scale = F._scale(D)
    ref = torch.empty(B, T, H, D, dtype=torch.float64)
    restated = torch.empty(B, T, H, D, dtype=torch.float32)
    smax = 0.0
    for b in range(B):
        lo, s0 = ks[b], c.slot0[b]
        for i in range(T):
            K = torch.cat([kc[b, :, lo:s0], kr[b, :, :i + 1]], dim=1).double()                      # [H, n, D]
            V = torch.cat([vc[b, :, lo:s0], vn[b, :, :i + 1]], dim=1).double()
            s = torch.einsum("hkd,hd->hk", K, qr[b, :, i].double()) * scale
            smax = max(smax, float(s.abs().max()))
            ref[b, i] = torch.einsum("hk,hkd->hd", torch.softmax(s, -1), V)
            Kf = torch.cat([kc[b, :, :s0], kr[b, :, :i + 1]], dim=1).float()
            Vf = torch.cat([vc[b, :, :s0], vn[b, :, :i + 1]], dim=1).float()
            restated[b, i] = F._restate_fp32(qr[b, :, i].float(), Kf, Vf, lo, s0 + i, scale)
    assert smax <= 8.0, smax                                               # the inputs' side of the tolerance
    vmax = max(float(vc.float().abs().max()), float(vn.float().abs().max()))
    bound = 2.0 ** -7 * ref.abs() + 1e-3 * vmax
    return SimpleNamespace(qkv=qkv, kc=kc, vc=vc, kr=kr, vn=vn, ref=ref.view(B * T, H, D), bound=bound.view(B * T, H, D), scale=scale,
                           smax=smax, restated=float(((restated.double() - ref).abs() / bound).max()))


def _caches(c: Chunk, fill: Optional[str]):
    """The case's caches with the dead slots (below kstart, from slot0 on) as they are (None), zeroed or holding NaN patterns."""
    d = _data(c)
    kc, vc = d.kc.clone(), d.vc.clone()
    if fill is not None:
        ks, _ = _ks_pos(c)
        s = torch.arange(c.S_max)[None, :]
        dead = ((s < torch.tensor(ks)[:, None]) | (s >= torch.tensor(c.slot0)[:, None]))[:, None, :, None].expand_as(kc)
        for t in (kc, vc):
            t[dead] = F._nan_like(t)[dead] if fill == "nan" else 0
    return kc, vc


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _launch(c: Chunk, kc, vc, ws_fill="zero"):
    """One chunk launch on copies of the given CPU caches -> (o [B*T, H, D], K cache after, V cache after), on the CPU."""
    ops, d = F._ops(), _data(c)
    B = len(c.slot0)
    ks, pos0 = _ks_pos(c)
    cos, sin = F._tables(c.D)
    n = F._lib().emu_decode_chunk_ws_bytes(B, c.T, c.H, c.D, c.ctx_max) // 4
    assert n == B * c.T * c.H * ((c.ctx_max + F.CHUNK - 1) // F.CHUNK) * (c.D + 2) + B * c.T
    ws = torch.zeros(n, dtype=torch.float32)
    if ws_fill == "nan":
        ws = F._nan_like(ws)
    qkv, dk, dv = d.qkv.cuda(), kc.cuda(), vc.cuda()
    o = ops.decode_chunk(qkv, cos, sin, _i32(pos0), _i32(c.slot0), dk, dv, c.H, c.T, c.ctx_max, d.scale,
                         kstart=None if c.kstart is None else _i32(ks), ws=ws.cuda())
    torch.cuda.synchronize()
    assert F.same_bits(qkv.cpu(), d.qkv), "the launch wrote to the projection rows"
    return o.cpu(), dk.cpu(), dv.cpu()


def _one_row_launches(c: Chunk, kc, vc):
    """T successive one-row launches, row i of every sequence at slot0 + i, on the same device caches."""
    ops, d = F._ops(), _data(c)
    B, T = len(c.slot0), c.T
    ks, pos0 = _ks_pos(c)
    cos, sin = F._tables(c.D)
    dk, dv = kc.cuda(), vc.cuda()
    rows = d.qkv.view(B, T, -1)
    o = torch.empty(B, T, c.H, c.D, dtype=BF16)
    for i in range(T):
        oi = ops.decode_fused(rows[:, i].contiguous().cuda(), cos, sin, _i32([p + i for p in pos0]), _i32([s + i for s in c.slot0]),
                              dk, dv, c.H, c.ctx_max, d.scale, kstart=None if c.kstart is None else _i32(ks))
        o[:, i] = oi.cpu()
    torch.cuda.synchronize()
    return o.view(B * T, c.H, c.D), dk.cpu(), dv.cpu()


def _check_o(c: Chunk, o, what=""):
    d = _data(c)
    print(f"{what} fp32 restatement / bound = {d.restated:.2e}, max |score| = {d.smax:.2f}")
    assert d.restated < 0.25, (d.restated, c)                              # the bound has room for fp32 split attention
    assert bool(torch.isfinite(o.float()).all()), what
    err = (o.double() - d.ref).abs() / d.bound                              # every element, none excluded
    print(f"{what} kernel / bound = {float(err.max()):.3f}")
    assert float(err.max()) <= 1.0, (what, float(err.max()), [int(i) for i in (err == err.max()).nonzero()[0]], c)


def _check_caches(c: Chunk, before, after, what=""):
    """Exactly T K rows and T V rows per (sequence, head) were written -- the oracle-rotated keys and the projection's values --
    and every other element of both caches holds the bits it held before."""
    d = _data(c)
    for name, b4, aft, new in (("K", before[0], after[0], d.kr), ("V", before[1], after[1], d.vn)):
        want = b4.clone()
        for b, s0 in enumerate(c.slot0):
            want[b, :, s0:s0 + c.T] = new[b]
        diff = F._bits(aft) != F._bits(want)
        assert not bool(diff.any()), f"{what}: {name} cache differs at {diff.nonzero()[:4].tolist()}"


def _full_check(c: Chunk, fill=None, ws_fill="zero", what=""):
    kc, vc = _caches(c, fill)
    o, k1, v1 = _launch(c, kc, vc, ws_fill)
    _check_caches(c, (kc, vc), (k1, v1), what)
    _check_o(c, o, what)
    return o, k1, v1


# ------------------------------------------------------------------------------------------------------------ cases
def _placements(D, T):
    s = D + T                                                              # a seed per (D, T)
    return [
        Chunk(D, T, 384, 384, (5,), None, seed=s),                          # inside one split
        Chunk(D, T, 384, 384, (126,), (3,), seed=s + 1),                    # straddling a split boundary (T = 2: ending on it)
        Chunk(D, T, 384, 384, (128,), None, seed=s + 2),                    # starting on one
        Chunk(D, T, 384, 384, (200,), (200,), seed=s + 3),                  # slot0 == kstart: row 0 returns its own v
        Chunk(D, T, 384, 384, (300,), (260,), seed=s + 4),                  # kstart inside the last split: two dead splits
        Chunk(D, T, 384, 300, (126, 290), (0, 131), seed=s + 5),            # two sequences, their own slot0 and kstart
    ]


CASES = [c for D in F.DS for T in TS for c in _placements(D, T)]
LONG = [Chunk(D, 8, 2304, 2304, (2304 - 8,), (130,), seed=77) for D in F.DS]    # 18 splits: the merge's loop form


def _id(c):
    return (f"D{c.D}-T{c.T}-slot{'_'.join(map(str, c.slot0))}-ctx{c.ctx_max}of{c.S_max}" +
            ("" if c.kstart is None else f"-ks{'_'.join(map(str, c.kstart))}"))


# ------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("c", CASES + LONG, ids=_id)
def test_chunk_equals_successive_one_row_launches_and_the_reference(c):
    """(a), (b), (d), (e): bits of T one-row launches, the float64 reference within the bound, the caches, a second launch."""
    o, k1, v1 = _full_check(c, what=_id(c))
    kc, vc = _caches(c, None)
    o_seq, k_seq, v_seq = _one_row_launches(c, kc, vc)
    assert F.same_bits(o, o_seq), (_id(c), (F._bits(o) != F._bits(o_seq)).nonzero()[:4].tolist())
    assert F.same_bits(k1, k_seq) and F.same_bits(v1, v_seq), _id(c)
    o2, k2, v2 = _launch(c, kc, vc)
    assert F.same_bits(o, o2) and F.same_bits(k1, k2) and F.same_bits(v1, v2)
    for b, (s0, ks) in enumerate(zip(c.slot0, c.kstart or (None,) * len(c.slot0))):
        if ks == s0:                                                       # a softmax over one key is 1: the new v itself
            assert F.same_bits(o[b * c.T], _data(c).vn[b, :, 0]), _id(c)


@pytest.mark.parametrize("c", CASES[1::2] + LONG, ids=_id)
def test_dead_cache_slots_and_workspace_are_never_consumed(c):
    """(c): NaN patterns below kstart, from slot0 on (the chunk's slots and everything above) and in the whole workspace: finite,
    within the bound, bit-equal to the launch with zeros there; the poison outside the appended rows is still in place."""
    o_nan, _, _ = _full_check(c, "nan", "nan", what=_id(c) + " poisoned")
    o_zero, _, _ = _full_check(c, "zero", "zero", what=_id(c) + " zeroed")
    assert F.same_bits(o_nan, o_zero)


def test_refusals():
    """(f): T outside 2..8, D not in {64, 128}, ctx_max outside [1, S_max] answer -22 and launch nothing (o keeps its bits)."""
    lib, ops = F._lib(), F._ops()
    from emu_amd._lib import EmuHipError

    def call(T, D, S_max, ctx_max):
        H = 2
        z = lambda *s: torch.zeros(*s, dtype=BF16, device="cuda")
        kc, vc, qkv, tab = z(1, H, S_max, D), z(1, H, S_max, D), z(max(T, 1), 3 * H * D), z(16, D)
        ws = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
        o = torch.full((max(T, 1), H, D), 3.0, dtype=BF16, device="cuda")
        st = lib.emu_decode_chunk_bf16(qkv.data_ptr(), tab.data_ptr(), tab.data_ptr(), _i32([0]).data_ptr(), _i32([0]).data_ptr(),
                                       kc.data_ptr(), vc.data_ptr(), o.data_ptr(), o.stride(0), o.stride(1), None, ws.data_ptr(), 1, T,
                                       H, D, S_max, ctx_max, 0.125, ops.stream(qkv))
        torch.cuda.synchronize()
        assert bool((o == 3.0).all())
        return st

    for T, D, S_max, ctx_max in ((1, 64, 16, 16), (9, 64, 16, 16), (0, 128, 16, 16), (2, 32, 16, 16), (2, 256, 16, 16),
                                 (2, 64, 16, 0), (2, 64, 16, 17), (8, 128, 16, -1)):
        assert call(T, D, S_max, ctx_max) == -22, (T, D, S_max, ctx_max)
    with pytest.raises(EmuHipError):
        z = torch.zeros(1, 2, 16, 64, dtype=BF16, device="cuda")
        ops.decode_chunk(torch.zeros(9, 3 * 2 * 64, dtype=BF16, device="cuda"), *F._tables(64), _i32([0]), _i32([0]), z, z.clone(), 2, 9,
                         16, 0.125)
