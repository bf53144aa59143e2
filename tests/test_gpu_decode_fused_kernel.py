"""GPU: the decode step's attention launch (launch_decode_fused, csrc/attention.hip, through emu_decode_fused_bf16) on its own
against a float64 reference written from the operation's definition.

One launch = RoPE of q and of the new key, append of the new key / value at ``slot``, attention of the rotated q over the keys
``kstart <= key <= slot`` in 128-key splits, merge of the splits.  The reference knows nothing of splits: q and the new key are
rotated with the oracle's bf16 ops (oracle.emu2_ref.apply_rope, the rounding points test_rope_kv_append pins), then
softmax(q K^T scale) V in float64 over the visible keys.

Exact (integer views, so NaN patterns compare): the K row and the V row written at ``slot``, every other cache element
untouched, ``kstart == slot`` gives the new v itself, a repeated launch gives the same bits, poisoned dead memory (cache slots
outside [kstart, slot), the whole split workspace, the prompt slots of a beam group's non-first rows) changes no bit.

Tolerance of o: |got - ref| <= 2^-7 |ref| + 1e-3 max|V| -- one bf16 ulp for the final rounding, the absolute term for fp32
accumulation over <= 2304 keys and __expf.  Headroom of that bound, measured with a plain fp32 CPU restatement of split
attention (per-128-key (m, l, acc) states, then the merge; ``_restate_fp32``) on every case of this file against the float64
reference: the restatement's fp32 result, before any rounding to bf16, is at worst 7.1e-5 of the bound (asserted < 1/4 for
every case that is compared, ``_check_o``).  Rounded to bf16 like the kernel's output it is at worst 0.36 of the bound, and so
is the kernel on an MI355X: that is the half ulp of the final rounding, which the relative term is there for, and not the
accumulation the 1/4 is about.  Scores stay within +-8 (asserted): max |score| is 5.03 over all cases.
The operation is the attention of transformers' LlamaAttention with a KV cache (Emu2/emu/emu.py:213-229)."""
import functools
from types import SimpleNamespace
from typing import NamedTuple, Optional, Tuple

import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
CHUNK = 128                                    # keys per split (the operation's definition has none; cases are placed around it)
MAX_POS = 2304
DS = [64, 128]


class Case(NamedTuple):
    D: int
    H: int
    S_max: int
    ctx_max: int
    slot: Tuple[int, ...]                      # per row
    kstart: Optional[Tuple[int, ...]]          # per row, or None: the launch gets a null pointer
    pos: Optional[Tuple[int, ...]] = None      # None: slot - kstart
    share_nb: int = 0                          # > 1: rows are groups of share_nb beams with share_len identical prompt slots
    share_len: int = 0
    seed: int = 0


def _ops():
    from emu_amd import ops
    return ops


def _lib():
    from emu_amd._lib import lib
    return lib()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _scale(D):
    return float(torch.tensor(D ** -0.5, dtype=torch.float32))


def _rows(c):
    ks = c.kstart if c.kstart is not None else (0,) * len(c.slot)
    pos = c.pos if c.pos is not None else tuple(s - k for s, k in zip(c.slot, ks))
    return ks, pos


def _restate_fp32(qr, K, V, ks, slot, scale):
    """Split attention restated in plain fp32 on the CPU: one (max, sum, weighted V sum) state per 128-key split of the absolute
    key index, then the merge of the states.  qr [H, D], K / V [H, S, D] (the new token already at ``slot``) fp32 -> [H, D] fp32."""
    states = []
    for k0 in range(0, slot + 1, CHUNK):
        lo, hi = max(k0, ks), min(k0 + CHUNK, slot + 1)
        if lo >= hi:
            continue                                                       # a dead split: (m = -inf, l = 0) is dropped by the merge
        s = torch.einsum("hkd,hd->hk", K[:, lo:hi], qr) * torch.tensor(scale, dtype=torch.float32)
        m = s.max(-1).values
        p = torch.exp(s - m[:, None])
        states.append((m, p.sum(-1), torch.einsum("hk,hkd->hd", p, V[:, lo:hi])))
    mt = torch.stack([m for m, _, _ in states]).max(0).values
    num = torch.zeros_like(states[0][2])
    den = torch.zeros_like(mt)
    for m, l, acc in states:
        f = torch.exp(m - mt)
        num += f[:, None] * acc
        den += f * l
    return num / den[:, None]


@functools.lru_cache(maxsize=4)
def _data(c: Case):
    """Inputs (CPU), the float64 reference and the bound of one case; computed once, shared by the tests, never modified."""
    from oracle import emu2_ref as R
    B, H, D = len(c.slot), c.H, c.D
    ks, pos = _rows(c)
    assert all(0 <= k <= s < c.ctx_max <= c.S_max and 0 <= p < MAX_POS for k, s, p in zip(ks, c.slot, pos)), c
    g = torch.Generator().manual_seed(4100 + c.seed)
    qkv = torch.randn(B, 3 * H * D, generator=g).to(BF16)
    kc = torch.randn(B, H, c.S_max, D, generator=g).to(BF16)
    vc = torch.randn(B, H, c.S_max, D, generator=g).to(BF16)
    if c.share_nb > 1:                                                      # the beams of a group hold one prompt
        assert B % c.share_nb == 0 and all(s >= c.share_len for s in c.slot)
        for b in range(B):
            b0 = b - b % c.share_nb
            kc[b, :, :c.share_len] = kc[b0, :, :c.share_len]
            vc[b, :, :c.share_len] = vc[b0, :, :c.share_len]
    q3 = qkv.view(B, 3, H, D)
    cos, sin = R.rope_cos_sin(torch.tensor(pos, dtype=torch.long)[:, None], D, 10000.0, BF16)       # [B, 1, D]
    qr, kr = R.apply_rope(q3[:, 0, :, None, :], q3[:, 1, :, None, :], cos, sin)                     # bf16 ops, [B, H, 1, D]
    qr, kr, vn = qr[:, :, 0], kr[:, :, 0], q3[:, 2].clone()
    scale = _scale(D)
    ref = torch.empty(B, H, D, dtype=torch.float64)
    restated = torch.empty(B, H, D, dtype=torch.float32)
    smax = 0.0
    for b in range(B):
        lo, sl = ks[b], c.slot[b]
        K = torch.cat([kc[b, :, lo:sl], kr[b, :, None]], dim=1).double()                            # [H, n, D]
        V = torch.cat([vc[b, :, lo:sl], vn[b, :, None]], dim=1).double()
        s = torch.einsum("hkd,hd->hk", K, qr[b].double()) * scale
        smax = max(smax, float(s.abs().max()))
        ref[b] = torch.einsum("hk,hkd->hd", torch.softmax(s, -1), V)
        Kf = torch.cat([kc[b, :, :sl], kr[b, :, None]], dim=1).float()
        Vf = torch.cat([vc[b, :, :sl], vn[b, :, None]], dim=1).float()
        restated[b] = _restate_fp32(qr[b].float(), Kf, Vf, lo, sl, scale)
    assert smax <= 8.0, smax                                               # the inputs' side of the tolerance
    vmax = max(float(vc.float().abs().max()), float(vn.float().abs().max()))
    bound = 2.0 ** -7 * ref.abs() + 1e-3 * vmax
    return SimpleNamespace(qkv=qkv, kc=kc, vc=vc, kr=kr, vn=vn, ref=ref, bound=bound, scale=scale, smax=smax,
                           restated=float(((restated.double() - ref).abs() / bound).max()),
                           restated_bf16=float(((restated.to(BF16).double() - ref).abs() / bound).max()))


_NAN16 = torch.tensor([0x7FC0, 0x7F81, -1, -0x7F], dtype=torch.int16)                # quiet, signalling, all ones, negative
_NAN32 = torch.tensor([0x7FC00000, 0x7F800001, -1, -0x7FFFFF], dtype=torch.int32)


def _nan_like(t):
    pat = _NAN16 if t.dtype == BF16 else _NAN32
    return pat[torch.arange(t.numel()) % len(pat)].view(t.dtype).reshape(t.shape)


def _dead_slots(c: Case):
    """[B, S_max] bool: the cache slots a launch may not consume -- outside [kstart, slot) (the new token's own slot is written
    before anyone could read it), and for a beam group's non-first rows the prompt, which lives in the group's first row."""
    ks, _ = _rows(c)
    s = torch.arange(c.S_max)[None, :]
    dead = (s < torch.tensor(ks)[:, None]) | (s >= torch.tensor(c.slot)[:, None])
    if c.share_nb > 1:
        dead |= (s < c.share_len) & (torch.arange(len(c.slot)) % c.share_nb != 0)[:, None]
    return dead


def _caches(c: Case, fill: Optional[str]):
    """The case's caches with the dead slots as they are (None), zeroed ("zero") or holding NaN bit patterns ("nan")."""
    d = _data(c)
    kc, vc = d.kc.clone(), d.vc.clone()
    if fill is not None:
        dead = _dead_slots(c)[:, None, :, None].expand_as(kc)
        for t in (kc, vc):
            t[dead] = _nan_like(t)[dead] if fill == "nan" else 0
    return kc, vc


@functools.lru_cache(maxsize=2)
def _tables(D):
    from emu_amd.llama import rope_tables
    return rope_tables(D, MAX_POS, 10000.0, "cuda")


def _launch(c: Case, kc, vc, ws_fill="zero", arrive=None, share=True):
    """One launch on copies of the given CPU caches -> (o, K cache after, V cache after), all on the CPU."""
    ops, d = _ops(), _data(c)
    B = len(c.slot)
    ks, pos = _rows(c)
    cos, sin = _tables(c.D)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    ws = torch.zeros(_lib().emu_decode_fused_ws_bytes(B, c.H, c.D, c.ctx_max) // 4, dtype=torch.float32)
    assert ws.numel() == B * c.H * ((c.ctx_max + CHUNK - 1) // CHUNK) * (c.D + 2)
    if ws_fill == "nan":
        ws = _nan_like(ws)
    qkv, dk, dv = d.qkv.cuda(), kc.cuda(), vc.cuda()
    o = ops.decode_fused(qkv, cos, sin, i32(pos), i32(c.slot), dk, dv, c.H, c.ctx_max, d.scale,
                         kstart=None if c.kstart is None else i32(ks), ws=ws.cuda(),
                         share_nb=c.share_nb if share else 0, share_len=c.share_len if share else 0, arrive=arrive)
    torch.cuda.synchronize()
    assert same_bits(qkv.cpu(), d.qkv), "the launch wrote to the projection rows"
    return o.cpu(), dk.cpu(), dv.cpu()


def _check_o(c: Case, o, what=""):
    d = _data(c)
    print(f"{what} fp32 restatement / bound = {d.restated:.2e} (as bf16 {d.restated_bf16:.2f}), max |score| = {d.smax:.2f}")
    assert d.restated < 0.25, (d.restated, c)                              # the bound has room for fp32 split attention
    assert bool(torch.isfinite(o.float()).all()), what
    err = (o.double() - d.ref).abs() / d.bound                              # every element, none excluded
    print(f"{what} kernel / bound = {float(err.max()):.3f}")
    assert float(err.max()) <= 1.0, (what, float(err.max()), [int(i) for i in (err == err.max()).nonzero()[0]], c)


def _check_caches(c: Case, before, after, what=""):
    """Exactly one K row and one V row per (row, head) were written -- the oracle-rotated key and the projection's v -- and every
    other element of both caches holds the bits it held before."""
    d = _data(c)
    for name, b4, aft, new in (("K", before[0], after[0], d.kr), ("V", before[1], after[1], d.vn)):
        want = b4.clone()
        for b, sl in enumerate(c.slot):
            assert same_bits(aft[b, :, sl], new[b]), f"{what}: {name} row written at slot {sl} of row {b}"
            want[b, :, sl] = new[b]
        diff = _bits(aft) != _bits(want)
        assert not bool(diff.any()), f"{what}: {name} cache changed outside the new slot at {diff.nonzero()[:4].tolist()}"


def _full_check(c: Case, fill=None, ws_fill="zero", what=""):
    kc, vc = _caches(c, fill)
    o, k1, v1 = _launch(c, kc, vc, ws_fill)
    _check_caches(c, (kc, vc), (k1, v1), what)
    _check_o(c, o, what)
    return o


# ------------------------------------------------------------------------------------------------------------ cases
SLOTS = [0, 1, 126, 127, 128, 129, 255, 256, 700]


def _slot_case(D, slot, tight):
    # tight: the launch and the cache end with the new token (the kernel's clamped loads have nothing behind it);
    # bucket-sized: dead splits behind the live ones
    n = slot + 1 if tight else 1024
    return Case(D, 2, n, n, (slot, slot), None, seed=slot)


SLOT_CASES = [_slot_case(D, s, t) for D in DS for s in SLOTS for t in (True, False)]
# rows of one batch at different slots, left padded: the RoPE position is not the slot
ROWS_CASES = [Case(D, 3, 512, cm, (5, 127, 300), (3, 0, 129), seed=11) for D in DS for cm in (301, 512)]
# left padding at slot 400, one row each: none, one key, up to a split's last key, a whole split, a split and a key, two splits
# and a partly masked third; and everything but the new token
KSTART_CASES = [Case(D, 2, 512, cm, (400,) * 7, (0, 1, 127, 128, 129, 300, 400), seed=12) for D in DS for cm in (401, 512)]
ONLY_NEW_CASES = [Case(D, 3, 512, 512, (0, 5, 128, 400), (0, 5, 128, 400), pos=(0, 0, 7, 33), seed=13) for D in DS]


def _combine_case(D, ctx_max):
    # 1 / 8 / 9 / 16 / 17 splits: the unrolled forms of 8 and of 16 at their last size, the 16 form at its first, the loop form
    s_max = (ctx_max + CHUNK - 1) // CHUNK * CHUNK
    slot = (0, ctx_max // 2, ctx_max - 1, ctx_max - 1)
    return Case(D, 2, s_max, ctx_max, slot, (0, 0, 0, min(130, ctx_max - 1)), seed=ctx_max)


COMBINE_CASES = [_combine_case(D, cm) for D in DS for cm in (128, 1024, 1025, 2048, 2176)]
POISON_CASES = ROWS_CASES + KSTART_CASES + [Case(D, 2, 1024, 1024, (700, 129), (0, 128), seed=14) for D in DS] + COMBINE_CASES[4::5]
ARRIVE_CASES = ROWS_CASES + KSTART_CASES[1::2] + [c for c in SLOT_CASES if c.slot[0] in (0, 700)] + COMBINE_CASES[4::5]


def _share_case(D, nb, share_len, off):
    # two prompts of nb beams; the second one is left padded by a whole split and more where the prompt is that long (a prompt
    # of 128 slots: all of it, so its one shared split is dead; of 100: no padding of >= 128 can leave a key visible)
    k1 = {100: 37, 128: 128}.get(share_len, 130)
    slot = share_len + off
    return Case(D, 2, 384, 384, (slot,) * (2 * nb), (5,) * nb + (k1,) * nb, share_nb=nb, share_len=share_len,
                seed=share_len + nb)


SHARE_NB = [2, 3, 4, 5, 6, 8]
SHARE_LEN = [100, 128, 200, 256, 300]
ALL_CASES = (SLOT_CASES + ROWS_CASES + KSTART_CASES + ONLY_NEW_CASES + COMBINE_CASES + POISON_CASES + ARRIVE_CASES +
             [_share_case(D, nb, sl, off) for D in DS for nb in SHARE_NB for sl in SHARE_LEN for off in (0, 3)])


def _id(c):
    return (f"D{c.D}-slot{'_'.join(map(str, sorted(set(c.slot))))}-ctx{c.ctx_max}of{c.S_max}" +
            ("" if c.kstart is None else f"-ks{'_'.join(map(str, sorted(set(c.kstart))))}"))


# ------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("c", SLOT_CASES, ids=_id)
def test_slots_around_the_split_edges(c):
    """The new token's slot inside, at the end of, and just behind a 128-key split; launches sized tightly and by a bucket.  Two
    launches on restored caches give identical bits."""
    o = _full_check(c, what=_id(c))
    o2, _, _ = _launch(c, *_caches(c, None))
    assert same_bits(o, o2)


@pytest.mark.parametrize("c", ROWS_CASES + KSTART_CASES, ids=_id)
def test_rows_with_their_own_slot_position_and_left_padding(c):
    o = _full_check(c, what=_id(c))
    o2, _, _ = _launch(c, *_caches(c, None))
    assert same_bits(o, o2)


@pytest.mark.parametrize("c", ONLY_NEW_CASES, ids=_id)
def test_only_the_new_token_visible_gives_its_value_exactly(c):
    """kstart == slot: a softmax over one key is 1, so o is the new v bit for bit -- whatever the key is, whatever lies below."""
    for fill in (None, "nan"):
        kc, vc = _caches(c, fill)
        o, k1, v1 = _launch(c, kc, vc, "nan" if fill else "zero")
        _check_caches(c, (kc, vc), (k1, v1), _id(c))
        assert same_bits(o, _data(c).vn), fill
    _check_o(c, o, _id(c))


@pytest.mark.parametrize("c", POISON_CASES, ids=_id)
def test_dead_cache_slots_and_workspace_are_never_consumed(c):
    """NaN bit patterns in every K and V slot outside [kstart, slot) and in the whole split workspace: the output is finite,
    within the bound, and bit-equal to the launch with zeros there; the poison itself is still in place afterwards."""
    o_nan = _full_check(c, "nan", "nan", what=_id(c) + " poisoned")
    o_zero = _full_check(c, "zero", "zero", what=_id(c) + " zeroed")
    assert bool(torch.isfinite(o_nan.float()).all())
    assert same_bits(o_nan, o_zero)


@pytest.mark.parametrize("c", COMBINE_CASES, ids=_id)
def test_combine_forms(c):
    """The merge of 1, 8, 9, 16 and 17 splits (the unrolled forms of 8 and 16, and the loop form on its own merit), each again
    with the loop form forced (emu_gemm_tune bit 20): same bits, with a clean and with a poisoned workspace."""
    o = _full_check(c, what=_id(c))
    try:
        _lib().emu_gemm_tune(1 << 20)
        o_loop = _full_check(c, what=_id(c) + " loop form")
        o_loop_nan, _, _ = _launch(c, *_caches(c, None), ws_fill="nan")
    finally:
        _lib().emu_gemm_tune(0)
    o_nan, _, _ = _launch(c, *_caches(c, None), ws_fill="nan")
    assert same_bits(o, o_loop) and same_bits(o, o_loop_nan) and same_bits(o, o_nan)


@pytest.mark.parametrize("share_len", SHARE_LEN)
@pytest.mark.parametrize("nb", SHARE_NB)
@pytest.mark.parametrize("D", DS)
def test_beams_sharing_the_prompt(D, nb, share_len):
    """Groups of nb beams whose prompt is stored in the group's first row only (the other rows' prompt slots hold NaN patterns):
    every row within the bound of the reference, the whole launch bit-equal to the one on replicated caches.  Every NB
    instantiation (2, 4, 5, 8; 3 and 6 run with idle beams), prompts ending inside / on a split edge and without a whole shared
    split, the new token right behind the prompt and three generated slots (which differ per beam) further."""
    for off in (0, 3):
        c = _share_case(D, nb, share_len, off)
        what = f"{_id(c)} nb{nb} share{share_len}"
        d = _data(c)
        if off:
            assert not same_bits(d.kc[0, :, share_len:c.slot[0]], d.kc[1, :, share_len:c.slot[0]])
        kc, vc = _caches(c, "nan")                                          # poisons the non-first rows' prompt slots as well
        assert not bool(torch.isfinite(kc[1, :, :share_len].float()).any())
        o, k1, v1 = _launch(c, kc, vc, "nan")
        _check_caches(c, (kc, vc), (k1, v1), what)
        _check_o(c, o, what)
        o_rep, k2, v2 = _launch(c, d.kc, d.vc, share=False)
        _check_caches(c, (d.kc, d.vc), (k2, v2), what + " replicated")
        assert same_bits(o, o_rep), what
        assert not same_bits(o[0], o[1])                                    # beams do differ


@pytest.mark.parametrize("c", ARRIVE_CASES, ids=_id)
def test_tail_merge_by_the_last_split_to_arrive(c):
    """DecodeFusedArgs::arrive: no combine launch, the last split workgroup of a head merges it.  Same bits as the combine form,
    the counters are zero again afterwards, and a second launch on the same counters (and a poisoned workspace) repeats them."""
    o = _full_check(c, what=_id(c))
    arrive = torch.zeros(len(c.slot) * c.H, dtype=torch.int32, device="cuda")
    for ws_fill in ("zero", "nan"):
        kc, vc = _caches(c, None)
        o_tail, k1, v1 = _launch(c, kc, vc, ws_fill, arrive=arrive)
        _check_caches(c, (kc, vc), (k1, v1), _id(c) + " tail merge")
        assert same_bits(o_tail, o), ws_fill
        assert int(arrive.abs().max()) == 0, arrive.tolist()
