"""GPU: the prefill flash-attention launch (flash_kernel, csrc/attention.hip, through emu_flash_attn_bf16) and the producer of its
V^T operand (transpose_v_kernel, emu_transpose_v_bf16) on their own, against a float64 reference written from the definition.

Reference, per (b, h): softmax(q k^T scale + mask) v in float64 on the bf16 input values; the mask is ``kstart[b] <= key`` and, when
causal, ``key <= i + (Sk - Sq)``; ``scale`` is the float32 value of D ** -0.5.  With the same weights, A = softmax(..) |v|.

Bound, for every element of every query row that sees at least one key:

    |got - ref| <= 1.02 * 2^-8 * (|ref| + A)

Derivation (from the code, none of it measured on the kernel): the kernel keeps the row sum l in fp32 from the unrounded weights p but
feeds bf16(p) to the P.V MFMA -- at most 2^-8 relative per weight, so at most 2^-8 A per output; it rounds O to bf16 once, at most
2^-8 |o|.  Everything else is far below that (fp32 accumulation over at most a few thousand keys, v_exp_f32, the scale folded into
the exponent's fma); the 2 % is for these and for second-order terms.  Rows that see no key (left-padded queries) must be exactly
zero, either sign.  No element is excluded from any comparison.

``_restate`` is a plain CPU restatement of the algorithm (64-key tiles, fp32 online softmax in the exp2 domain with the running-max
rescale, ``p.to(bf16)`` ahead of the P.V product, one final rounding).  It is asserted to stay <= 1.0 of the bound on every case
(``_check``); its worst ratio over all cases and input kinds of this file is RESTATED_WORST below.  If it goes over 1.0 on a new
case, the case or the derivation is wrong: the constant is not raised.  tests/test_flash_bound_host.py shows, without a GPU, that
restatements with one deliberate error each (a mask bound off by one key for the query rows >= 128, a dropped key tile, a swapped
V row) exceed the bound where the earlier criterion 2e-2 + 2e-2 |want| let them pass.

Inputs, three kinds per case, all bf16, max |score| <= 40 asserted: ``rand`` (randn q, k, v); ``point`` (q[i] = 2 k[t(i)], so the
softmax sits on one key and o ~ v[t(i)]: a dropped, shifted or mis-addressed key is an O(1) error; t(i) cycles through the visible
range, every third query hits its last visible key, every fifth its first, and every visible 64-key tile edge is some query's
target); ``big`` (rand with v * 8 + 3: an error in l or in the rescale shows against a non-zero mean).

Exact (integer views, so NaN patterns compare): a second launch; every form of the kernel (straight / XCD order, staged / direct O
stores, 4 / 8 waves, heavy_first on / off); one (b, h) pair alone against its slice of the batched launch; O outside [B, Sq, H, D]
untouched; NaN patterns in masked K rows, the largest finite values in masked V rows, NaN patterns behind Sq / Sk / ceil64(Sk);
emu_transpose_v_bf16 against ``transpose`` + zero pad; refusals write nothing.

Kernel's worst ratio to the bound per test group on MI355X: MEASURED below (largest over the three input kinds).
"""
import functools
from types import SimpleNamespace
from typing import NamedTuple, Optional, Tuple

import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
TILE = 64                                      # keys per tile; 32 queries per wave, 128 (256 in the 8-wave form) per workgroup
DS = [64, 128]
KINDS = ("rand", "point", "big")
BOUND_C = 1.02 * 2.0 ** -8
LOG2E = 1.4426950408889634

# worst |restatement - ref| / bound over every case and input kind of this file (CPU)
RESTATED_WORST = 0.858                         # D = 128, 129 heads x 256 x 256 causal, rand; per group 0.48 .. 0.86
# worst |kernel - ref| / bound on MI355X, per group of test_against_the_reference
# (printed per case as "MEASURED [group] ratio").  In all 282 (case, kind) pairs the kernel's ratio equals the restatement's to the
# three digits printed: the worst element is decided by the two bf16 roundings, which the two perform alike.
MEASURED = {"key-count edges": 0.731, "query-count edges": 0.775, "chunked-prefill windows": 0.484, "left padding": 0.737,
            "natural dispatch": 0.858, "packed qkv": 0.702}


class Case(NamedTuple):
    D: int
    B: int
    H: int
    Sq: int
    Sk: int
    causal: bool
    kstart: Optional[Tuple[int, ...]] = None   # per batch row, or None: the launch gets a null pointer
    packed: bool = False                       # q, k, v are slices of one [B, S, 3, H, D] buffer


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


def _ks(c):
    return c.kstart if c.kstart is not None else (0,) * c.B


def _visible(c):
    """(lo [B, Sq], hi [B, Sq]): query i of row b sees the keys lo <= key <= hi (none where lo > hi)."""
    i = torch.arange(c.Sq)
    hi = torch.clamp(i + (c.Sk - c.Sq), max=c.Sk - 1) if c.causal else torch.full((c.Sq,), c.Sk - 1)
    lo = torch.tensor(_ks(c))[:, None].expand(c.B, c.Sq)
    return lo, hi[None].expand(c.B, c.Sq)


def _targets(c):
    """The ``point`` kind's key per query, [B, Sq] (-1: the row sees no key), and the visible tile edges no query got."""
    lo, hi = _visible(c)
    tgt = torch.full((c.B, c.Sq), -1, dtype=torch.long)
    missed = []
    for b in range(c.B):
        edges = {e for n in range(1, (c.Sk + TILE - 1) // TILE) for e in (TILE * n - 1, TILE * n)
                 if int(lo[b, 0]) <= e <= int(hi[b, -1])}                   # visible to the last query at least
        for i in range(c.Sq):
            l, h = int(lo[b, i]), int(hi[b, i])
            if l > h:
                continue
            seen = [e for e in edges if l <= e <= h]
            if i % 3 == 0:
                t = h
            elif i % 5 == 0:
                t = l
            elif seen:
                t = max(seen)                                              # causal: the edge the fewest later queries can see
            else:
                t = l + (7 * i + b) % (h - l + 1)
            edges.discard(t)
            tgt[b, i] = t
        missed += [(b, e) for e in sorted(edges)]
    return tgt, missed


@functools.lru_cache(maxsize=8)
def _inputs(c: Case, kind: str):
    """q [B, Sq, H, D], k, v [B, Sk, H, D], bf16 on the CPU; computed once per case and kind, never modified."""
    assert kind in KINDS and all(0 <= s < c.Sk for s in _ks(c)) and len(_ks(c)) == c.B, c
    seed = (c.D * 1000003 + c.Sq * 10007 + c.Sk * 101 + c.B * 31 + c.H * 7 + int(c.causal) + 2 * sum(_ks(c))) % (2 ** 31)
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(c.B, c.Sq, c.H, c.D, generator=g).to(BF16)
    k = torch.randn(c.B, c.Sk, c.H, c.D, generator=g).to(BF16)
    v = torch.randn(c.B, c.Sk, c.H, c.D, generator=g).to(BF16)
    if kind == "big":
        v = (v.float() * 8 + 3).to(BF16)
    if kind == "point":
        tgt, missed = _targets(c)
        assert not missed or c.Sq == 1, (c, missed)                         # one query cannot hit every edge
        for b in range(c.B):
            live = tgt[b] >= 0
            q[b, live] = (2 * k[b, tgt[b, live]].float()).to(BF16)          # exact
    return q, k, v


def reference(q, k, v, ks, causal, scale):
    """float64 on the bf16 values -> (ref [B, Sq, H, D], A = the same weights on |v|, live [B, Sq], max |score| of a visible key)."""
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    qd, kd, vd = (t.double().permute(0, 2, 1, 3) for t in (q, k, v))       # [B, H, S, D]
    s = qd @ kd.transpose(-1, -2) * scale
    key = torch.arange(Sk)
    ok = key[None, None, :] >= torch.tensor(ks)[:, None, None]
    if causal:
        ok = ok & (key[None, None, :] <= (torch.arange(Sq) + (Sk - Sq))[None, :, None])
    ok = ok.expand(B, Sq, Sk)[:, None]                                      # [B, 1, Sq, Sk]
    live = ok[:, 0].any(-1)
    smax = float(s.abs()[ok.expand_as(s)].max()) if bool(live.any()) else 0.0
    s = s.masked_fill(~ok, float("-inf"))
    m = s.max(-1, keepdim=True).values
    w = torch.exp(s - torch.where(torch.isinf(m), torch.zeros_like(m), m))  # rows without a key: all zero
    l = w.sum(-1, keepdim=True)
    w = w / torch.where(l > 0, l, torch.ones_like(l))
    return (w @ vd).permute(0, 2, 1, 3), (w @ vd.abs()).permute(0, 2, 1, 3), live, smax


def bound_of(ref, A):
    return BOUND_C * (ref.abs() + A)


def _restate(q, k, v, ks, causal, scale, mutant=None):
    """flash_kernel's algorithm restated in plain fp32 on the CPU -> bf16 [B, Sq, H, D].  ``mutant``: one deliberate error
    (tests/test_flash_bound_host.py): "kstart+1" / "causal+1" (the bound off by one key for the query rows >= 128), "drop_last" /
    "drop_tile1" (a key tile skipped), "v70" (v[70] replaced by v[71])."""
    assert mutant in (None, "kstart+1", "causal+1", "drop_last", "drop_tile1", "v70")
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    f32 = torch.float32
    qf, kf, vf = (t.float().permute(0, 2, 1, 3) for t in (q, k, v))
    if mutant == "v70":
        vf = vf.clone()
        vf[:, :, 70] = vf[:, :, 71]
    sc = torch.tensor(scale, dtype=f32) * torch.tensor(LOG2E, dtype=f32)    # softmax in the exp2 domain
    lo = torch.tensor(ks)[:, None].expand(B, Sq).clone()
    hi = (torch.arange(Sq) + (Sk - Sq)) if causal else torch.full((Sq,), Sk - 1)
    hi = hi[None].expand(B, Sq).clone()
    if mutant == "kstart+1":
        lo[:, 128:] += 1
    if mutant == "causal+1":
        assert causal
        hi[:, 128:] += 1
    ninf = torch.tensor(float("-inf"), dtype=f32)
    m = torch.full((B, H, Sq), float("-inf"), dtype=f32)
    l = torch.zeros(B, H, Sq, dtype=f32)
    o = torch.zeros(B, H, Sq, D, dtype=f32)
    ntile = (Sk + TILE - 1) // TILE
    for t in range(ntile):
        if (mutant == "drop_last" and t == ntile - 1) or (mutant == "drop_tile1" and t == 1):
            continue
        key = torch.arange(t * TILE, min(t * TILE + TILE, Sk))
        ok = (key[None, None, :] >= lo[:, :, None]) & (key[None, None, :] <= hi[:, :, None])       # [B, Sq, n]
        s = torch.where(ok[:, None], qf @ kf[:, :, key].transpose(-1, -2), ninf)
        mnew = torch.maximum(m, s.max(-1).values * sc)                      # sc > 0: the maximum commutes with the scale
        dead = torch.isinf(mnew)                                            # every key so far masked for this query
        alpha = torch.where(dead, torch.ones_like(m), torch.exp2(m - mnew))
        nm = torch.where(dead, torch.zeros_like(m), -mnew)
        p = torch.exp2(s * sc + nm[..., None])                              # masked: exp2(-inf) = 0
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + p.to(BF16).float() @ vf[:, :, key]
        m = mnew
    inv = torch.where(l > 0, 1 / l, torch.zeros_like(l))
    return (o * inv[..., None]).to(BF16).permute(0, 2, 1, 3)


def ratio_to_bound(got, ref, bound, live):
    """max over the live rows' elements of |got - ref| / bound; the rows that see no key must be zero bit patterns."""
    dead_rows = got[~live]
    assert bool(((_bits(dead_rows) & 0x7FFF) == 0).all()), "a query row without a visible key is not exactly zero"
    if not bool(live.any()):
        return 0.0
    err, bd = (got.double() - ref).abs()[live], bound[live]
    assert bool(torch.isfinite(got.float()).all())
    # a zero bound (``big``: -0.375 * 8 + 3 is an exact zero, alone under a causal first query) asks for the exact result
    return float(torch.where(bd > 0, err / bd, torch.where(err > 0, float("inf"), 0.0).double()).max())


@functools.lru_cache(maxsize=4)
def _data(c: Case, kind: str):
    """The float64 reference, the bound and the restatement's ratio of one case and kind; computed once, never modified."""
    q, k, v = _inputs(c, kind)
    scale = _scale(c.D)
    ref, A, live, smax = reference(q, k, v, _ks(c), c.causal, scale)
    assert smax <= 40.0, (c, kind, smax)                                    # the inputs' side of the bound
    bound = bound_of(ref, A)
    restated = ratio_to_bound(_restate(q, k, v, _ks(c), c.causal, scale), ref, bound, live)
    return SimpleNamespace(ref=ref, bound=bound, live=live, smax=smax, restated=restated)


# ------------------------------------------------------------------------------------------------------------ launches
def _dev(c: Case, kind: str):
    """The case's operands on the GPU (views of one packed projection buffer where the case says so) and its kstart."""
    q, k, v = _inputs(c, kind)
    if c.packed:
        assert c.Sq == c.Sk
        buf = torch.stack([q, k, v], dim=2).cuda()                          # [B, S, 3, H, D]
        q, k, v = buf[:, :, 0], buf[:, :, 1], buf[:, :, 2]
        assert not q.is_contiguous()
    else:
        q, k, v = q.cuda(), k.cuda(), v.cuda()
    ks = None if c.kstart is None else torch.tensor(c.kstart, dtype=torch.int32, device="cuda")
    return q, k, v, ks


def _launch(c: Case, q, k, v, ks, tune=0, **kw):
    ops = _ops()
    try:
        if tune:
            _lib().emu_gemm_tune(tune)
        o = ops.flash_attn(q, k, v, c.causal, _scale(c.D), kstart=ks, **kw)
        torch.cuda.synchronize()
    finally:
        if tune:
            _lib().emu_gemm_tune(0)
    return o.cpu()


def _form(D, B, H, Sq, causal, tune=0):
    """launch_flash_attn's choice restated: (waves per workgroup, heavy_first, workgroups launched)."""
    wg4 = (Sq + 127) // 128 * H * B
    w8 = D == 64 and 256 < wg4 <= 400 and Sq >= 256
    if (tune >> 12) & 3 == 1:
        w8 = False
    if (tune >> 12) & 3 == 2:
        w8 = D == 64
    heavy = bool(causal) and not w8 and Sq >= 256 and wg4 > 256 and not tune & (1 << 15)
    grid = (Sq + 255) // 256 * H * B if w8 else (8 * ((H * B + 7) // 8) * ((Sq + 127) // 128) if heavy else wg4)
    return (8 if w8 else 4), heavy, grid


def _check(c: Case, kind: str, o, what=""):
    d = _data(c, kind)
    print(f"{what} {kind}: restatement / bound = {d.restated:.3f}, max |score| = {d.smax:.2f}")
    assert d.restated <= 1.0, (d.restated, c, kind)                         # the bound holds for the algorithm as stated
    r = ratio_to_bound(o, d.ref, d.bound, d.live)                           # every element, none excluded
    print(f"{what} {kind}: kernel / bound = {r:.3f}")
    assert r <= 1.0, (what, kind, r, c)
    return r


# ------------------------------------------------------------------------------------------------------------ cases
def _edge(D, Sq, Sk, causal, **kw):
    return Case(D, 2, 2, Sq, Sk, causal, **kw)


KEY_EDGES = [_edge(D, S, S, causal) for D in DS for S in (1, 63, 64, 65, 127, 128, 129, 200) for causal in (True, False)]
QUERY_EDGES = [_edge(D, Sq, Sk, causal) for D in DS for Sq in (1, 31, 32, 33, 127, 128, 129, 255, 256, 257)
               for Sk, causal in ((Sq, True), (300, False))]
WINDOWS = [_edge(D, Sq, Sk, True) for D in DS for Sq, Sk in ((1, 300), (5, 77), (70, 200), (130, 333))]
# left padding, a different one per batch row: dead rows and live rows share one wave and one query block
LEFT_PAD = [Case(D, 3, 2, Sq, Sk, True, ks) for D in DS for Sq, Sk in ((260, 260), (70, 200))
            for ks in ((0, 63, 130), (1, 64, Sk - 1), (65, 130, 0))] + [Case(D, 3, 2, 260, 260, True, None) for D in DS]
# the smallest shape at which the launcher picks each form by itself: (case, waves, heavy_first, workgroups)
DISPATCH = [
    (Case(64, 3, 43, 256, 256, False), 8, False, 129),                      # wg4 = 258: 256-query workgroups
    (Case(128, 3, 43, 256, 256, True), 4, True, 8 * 17 * 2),                # 129 heads: 1 XCD owns 17, 7 own 16, surplus blocks leave
    (Case(128, 2, 68, 300, 300, True), 4, True, 136 * 3),                   # 136 heads, a ragged last query block
    (Case(64, 3, 67, 256, 256, True), 4, True, 8 * 26 * 2),                 # wg4 = 402 > 400: 4 waves
]
PACKED = [Case(D, 2, 2, 150, 150, True, ks, packed=True) for D in DS for ks in (None, (0, 37))]
GROUPS = {"key-count edges": KEY_EDGES, "query-count edges": QUERY_EDGES, "chunked-prefill windows": WINDOWS,
          "left padding": LEFT_PAD, "natural dispatch": [c for c, *_ in DISPATCH], "packed qkv": PACKED}
ALL_CASES = list(dict.fromkeys(c for cs in GROUPS.values() for c in cs))    # each case once
GROUPED = [(next(g for g, cs in GROUPS.items() if c in cs), c) for c in ALL_CASES]
# memory contracts: left-padded (a masked key exists), a window, no mask at all, the 8-wave form's default
MEM_CASES = LEFT_PAD[1::3][:4] + [Case(D, 2, 2, 130, 333, True, (3, 70)) for D in DS] + [Case(64, 2, 2, 257, 300, False, (64, 1)),
                                                                                        Case(128, 2, 3, 129, 129, False, None)]


def _id(c):
    return (f"D{c.D}-B{c.B}H{c.H}-{c.Sq}x{c.Sk}-{'causal' if c.causal else 'full'}" +
            ("" if c.kstart is None else f"-ks{'_'.join(map(str, c.kstart))}") + ("-packed" if c.packed else ""))


TUNES = [1 << 6, 1 << 7, (1 << 6) | (1 << 7), 1 << 15]
TUNES_D64 = [1 << 12, 2 << 12, (1 << 12) | 192, (2 << 12) | 192]


# ------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("group,c", GROUPED, ids=lambda x: _id(x) if isinstance(x, Case) else x.replace(" ", "_"))
def test_against_the_reference(group, c):
    """Every case and input kind at the default dispatch, every element compared; a second launch gives the same bits."""
    for kind in KINDS:
        ops = _dev(c, kind)
        o = _launch(c, *ops)
        r = _check(c, kind, o, _id(c))
        print(f"MEASURED [{group}] {r:.3f}")
        assert same_bits(o, _launch(c, *ops)), kind


@pytest.mark.parametrize("c,waves,heavy,grid", DISPATCH, ids=lambda x: _id(x) if isinstance(x, Case) else str(x))
def test_the_dispatch_cases_select_their_form(c, waves, heavy, grid):
    """No launch: the launcher's conditions, restated in ``_form``, pick the form each DISPATCH case is there for; bit 15 (and only
    it) takes heavy_first away; no other case of this file reaches the 8-wave form or heavy_first by itself."""
    assert _form(c.D, c.B, c.H, c.Sq, c.causal) == (waves, heavy, grid)
    assert _form(c.D, c.B, c.H, c.Sq, c.causal, 1 << 15) == (waves, False, (c.Sq + 32 * waves - 1) // (32 * waves) * c.H * c.B)
    assert grid >= (c.Sq + 32 * waves - 1) // (32 * waves) * c.H * c.B
    others = [o for o in ALL_CASES if o not in [d for d, *_ in DISPATCH]]
    assert all(_form(o.D, o.B, o.H, o.Sq, o.causal)[:2] == (4, False) for o in others)


@pytest.mark.parametrize("c", ALL_CASES, ids=_id)
def test_every_form_gives_the_same_bits(c):
    """emu_gemm_tune: bit 6 straight block order, bit 7 direct O stores, both, bit 15 heavy_first off; at D = 64 bits 12-13 = 1 / 2
    (always 4 / 8 waves), alone and with 6|7.  All bit-equal to the default's, D = 128 and the heavy_first shapes included."""
    for kind in KINDS:
        ops = _dev(c, kind)
        o = _launch(c, *ops)
        for tune in TUNES + (TUNES_D64 if c.D == 64 else []):
            assert same_bits(o, _launch(c, *ops, tune=tune)), (kind, hex(tune))         # (_launch resets the mask in ``finally``)


@pytest.mark.parametrize("c", ALL_CASES, ids=_id)
def test_a_head_alone_equals_its_slice_of_the_batch(c):
    """One (b, h) pair launched alone -- another workgroup, another XCD, a different remap, never heavy_first or 8 waves -- gives
    the bits of its slice of the batched launch."""
    pairs = sorted({(0, 0), (c.B - 1, c.H - 1), (c.B // 2, c.H // 2), (0, c.H - 1)})
    for kind in KINDS:
        q, k, v, ks = _dev(c, kind)
        o = _launch(c, q, k, v, ks)
        for b, h in pairs:
            one = c._replace(B=1, H=1)
            alone = _launch(one, q[b:b + 1, :, h:h + 1], k[b:b + 1, :, h:h + 1], v[b:b + 1, :, h:h + 1],
                            None if ks is None else ks[b:b + 1].contiguous())
            assert same_bits(alone[0, :, 0], o[b, :, h]), (kind, b, h)


# ---- memory contracts, all exact on integer views
def _sentinel(n):
    return ((torch.arange(n, dtype=torch.int64) * 2654435761 >> 7) % 65536 - 32768).to(torch.int16)


def _vt(v, S, S_pad=None):
    """ops.transpose_v of v [B, S, H, D] (any strides), with the zero pad the flash kernel relies on asserted on the result."""
    B, _, H, D = v.shape
    vt = _ops().transpose_v(v, B, H, S, D, v.stride(0), v.stride(2), v.stride(1), S_pad)
    torch.cuda.synchronize()
    assert vt.shape[-1] % TILE == 0 and vt.shape[-1] >= S
    assert bool((_bits(vt[..., S:]) == 0).all()), "V^T pad is not zero"
    return vt


O_LAYOUTS = ["staged", "direct by tune bit 7", "direct by a token stride = 4 mod 8", "direct by a base 8 bytes off a 16-byte line"]


@pytest.mark.parametrize("layout", O_LAYOUTS)
@pytest.mark.parametrize("c", MEM_CASES, ids=_id)
def test_o_outside_the_result_is_untouched(c, layout):
    """o is a view into a larger, sentinel-filled buffer: a token stride above H * D, rows beyond Sq, elements in front.  Only
    [B, Sq, H, D] changes, and to the bits of the plain launch -- staged stores, direct stores forced, and direct stores taken by
    the launcher's own condition (an O stride that is a multiple of 4 but not of 8; a base that is not 16-byte aligned)."""
    HD = c.H * c.D
    row = HD + (4 if "stride" in layout else 8)
    front = 4 if "base" in layout else 8
    n = front + c.B * (c.Sq + 2) * row
    for kind in ("rand", "point"):
        q, k, v, ks = _dev(c, kind)
        want_o = _launch(c, q, k, v, ks)
        buf = _sentinel(n).cuda()
        o = buf.view(BF16).as_strided((c.B, c.Sq, c.H, c.D), ((c.Sq + 2) * row, row, c.D, 1), front)
        direct = bool((o.stride(0) | o.stride(1) | o.stride(2)) & 7) or bool(o.data_ptr() & 15)    # the launcher's condition
        assert direct == (layout in O_LAYOUTS[2:]) and o.data_ptr() % 8 == 0
        got = _launch(c, q, k, v, ks, tune=(1 << 7) if "tune" in layout else 0, out=o)
        assert same_bits(got, want_o), (kind, layout)
        want = _sentinel(n)
        want.view(BF16).as_strided(o.shape, o.stride(), front).copy_(want_o)
        diff = buf.cpu() != want
        assert not bool(diff.any()), f"{layout}: buffer changed outside the result at {diff.nonzero()[:4].tolist()}"


_NAN16 = torch.tensor([0x7FC0, 0x7F81, -1, -0x7F], dtype=torch.int16)                # quiet, signalling, all ones, negative


def _nan_like(t):
    return _NAN16[torch.arange(t.numel()) % len(_NAN16)].view(BF16).reshape(t.shape)


def _masked_keys(c):
    """[B, Sk] bool: keys in front of kstart[b]."""
    return torch.arange(c.Sk)[None, :] < torch.tensor(_ks(c))[:, None]


@pytest.mark.parametrize("c", [c for c in MEM_CASES if c.kstart], ids=_id)
def test_k_rows_of_masked_keys_are_never_consumed(c):
    """A masked key's score is selected away, not added to: NaN bit patterns in every K row with key < kstart[b] give the bits of
    the launch with zeros there, and of the launch on the data as it was."""
    dead = _masked_keys(c)[:, :, None, None]
    assert bool(dead.any())
    for kind in KINDS:
        q, k, v, ks = _dev(c, kind)
        k_cpu = _inputs(c, kind)[1]
        outs = [_launch(c, q, k, v, ks)]
        for fill in (torch.zeros_like(k_cpu), _nan_like(k_cpu)):
            outs.append(_launch(c, q, torch.where(dead, fill, k_cpu).cuda(), v, ks))
        assert bool(torch.isfinite(outs[2].float()).all())
        assert same_bits(outs[1], outs[2]) and same_bits(outs[0], outs[1]), kind


@pytest.mark.parametrize("c", [c for c in MEM_CASES if c.kstart], ids=_id)
def test_v_rows_of_masked_keys_count_as_zero_times_v(c):
    """A masked key's weight is an exact zero, but its V row does reach the P.V MFMA, as 0 * v: + and - the largest finite bf16 in
    every V row with key < kstart[b] give the bits of the launch with zeros there (and of the data as it was).  NaN or Inf in
    such a row is outside the contract (0 * NaN = NaN): whoever leaves the cache's dead slots to the kernel keeps them finite."""
    dead = _masked_keys(c)[:, :, None, None]
    for kind in KINDS:
        q, k, v, ks = _dev(c, kind)
        v_cpu = _inputs(c, kind)[2]
        big = torch.full(v_cpu.shape, 0x7F7F, dtype=torch.int16)
        big[..., 1::2] = -0x0081                                            # 0xFF7F: the largest finite bf16, negative
        outs = [_launch(c, q, k, v, ks)]
        for fill in (torch.zeros_like(v_cpu), big.view(BF16)):
            outs.append(_launch(c, q, k, torch.where(dead, fill, v_cpu).cuda(), ks))
        assert float(big.view(BF16).float().abs().min()) > 3.3e38
        assert same_bits(outs[1], outs[2]) and same_bits(outs[0], outs[1]), kind


@pytest.mark.parametrize("c", MEM_CASES, ids=_id)
def test_nothing_behind_the_operands_is_read(c):
    """q, k, v are the leading rows of larger buffers whose rows >= Sq / >= Sk hold NaN patterns, and V^T has one more 64-key tile
    than the keys need, all NaN: the bits of the launch on tight buffers.  (The kernel clamps these loads; this confirms the
    clamp is what the code says.  The buffers are larger and valid: nothing here reads past an allocation.)"""
    for kind in ("rand", "point"):
        q, k, v, ks = _dev(c, kind)
        want = _launch(c, q, k, v, ks)
        qc, kc, vc = _inputs(c, kind)
        grow = lambda t, extra: torch.cat([t, _nan_like(t[:, :1].expand(-1, extra, -1, -1).contiguous())], dim=1).cuda()
        qb, kb, vb = grow(qc, 5), grow(kc, 7), grow(vc, 7)
        pad = (c.Sk + TILE - 1) // TILE * TILE
        vt = _vt(vb[:, :c.Sk], c.Sk, pad + TILE)
        vt[..., pad:] = _nan_like(vt[..., pad:].cpu()).cuda()
        assert bool((_bits(vt[..., c.Sk:pad]) == 0).all()) and not bool(torch.isfinite(vt[..., pad:].float()).any())
        got = _launch(c, qb[:, :c.Sq], kb[:, :c.Sk], None, ks, vt=vt)
        assert same_bits(got, want), kind
        assert same_bits(_launch(c, q, k, None, ks, vt=_vt(v, c.Sk)), want), kind   # vt= itself changes nothing


# ---- emu_transpose_v_bf16 on its own
@pytest.mark.parametrize("packed", (False, True), ids=("contiguous", "packed"))
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("S", (1, 63, 64, 65, 200))
def test_transpose_v(S, D, packed):
    """Exactly v.transpose zero padded to S_pad, at the minimal S_pad and with two whole extra tiles (all zero, not just the
    partial one), from contiguous and from packed-qkv sources."""
    B, H = 2, 3
    g = torch.Generator().manual_seed(900 + 2 * S + D)
    if packed:
        buf = torch.randn(B, S, 3, H, D, generator=g).to(BF16)
        v, vd = buf[:, :, 2], buf.cuda()[:, :, 2]
    else:
        v = torch.randn(B, S, H, D, generator=g).to(BF16)
        vd = v.cuda()
    assert vd.is_contiguous() != packed or S == 1
    lo = (S + TILE - 1) // TILE * TILE
    for S_pad in (lo, lo + 2 * TILE):
        want = torch.zeros(B, H, D, S_pad, dtype=BF16)
        want[..., :S] = v.permute(0, 2, 3, 1)
        got = _vt(vd, S, S_pad).cpu()
        assert same_bits(got, want), S_pad
        assert bool((_bits(got[..., S:]) == 0).all())


def test_transpose_v_refusals_write_nothing():
    ops = _ops()
    B, H, S, D = 2, 3, 70, 64
    v = torch.randn(B, S, H, 128, generator=torch.Generator().manual_seed(7)).to(BF16).cuda()
    sent = _sentinel(B * H * 128 * 256)
    vt = sent.clone().cuda()
    good = dict(sb=v.stride(0), sh=v.stride(2), ss=v.stride(1), S=S, D=D, S_pad=128)

    def call(**over):
        a = dict(good, **over)
        return _lib().emu_transpose_v_bf16(ops._p(v), a["sb"], a["sh"], a["ss"], ops._p(vt), B, H, a["S"], a["D"], a["S_pad"],
                                           ops.stream(v))

    bad = [dict(D=96), dict(S_pad=96), dict(S_pad=100), dict(S_pad=64), dict(S=129), dict(ss=good["ss"] + 4), dict(sh=good["sh"] + 4),
           dict(sb=good["sb"] + 4), dict(ss=good["ss"] + 1)]
    for over in bad:
        assert call(**over) == -22, over
        torch.cuda.synchronize()
        assert torch.equal(vt.cpu(), sent), over
    assert call() == 0
    torch.cuda.synchronize()
    n = B * H * D * 128
    want = torch.zeros(B, H, D, 128, dtype=BF16)
    want[..., :S] = v.cpu()[..., :D].permute(0, 2, 3, 1)
    assert torch.equal(vt.cpu()[:n], _bits(want).flatten()) and torch.equal(vt.cpu()[n:], sent[n:])


# ---- entry refusals of emu_flash_attn_bf16
def test_entry_refusals_write_nothing():
    ops = _ops()
    B, H, Sq, Sk, D = 2, 2, 5, 70, 128
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(B, s, H, D, generator=g).to(BF16).cuda() for s in (Sq, Sk, Sk))
    vt = _vt(v, Sk)
    sent = _sentinel(B * Sq * H * D)
    o = sent.clone().cuda().view(BF16).view(B, Sq, H, D)
    good = dict(q_sb=q.stride(0), q_sh=q.stride(2), q_ss=q.stride(1), k_sb=k.stride(0), k_sh=k.stride(2), k_ss=k.stride(1),
                o_sb=o.stride(0), o_sh=o.stride(2), o_ss=o.stride(1), Sq=Sq, Sk=Sk, Sk_pad=128, D=D)

    def call(**over):
        a = dict(good, **over)
        return _lib().emu_flash_attn_bf16(ops._p(q), a["q_sb"], a["q_sh"], a["q_ss"], ops._p(k), a["k_sb"], a["k_sh"], a["k_ss"],
                                          ops._p(vt), ops._p(o), a["o_sb"], a["o_sh"], a["o_ss"], None, B, H, a["Sq"], a["Sk"],
                                          a["Sk_pad"], a["D"], 1, _scale(D), ops.stream(q))

    bad = [dict(Sq=0), dict(Sk=0), dict(Sk_pad=96), dict(Sk_pad=100), dict(Sk_pad=64), dict(D=96)]
    bad += [{s: good[s] + 4} for s in ("q_sb", "q_sh", "q_ss", "k_sb", "k_sh", "k_ss")]
    bad += [{s: good[s] + 2} for s in ("o_sb", "o_sh", "o_ss")]
    for over in bad:
        assert call(**over) == -22, over
        torch.cuda.synchronize()
        assert torch.equal(_bits(o).flatten().cpu(), sent), over
    assert call() == 0
    torch.cuda.synchronize()
    assert same_bits(o.cpu(), ops.flash_attn(q, k, v, True, _scale(D)).cpu())
