"""GPU: the kernels of contrastive search (emu_amd/csrc/contrastive.hip) through the C ABI on synthetic data, against their
specification ``emu_amd/sampling.py`` (``contrastive_reference_candidates`` / ``contrastive_reference_select``) in fp64."""
import itertools

import pytest
import torch

from emu_amd import _lib, ops, sampling
from tests import tiny

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda"
CHUNK = _lib.CONTRASTIVE_CHUNK_ROWS
P_TOL = 1e-5               # the project's bound for the blocked softmax sums (test_gpu_sampler.test_kept_set_and_probabilities)


def cos_tol(H: int) -> float:
    """The kernel's dot product of a unit context row with a candidate row is, per lane, 4 * ceil(H / 256) sequential fp32
    multiply-adds, then the 6 levels of the wave tree; the context row's norm (it arrives normalised, rounded to fp32), the
    candidate's inverse norm (an fp64 sum rounded to fp32) and the final multiplication add one rounding each.  Every rounding is
    relative 2^-24 on a partial sum bounded by sum |a_i b_i| <= 1 for unit vectors."""
    return (4 * ((H + 255) // 256) + 6 + 3) * 2.0 ** -24


COS_TOL = cos_tol(6656)


def test_cos_tol_is_small():
    assert COS_TOL < 1e-4 and cos_tol(256) < COS_TOL


def _stream():
    return ops.stream(torch.device(DEV))


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32).to(DEV)


# ------------------------------------------------------------------------------------------------------------------ pick
def _pick(lg, V, B, k, L, sel, hist, step, penalty, eos, min_len):
    ids = torch.full((B * k,), -7, dtype=torch.int32, device=DEV)
    p = torch.full((B * k,), -7.0, dtype=torch.float32, device=DEV)
    rc = _lib.lib().emu_contrastive_pick_bf16(lg.data_ptr(), lg.stride(0), V, B, k, L, ops._p(sel), ops._p(hist),
                                              hist.shape[1] if hist is not None else 0, step.data_ptr(), penalty, eos, min_len,
                                              ids.data_ptr(), p.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, ids.cpu().view(B, k), p.cpu().view(B, k)


@pytest.mark.parametrize("V", [97, 1000, 4099, 32274])
def test_pick_equals_the_spec(V):
    g = torch.Generator().manual_seed(V)
    L, worst = 4, 0.0
    for B, k, use_sel, step, pad in itertools.product((1, 3), (1, 2, 8), (False, True), (1, 3), (0, 3)):
        rows = B * k
        x = (2.0 * torch.randn(rows, V, generator=g)).to(BF16)
        planted = torch.stack([torch.randperm(V, generator=g)[:k + 1] for _ in range(rows)])
        vals = (24.0 - 0.25 * torch.arange(k + 1, dtype=torch.float32)).to(BF16)          # exact in bf16 (spacing 0.125 there)
        x.scatter_(1, planted, vals[None].expand(rows, -1).contiguous())
        sel = torch.randint(0, k, (B,), generator=g) if use_sel else torch.zeros(B, dtype=torch.int64)
        src = torch.arange(B) * k + sel
        # history: the row's best token (the penalty 1.4 sends 24 to 17.1: from first to last of the planted) and ids
        # that are not planted
        hist = torch.empty(L, B, dtype=torch.int64)
        for b in range(B):
            free = torch.ones(V, dtype=torch.bool)
            free[planted[src[b]]] = False
            pool = free.nonzero()[:, 0]
            hist[:, b] = pool[torch.randint(0, pool.numel(), (L,), generator=g)]
        hist[0] = planted[src, 0]
        eos, min_len = int(planted[src[0], 1]), 2                                          # suppressed while step < 2: step 1, not step 3
        buf = torch.zeros(rows, V + pad, dtype=BF16)
        buf[:, :V] = x
        lg = buf.to(DEV)[:, :V]
        sel_d, hist_d, step_d = (_i32(sel) if use_sel else None), _i32(hist), _i32([step])
        rc, ids, p = _pick(lg, V, B, k, L, sel_d, hist_d, step_d, 1.4, eos, min_len)
        assert rc == 0
        hrows = hist[:step].t()
        s = sampling.reference_scores(x[src], hrows, 1.4, eos if step < min_len else None)
        top = torch.sort(s, dim=-1, descending=True)[0][:, :k + 1]
        assert float((top[:, :-1] - top[:, 1:]).min()) >= 0.25                             # the inputs: no fp32 effect decides
        want_ids, want_p = sampling.contrastive_reference_candidates(x[src], hrows, 1.4, eos, step < min_len, k, torch.float64)
        assert torch.equal(ids.long(), want_ids), (B, k, use_sel, step, pad)
        err = float((p.double() - want_p).abs().max())
        worst = max(worst, err)
        assert err <= P_TOL, (B, k, use_sel, step, pad, err)
        if step < min_len:
            assert eos not in ids[0].tolist() or V <= k
    print(f"V {V}: largest |p - p64| {worst:.3g}")


def test_pick_ties_across_the_kth_place_go_to_the_lower_id():
    V, k = 1000, 4
    x = torch.randn(2, V, generator=torch.Generator().manual_seed(1)).to(BF16)
    x[0, 700], x[0, 20] = 9.0, 8.0
    x[0, [910, 33, 512, 47]] = 7.0                           # four equal logits for the places 3 and 4: 33 and 47
    x[1, [5, 999, 0]] = 6.0                                  # ties from the top, the first and the last id among them
    x[1, 400] = 5.5
    step0 = _i32([0])
    want_ids, want_p = sampling.contrastive_reference_candidates(x, k=k, dtype=torch.float64)
    assert want_ids.tolist() == [[700, 20, 33, 47], [0, 5, 999, 400]]
    lg = torch.zeros(8, V, dtype=BF16)                       # prompt b reads row b * k of the [B * k, V] matrix
    lg[0], lg[4] = x[0], x[1]
    rc, ids, p = _pick(lg.to(DEV), V, 2, k, 4, None, None, step0, 1.0, -1, 0)
    assert rc == 0 and torch.equal(ids.long(), want_ids)
    assert float((p.double() - want_p).abs().max()) <= P_TOL and float(p[0, 2]) == float(p[0, 3])


def test_pick_refusals_write_nothing():
    V = 1000
    x = torch.randn(9, V).to(BF16).to(DEV)
    step = _i32([0])
    big = torch.zeros(1, _lib.SAMPLE_MAX_VOCAB + 1, dtype=BF16, device=DEV)
    for lg, v, k in ((x, V, 9), (big, _lib.SAMPLE_MAX_VOCAB + 1, 2), (x, 3, 4)):
        rc, ids, p = _pick(lg, v, 1, k, 4, None, None, step, 1.0, -1, 0)
        assert rc == -22 and bool((ids == -7).all()) and bool((p == -7).all())
    ids = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    rc = _lib.lib().emu_contrastive_pick_bf16(x.data_ptr(), V, V, 1, 2, 4, None, None, 0, step.data_ptr(), 1.0, -1, 0, ids.data_ptr(), None,
                                              _stream())
    torch.cuda.synchronize()
    assert rc == -22 and bool((ids == -7).all())
    # beyond the length limit the launch does nothing
    step4 = _i32([4])
    rc, ids, p = _pick(x, V, 1, 2, 4, None, None, step4, 1.0, -1, 0)
    assert rc == 0 and bool((ids == -7).all())


# ------------------------------------------------------------------------------------------------------------------ score
class Score:
    """One call of emu_contrastive_score on host-made inputs; the outputs back on the host."""

    def __init__(self, ctx_n, cand, cand_ids, p, kstart, S, step, L, alpha, eos=-1, pad=32000, unfinished=None, k_arg=None,
                 ws_short=0):
        B, Lc, H = ctx_n.shape
        k = cand.shape[1]
        self.ctx = ctx_n.to(DEV).contiguous()
        cd = cand.to(BF16).to(DEV).contiguous()
        ci, pp = _i32(cand_ids).contiguous(), p.float().to(DEV).contiguous()
        self.out = torch.full((L, B), -7, dtype=torch.int32, device=DEV)
        self.unf = _i32(torch.ones(B) if unfinished is None else unfinished)
        self.sel = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        self.pen = torch.full((B, k), -7.0, dtype=torch.float32, device=DEV)
        ws = torch.empty(_lib.lib().emu_contrastive_workspace_bytes(B, k, Lc) - ws_short, dtype=torch.uint8, device=DEV)
        ks_d, step_d = _i32(kstart), _i32([step])
        self.rc = _lib.lib().emu_contrastive_score(self.ctx.data_ptr(), cd.data_ptr(), ci.data_ptr(), pp.data_ptr(), ks_d.data_ptr(),
                                                   step_d.data_ptr(), B, k_arg or k, H, S, L, Lc, alpha, 1.0 - alpha, eos, pad,
                                                   self.out.data_ptr(), self.unf.data_ptr(), self.sel.data_ptr(), self.pen.data_ptr(),
                                                   ws.data_ptr(), ws.numel(), _stream())
        torch.cuda.synchronize()
        self.ctx, self.out, self.unf, self.sel, self.pen = (t.cpu() for t in (self.ctx, self.out, self.unf, self.sel, self.pen))

    def bytes(self):
        return [t.numpy().tobytes() for t in (self.ctx, self.out, self.unf, self.sel, self.pen)]


GARBAGE = 1.0e30
L_NEW = 4


def _context(B, H, rows, g):
    """Unit rows in fp64, rounded to fp32: what the loop keeps in ctx_n."""
    c = torch.randn(B, rows, H, generator=g, dtype=torch.float64)
    return (c / c.norm(dim=2, keepdim=True)).float()


def _candidates(ctx_n, target, k, g):
    """Candidate j of prompt b = cos_j * (context row target[b]) + sin_j * (unit noise), at some scale, as bf16: cosines near
    0.1 / 0.5 / 0.9 with the target row."""
    B, _, H = ctx_n.shape
    cosv = torch.tensor([0.9, 0.1, 0.5, 0.3, 0.7, 0.2, 0.8, 0.4], dtype=torch.float64)[:k]
    n = torch.randn(B, k, H, generator=g, dtype=torch.float64)
    n = n / n.norm(dim=2, keepdim=True)
    t = ctx_n[torch.arange(B), target].double()[:, None, :]
    return ((cosv[None, :, None] * t + (1 - cosv ** 2).sqrt()[None, :, None] * n) * 37.5).to(BF16)


def _scenario(ctx_base, g, k, length, kstart, where, alpha=0.6):
    """Inputs for one call: the current length is ``length`` = S + step; the row the candidates are built from sits at ``where``."""
    B, _, H = ctx_base.shape
    step = min(2, length - 1)
    S = length - step
    Lc = S + L_NEW
    ctx = ctx_base[:, :Lc].clone()
    ctx[:, length:] = GARBAGE                                # rows beyond the current length: never to be read
    ks = torch.tensor([kstart, 0, kstart][:B])
    target = {"first": ks.clone(), "last": torch.full((B,), length - 1), "before": (ks - 1).clamp(min=0),
              "beyond": torch.full((B,), min(length + 1, Lc - 1))}[where]
    if where == "beyond":                                    # built from a row that then disappears under the garbage
        cand = _candidates(ctx_base[:, :Lc], target, k, g)
    else:
        cand = _candidates(ctx, target, k, g)
    valid = torch.arange(length)[None, :] >= ks[:, None]     # the rows [kstart, length)
    safe = ctx[:, :length]
    pen64, _ = sampling.contrastive_reference_select(safe, valid, cand.float().view(B, k, H), torch.zeros(B, k), alpha, torch.float64)
    # p so that the scores are 0.06 apart in a random order
    rank = torch.stack([torch.randperm(k, generator=g) for _ in range(B)]).double()
    p = ((0.3 - 0.06 * rank + alpha * pen64) / (1.0 - alpha)).float()
    pen64, sel64 = sampling.contrastive_reference_select(safe, valid, cand.float().view(B, k, H), p, alpha, torch.float64)
    sc = (1.0 - alpha) * p.double() - alpha * pen64
    top2 = torch.topk(sc, min(2, k), dim=1)[0]
    assert k == 1 or float((top2[:, 0] - top2[:, 1]).min()) >= 0.05
    ids = torch.randint(0, 30000, (B, k), generator=g)
    return dict(ctx=ctx, cand=cand, ids=ids, p=p, ks=ks, S=S, step=step, length=length, pen64=pen64, sel64=sel64, valid=valid)


def _check(sc, r, H, k):
    B = sc["ctx"].shape[0]
    assert r.rc == 0
    err = float((r.pen.double() - sc["pen64"]).abs().max())
    assert err <= cos_tol(H), err
    assert torch.equal(r.sel.long(), sc["sel64"])
    ar = torch.arange(B)
    assert torch.equal(r.out[sc["step"]].long(), sc["ids"][ar, sc["sel64"]])
    kept = sc["cand"].float().view(B, k, H)[ar, sc["sel64"]].double()
    want = kept / kept.norm(dim=1, keepdim=True)
    assert float((r.ctx[:, sc["length"]].double() - want).abs().max()) <= 4 * 2.0 ** -24
    before = sc["ctx"].clone()
    before[:, sc["length"]] = r.ctx[:, sc["length"]]
    assert before.numpy().tobytes() == r.ctx.numpy().tobytes()          # every other row bit for bit
    return err


@pytest.mark.parametrize("H", [256, 1000, 6656])
def test_score_equals_the_spec(H):
    g = torch.Generator().manual_seed(H)
    worst, n = 0.0, 0
    for B in (1, 3):
        base = _context(B, H, CHUNK + 1 + 64 + L_NEW + 2, g)
        for k in (2, 4, 8):
            for length, kstart, where in itertools.product((1, 63, 64, 65, CHUNK + 1), (0, 5), ("first", "last", "before", "beyond")):
                if kstart >= length or (where == "before" and kstart == 0):
                    continue
                n += 1
                sc = _scenario(base, g, k, length, kstart, where)
                if where == "before":                        # the row that must be ignored would have changed the answer
                    pen_all, _ = sampling.contrastive_reference_select(sc["ctx"][:, :length], torch.ones(B, length, dtype=torch.bool),
                                                                       sc["cand"].float().view(B, k, H), sc["p"], 0.6, torch.float64)
                    assert float((pen_all[0] - sc["pen64"][0]).abs().max()) > 0.3
                r = Score(sc["ctx"], sc["cand"].view(B, k, H), sc["ids"], sc["p"], sc["ks"], sc["S"], sc["step"], L_NEW, 0.6)
                worst = max(worst, _check(sc, r, H, k))
    print(f"H {H}: {n} calls, largest |pen - pen64| {worst:.3g} (bound {cos_tol(H):.3g})")


def test_score_identical_candidates_flags_and_determinism():
    H, k, B = 1000, 4, 3
    g = torch.Generator().manual_seed(7)
    base = _context(B, H, 40, g)
    sc = _scenario(base, g, k, 21, 5, "last")
    cand = sc["cand"].view(B, k, H).clone()
    cand[:, 2] = cand[:, 1]                                  # bit-identical candidates with the same p, far ahead of the others
    p = sc["p"].clone()
    p[:, 1] = p[:, 2] = 5.0
    eos = int(sc["ids"][2, 1])                               # prompt 2 will select it; prompt 1 has finished before
    unf = torch.tensor([1, 0, 1])
    run = lambda: Score(sc["ctx"], cand, sc["ids"], p, sc["ks"], sc["S"], sc["step"], L_NEW, 0.6, eos=eos, pad=31999, unfinished=unf)
    r = run()
    assert r.rc == 0 and r.sel.tolist() == [1, -7, 1]
    assert float(r.pen[0, 1]) == float(r.pen[0, 2]) and float(r.pen[2, 1]) == float(r.pen[2, 2])
    assert r.out[sc["step"]].tolist() == [int(sc["ids"][0, 1]), 31999, eos]
    assert r.unf.tolist() == [1, 0, 0]
    # nothing else of the finished prompt is written
    assert bool((r.pen[1] == -7).all()) and torch.equal(r.ctx[1], sc["ctx"][1])
    assert bool((r.out[torch.arange(L_NEW) != sc["step"]] == -7).all())
    assert run().bytes() == r.bytes()


def test_score_refusals_write_nothing():
    H, k, B = 256, 8, 1
    g = torch.Generator().manual_seed(8)
    base = _context(B, H, 40, g)
    sc = _scenario(base, g, k, 9, 0, "first")
    cand9 = torch.cat((sc["cand"].view(B, k, H), sc["cand"].view(B, k, H)[:, :1]), dim=1)
    p9, ids9 = torch.cat((sc["p"], sc["p"][:, :1]), dim=1), torch.cat((sc["ids"], sc["ids"][:, :1]), dim=1)
    for kw in (dict(cand=cand9, p=p9, ids=ids9), dict(ws_short=4)):
        r = Score(sc["ctx"], kw.get("cand", sc["cand"].view(B, k, H)), kw.get("ids", sc["ids"]), kw.get("p", sc["p"]), sc["ks"], sc["S"],
                  sc["step"], L_NEW, 0.6, ws_short=kw.get("ws_short", 0))
        assert r.rc == -22
        assert bool((r.out == -7).all()) and bool((r.sel == -7).all()) and bool((r.pen == -7).all()) and torch.equal(r.ctx, sc["ctx"])
    # beyond the length limit the launches do nothing
    r = Score(sc["ctx"], sc["cand"].view(B, k, H), sc["ids"], sc["p"], sc["ks"], sc["S"], L_NEW, L_NEW, 0.6)
    assert r.rc == 0 and bool((r.out == -7).all()) and torch.equal(r.ctx, sc["ctx"])


# ------------------------------------------------------------------------------------------------------------------ keep
def test_keep_copies_one_slot_to_the_siblings(golden_dir):
    from emu_amd import EmuModel, TextDecoderCfg
    z = tiny.load(golden_dir, "generate_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    m = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda")
    m.load_state_dict(W, strict=True)
    lm = m.decoder.lm
    B, k, slot0, L = 2, 4, 11, 6
    lm.alloc_kv(B * k, 256, zero=False, which="beam")
    g = torch.Generator().manual_seed(9)
    lm.kcache.copy_(torch.randn(lm.kcache.shape, generator=g).to(BF16))
    lm.vcache.copy_(torch.randn(lm.vcache.shape, generator=g).to(BF16))
    ar = torch.arange(B, device=DEV)
    for step, sel in ((0, [2, 0]), (L - 1, [3, 1])):
        sel_d = _i32(sel)
        kc, vc = lm.kcache.clone(), lm.vcache.clone()
        src = (ar * k + sel_d.long()).repeat_interleave(k)
        kc[:, :, :, slot0 + step] = kc[:, src, :, slot0 + step]
        vc[:, :, :, slot0 + step] = vc[:, src, :, slot0 + step]
        assert not torch.equal(kc, lm.kcache)
        step_d = _i32([step])
        rc = _lib.lib().emu_llama_contrastive_keep_kv(lm.handle, sel_d.data_ptr(), step_d.data_ptr(), k, slot0, L, _stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert torch.equal(lm.kcache, kc) and torch.equal(lm.vcache, vc)       # the slot of every group, and no other byte
    before = lm.kcache.clone()
    sel_d, s0, sL = _i32([1, 1]), _i32([0]), _i32([L])
    K = _lib.lib().emu_llama_contrastive_keep_kv
    assert K(lm.handle, sel_d.data_ptr(), sL.data_ptr(), k, slot0, L, _stream()) == 0          # beyond the length limit: nothing moves
    assert K(lm.handle, sel_d.data_ptr(), s0.data_ptr(), 9, slot0, L, _stream()) == -22
    assert K(lm.handle, sel_d.data_ptr(), s0.data_ptr(), 3, slot0, L, _stream()) == -22       # 8 rows are no groups of 3
    assert K(lm.handle, sel_d.data_ptr(), s0.data_ptr(), k, 252, L, _stream()) == -22         # slots beyond the cache
    assert K(lm.handle, None, s0.data_ptr(), k, slot0, L, _stream()) == -22
    torch.cuda.synchronize()
    assert torch.equal(lm.kcache, before)


def test_advance_follows_the_counter():
    step, pos, slot = _i32([2]), torch.zeros(6, dtype=torch.int32, device=DEV), torch.zeros(6, dtype=torch.int32, device=DEV)
    pos0 = _i32([5, 5, 5, 9, 9, 9])
    A = _lib.lib().emu_contrastive_advance
    assert A(step.data_ptr(), pos.data_ptr(), slot.data_ptr(), pos0.data_ptr(), 20, 6, 4, 0, _stream()) == 0
    assert A(step.data_ptr(), None, None, None, 20, 6, 4, 1, _stream()) == 0
    assert pos.tolist() == [7, 7, 7, 11, 11, 11] and slot.tolist() == [22] * 6 and step.tolist() == [3]
    assert A(step.data_ptr(), None, None, None, 20, 6, 4, 1, _stream()) == 0
    assert A(step.data_ptr(), None, None, None, 20, 6, 4, 1, _stream()) == 0        # at the limit: nothing moves
    assert A(step.data_ptr(), pos.data_ptr(), slot.data_ptr(), pos0.data_ptr(), 20, 6, 4, 0, _stream()) == 0
    assert step.tolist() == [4] and slot.tolist() == [22] * 6


@pytest.mark.parametrize("entry, bias", [("emu_contrastive_advance", 0), ("emu_beam_advance", -1)])
def test_the_shared_advance_through_both_entries(entry, bias):
    """One kernel behind both exported names: the contrastive entry counts from the step counter itself, the beam entry from one
    before it.  70 rows = one past the 64-lane stride, so the row loop takes a second trip.  Integers against integers."""
    rows, slot0, L = 70, 20, 4
    host0 = [5] * 33 + [9] * 37
    step, pos0 = _i32([2]), _i32(host0)
    pos, slot = torch.full((rows,), -7, dtype=torch.int32, device=DEV), torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    A = getattr(_lib.lib(), entry)
    p = lambda t: t.data_ptr()
    assert A(p(step), p(pos), p(slot), p(pos0), slot0, rows, L, 0, _stream()) == 0
    assert slot.tolist() == [slot0 + 2 + bias] * rows and pos.tolist() == [v + 2 + bias for v in host0] and step.tolist() == [2]
    for want in (3, 4, 4):                                                    # phase 1: counter + 1, up to the limit and no further
        assert A(p(step), None, None, None, slot0, rows, L, 1, _stream()) == 0
        assert step.tolist() == [want]
    pos.fill_(-7); slot.fill_(-7)
    assert A(p(step), p(pos), p(slot), p(pos0), slot0, rows, L, 0, _stream()) == 0          # phase 0 at the limit: writes nothing
    assert pos.tolist() == [-7] * rows and slot.tolist() == [-7] * rows and step.tolist() == [4]
    for args in ((None, p(slot), p(pos0)), (p(pos), None, p(pos0)), (p(pos), p(slot), None)):
        assert A(p(step), *args, slot0, rows, L, 0, _stream()) == -22
    assert A(p(step), p(pos), p(slot), p(pos0), slot0, 0, L, 0, _stream()) == -22
    assert A(p(step), None, None, None, slot0, 0, L, 1, _stream()) == -22
