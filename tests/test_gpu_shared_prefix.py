"""GPU: candidate ranking on a shared prefix -- the two-segment flash kernel (emu_flash_attn_prefix_bf16) against its specification
(``scoring.two_segment_attention``) and, where the key tiles coincide, bit for bit against the existing flash kernel on the
concatenated keys; ``emu_llama_set_kv_prefix`` in the engine; ``score_continuations(share_prefix=True)`` against the copying route;
``Emu.predict_ids`` and ``EmuModel.score_candidates_ids``.

Bounds.  The kernel's bound is not a constant: in the same test the EXISTING kernel runs on the concatenated keys [prefix ; own]
(``kstart`` as its left-pad mask, causal with Sk_total - Sq) and its largest error against the same fp64 reference, relative to
max |o|, is taken; the new kernel must stay within 2x that (one more bf16 rounding of the output and another tile partition where P
is no multiple of 64), with a floor of 2^-8 (one bf16 ulp of the largest output).  Measured on MI355X over all cases: see
MEASURED below.  The engine's bounds are test_gpu_scoring.py's: 1.5e-2 relative for a continuation forward, ORACLE_TOL = 0.0905 for
per-token log-probabilities against the fp32 oracle.
"""
import itertools

import pytest
import torch

from emu_amd import scoring
from tests import tiny
from tests.test_gpu_scoring import ORACLE_TOL, PREDICT_CANDS, _emu1_fixture, _oracle_lp, _t, emu1_oracle_losses, rel_err

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

# max relative error against the fp64 specification over all cases of test_kernel_against_the_specification on MI355X:
# existing kernel on the concatenated keys / two-segment kernel
# (per P in PS the pairs are 3.451e-3 / 3.096e-3, 3.420e-3 / 3.420e-3, 3.479e-3 / 3.479e-3, 3.440e-3 / 3.440e-3, 3.544e-3 / 3.544e-3: the
# two kernels differ in a handful of outputs, where P is no multiple of 64 and a query's first tile is almost wholly masked)
MEASURED = {"flash_attn on [prefix ; own]": 3.544e-3, "flash_attn_prefix": 3.544e-3}

H, D, B = 2, 128, 3
PS = (1, 63, 64, 65, 130)
SHAPES = ((1, 1), (5, 5), (33, 33), (70, 70), (4, 9))
SCALE = 1.0 / D ** 0.5


def kstarts(P):
    return sorted({0, P - 1} | ({3} if P > 3 else set()))


def kernel_inputs(P, Sq, Sk, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g).to(BF16).cuda()
    return mk(B, Sq, H, D), mk(P, H, D), mk(P, H, D), mk(B, Sk, H, D), mk(B, Sk, H, D)


def both_kernels(q, kp, vp, ko, vo, kstart):
    """(two-segment kernel, existing kernel on the concatenated keys)."""
    from emu_amd import ops
    new = ops.flash_attn_prefix(q, kp, vp, ko, vo, kstart, SCALE)
    kcat = torch.cat([kp[None].expand(B, -1, -1, -1), ko], dim=1).contiguous()
    vcat = torch.cat([vp[None].expand(B, -1, -1, -1), vo], dim=1).contiguous()
    old = ops.flash_attn(q, kcat, vcat, True, SCALE, kstart=torch.full((B,), kstart, dtype=torch.int32, device="cuda"))
    return new, old


@pytest.mark.parametrize("P", PS)
def test_kernel_against_the_specification(P):
    worst_new = worst_old = 0.0
    for (Sq, Sk), kstart in itertools.product(SHAPES, kstarts(P)):
        q, kp, vp, ko, vo = kernel_inputs(P, Sq, Sk, 1000 * P + 10 * Sq + Sk)
        new, old = both_kernels(q, kp, vp, ko, vo, kstart)
        want = scoring.two_segment_attention(*(t.double() for t in (q, kp, vp, ko, vo)), kstart, SCALE)
        top = float(want.abs().max())
        e_new = float((new.double() - want).abs().max()) / top
        e_old = float((old.double() - want).abs().max()) / top
        print(f"P={P} Sq={Sq} Sk={Sk} kstart={kstart}: existing kernel {e_old:.3e}, two-segment kernel {e_new:.3e}")
        assert e_new <= max(2 * e_old, 2.0 ** -8), (P, Sq, Sk, kstart, e_new, e_old)
        worst_new, worst_old = max(worst_new, e_new), max(worst_old, e_old)
    print(f"P={P}: worst existing {worst_old:.3e}, worst two-segment {worst_new:.3e}")


@pytest.mark.parametrize("P", (64, 128))
def test_bit_identity_where_the_tiles_coincide(P):
    """P a multiple of 64: the prefix tiles and the own tiles are the tiles the existing kernel walks over [prefix ; own]."""
    for (Sq, Sk), kstart in itertools.product(SHAPES, kstarts(P)):
        new, old = both_kernels(*kernel_inputs(P, Sq, Sk, 7000 + 1000 * P + 10 * Sq + Sk), kstart)
        assert torch.equal(new.view(torch.int16), old.view(torch.int16)), (P, Sq, Sk, kstart)


def test_result_does_not_depend_on_the_rows_around_it():
    """A row's output is the same alone and among others (another workgroup, wave and neighbours)."""
    from emu_amd import ops
    q, kp, vp, ko, vo = kernel_inputs(65, 33, 40, 5)
    full = ops.flash_attn_prefix(q, kp, vp, ko, vo, 3, SCALE)
    for b in range(B):
        alone = ops.flash_attn_prefix(q[b:b + 1].contiguous(), kp, vp, ko[b:b + 1].contiguous(), vo[b:b + 1].contiguous(), 3, SCALE)
        assert torch.equal(alone[0], full[b]), b


def test_entry_refusals_write_nothing():
    from emu_amd import ops
    from emu_amd._lib import lib
    P, Sq, Sk = 65, 5, 9
    q, kp, vp, ko, vo = kernel_inputs(P, Sq, Sk, 3)
    vtp = ops.transpose_v(vp, 1, H, P, D, 0, vp.stride(1), vp.stride(0))
    vto = ops.transpose_v(vo, B, H, Sk, D, vo.stride(0), vo.stride(2), vo.stride(1))
    o = torch.full((B, Sq, H, D), -7.0, dtype=BF16, device="cuda")
    good = dict(kstart=3, B=B, H=H, Sq=Sq, P=P, P_pad=128, Sk=Sk, Sk_pad=64, D=D)

    def call(**over):
        a = dict(good, **over)
        return lib().emu_flash_attn_prefix_bf16(
            ops._p(q), q.stride(0), q.stride(2), q.stride(1), ops._p(kp), kp.stride(1), kp.stride(0), ops._p(vtp),
            ops._p(ko), ko.stride(0), ko.stride(2), ko.stride(1), ops._p(vto), ops._p(o), o.stride(0), o.stride(2), o.stride(1),
            a["kstart"], a["B"], a["H"], a["Sq"], a["P"], a["P_pad"], a["Sk"], a["Sk_pad"], a["D"], SCALE, ops.stream(q))

    bad = [dict(D=64), dict(P=0), dict(kstart=-1), dict(kstart=P), dict(Sk=Sq - 1), dict(P_pad=96), dict(P_pad=64), dict(Sk_pad=32),
           dict(Sk=70, Sk_pad=64)]
    for over in bad:
        assert call(**over) == -22, over
        torch.cuda.synchronize()
        assert bool((o == -7).all()), over
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((o != -7).any())
    want = ops.flash_attn_prefix(q, kp, vp, ko, vo, 3, SCALE)
    assert torch.equal(o, want)


# ------------------------------------------------------------------------------------------------ the engine
@pytest.fixture(scope="module")
def tiny_model(golden_dir):
    """emu_amd.EmuModel (HIP) + oracle weights (fp32 tensors holding the same bf16 values)."""
    from emu_amd import EmuModel, TextDecoderCfg
    from oracle import emu2_ref as R
    z = tiny.load(golden_dir, "generate_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    m = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda")
    m.load_state_dict(W, strict=True)
    return m, R.bf16_round(W), tiny.oracle_cfg(v, l, vocab), z


def _prompt(S, hidden, seed):
    """One prompt of S slots, the first a left pad: random embeddings, as test_continuation_forward_on_top_of_the_cache's."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(1, S, hidden, generator=g) * 0.5).to(BF16).cuda()
    mask = torch.ones(1, S, dtype=torch.long)
    mask[0, :1] = 0
    return x, mask, g


def _both_forwards(lm, S, n=9, rows=3, s_max=256):
    """The unshared continuation forward (fan_out_kv's copies, slots S ..) and the shared one (16-slot suffix cache, slots 0 ..)."""
    Hd = lm.cfg.hidden_size
    x, mask, g = _prompt(S, Hd, 40 + S)
    cont = (torch.randn(rows, n, Hd, generator=g) * 0.5).to(BF16).cuda()
    _, kstart, pos = lm.prefill(x, mask, s_max)
    kmain, vmain = lm.kcache, lm.vcache
    ar = torch.arange(n, device="cuda", dtype=torch.int32)
    posr = (pos.expand(rows)[:, None] + ar[None]).reshape(-1).contiguous()
    ks = kstart.expand(rows).contiguous()
    lm.fan_out_kv(1, rows, S, s_max, share=False)
    unshared = cont.reshape(rows * n, Hd).contiguous().clone()
    lm.forward(unshared, rows, n, posr, (S + ar)[None].expand(rows, -1).reshape(-1).contiguous(), ks, ctx=S + n)
    lm.alloc_kv(rows, 16, zero=False, which="suffix")
    lm.set_kv_prefix(kmain, vmain, s_max, S)
    try:
        shared = cont.reshape(rows * n, Hd).contiguous().clone()
        lm.forward(shared, rows, n, posr, ar[None].expand(rows, -1).reshape(-1).contiguous(), ks, ctx=n)
    finally:
        lm.set_kv_prefix(None, None, 0, 0)
    return shared, unshared


def test_engine_forward_behind_a_prefix(tiny_model):
    lm = tiny_model[0].decoder.lm
    shared, unshared = _both_forwards(lm, 64)
    assert torch.equal(shared, unshared)                     # S = 64: the same key tiles, bit for bit
    shared, unshared = _both_forwards(lm, 70)
    e = rel_err(shared, unshared)
    print(f"S = 70: shared vs unshared continuation forward {e:.3e}")
    assert e < 1.5e-2


def test_engine_refusals_leave_the_caches_alone(tiny_model):
    from emu_amd._lib import EmuHipError
    lm = tiny_model[0].decoder.lm
    Hd, S, rows = lm.cfg.hidden_size, 64, 4
    x, mask, _ = _prompt(S, Hd, 9)
    _, kstart, pos = lm.prefill(x, mask, 256)
    kmain, vmain = lm.kcache, lm.vcache
    lm.alloc_kv(rows, 16, zero=True, which="suffix")
    lm.set_kv_prefix(kmain, vmain, 256, S)
    try:
        before = [t.clone() for t in (kmain, vmain, lm.kcache, lm.vcache)]
        one = torch.zeros(rows, Hd, dtype=BF16, device="cuda")
        z = torch.zeros(rows, dtype=torch.int32, device="cuda")
        with pytest.raises(EmuHipError, match="T > 1"):                             # a one-row step
            lm.forward(one, rows, 1, z, z, kstart.expand(rows).contiguous(), ctx=1)
        with pytest.raises(ValueError, match="KV prefix"):                          # a chunk step
            lm.forward_chunk(torch.zeros(8, Hd, dtype=BF16, device="cuda"), rows, 2, z, z, kstart.expand(rows).contiguous(), ctx=2)
        with pytest.raises(ValueError, match="KV prefix"):
            lm.set_kv_share(2, 1)
        torch.cuda.synchronize()
        for a, b in zip(before, (kmain, vmain, lm.kcache, lm.vcache)):
            assert torch.equal(a, b)
    finally:
        lm.set_kv_prefix(None, None, 0, 0)
    assert lm._kv_prefix is None


def _candidates(N, seed):
    """N candidates of 1..6 tokens, right padded (ragged masks)."""
    g = torch.Generator().manual_seed(seed)
    cand = torch.randint(3, 32000, (N, 6), generator=g)
    cmask = torch.arange(6)[None] < (1 + torch.arange(N) % 6)[:, None]
    return cand, cmask


@pytest.mark.parametrize("n_segments", (1, 2))
def test_score_continuations_shared_equals_unshared(tiny_model, n_segments):
    m, W, cfg, _ = tiny_model
    lm = m.decoder.lm
    N, S = 12, 64
    x, mask, _ = _prompt(S, lm.cfg.hidden_size, 21)
    cand, cmask = _candidates(N, 22)
    ids_before = lm.greedy_generate(x, mask, 4, min_len=0, stop_on_eos=False)
    lm.release_kv("beam")
    lp_s, counted_s = lm.score_continuations(x, mask, cand, cmask, n_segments=n_segments, share_prefix=True)
    # the caches the plan names, no N x s_max fan-out, the prefix off again
    segs = scoring.split_segments(N, n_segments)
    widths = [int(cmask[a:b].sum(dim=1).max()) for a, b in segs]
    plan = scoring.shared_prefix_plan(N, S, widths, lm.cfg.num_hidden_layers, lm.plan.heads_local, lm.cfg.head_dim, lm.kv_capacity)
    assert tuple(lm._kv_slots["suffix"][0].shape) == tuple(lm._kv_slots["suffix"][1].shape) == plan["segments"][-1]["suffix_shape"]
    assert tuple(lm._kv_slots["main"][0].shape) == plan["prefix_shape"]
    assert "beam" not in lm._kv_slots and lm._kv_prefix is None
    assert torch.equal(lm.greedy_generate(x, mask, 4, min_len=0, stop_on_eos=False), ids_before)
    lp_u, counted_u = lm.score_continuations(x, mask, cand, cmask, n_segments=n_segments)
    assert torch.equal(counted_s, counted_u) and torch.equal(counted_s.cpu(), cmask)
    assert torch.equal(lp_s, lp_u)                           # S = 64: bit for bit
    assert bool((lp_s.cpu()[~cmask] == 0).all()) and bool((lp_s.cpu()[cmask] < 0).all())


@pytest.mark.parametrize("n_segments", (1, 2))
def test_score_continuations_off_the_tile_grid_against_the_oracle(tiny_model, n_segments):
    """S = 70: the two routes walk different key tiles; both are held to the fp32 oracle and to each other."""
    m, W, cfg, _ = tiny_model
    lm = m.decoder.lm
    N, S = 12, 70
    x, mask, _ = _prompt(S, lm.cfg.hidden_size, 31)
    cand, cmask = _candidates(N, 32)
    want = _oracle_lp(W, cfg, x.cpu().expand(N, -1, -1), mask.expand(N, -1), cand.masked_fill(~cmask, -100))
    lp_s, counted_s = lm.score_continuations(x, mask, cand, cmask, n_segments=n_segments, share_prefix=True)
    lp_u, counted_u = lm.score_continuations(x, mask, cand, cmask, n_segments=n_segments)
    d_s = float((lp_s.cpu() - want)[cmask].abs().max())
    d_u = float((lp_u.cpu() - want)[cmask].abs().max())
    d_routes = float((lp_s - lp_u).abs().max())
    print(f"S = 70, {n_segments} segment(s): shared vs oracle {d_s:.4e}, unshared vs oracle {d_u:.4e}, shared vs unshared {d_routes:.4e}")
    assert torch.equal(counted_s, counted_u)
    assert d_s <= ORACLE_TOL and d_u <= ORACLE_TOL and d_routes <= ORACLE_TOL


def test_emu1_predict_ids_ranks_the_same_with_a_shared_prefix(golden_dir):
    from emu_amd.emu1 import Emu
    z, v, t5, l, vocab, W, cfg, ids, mask, img = _emu1_fixture(golden_dir)
    want, cand, counted = emu1_oracle_losses(golden_dir, PREDICT_CANDS, 1)
    m = Emu(v, l, t5, vocab=vocab, device="cuda")
    m.load_state_dict(W, strict=True)
    for n_segments in (2, 1):
        r_u, l_u = m.predict_ids(ids, mask, img.cuda(), cand.clamp(min=0), counted, n_segments=n_segments, return_losses=True)
        r_s, l_s = m.predict_ids(ids, mask, img.cuda(), cand.clamp(min=0), counted, n_segments=n_segments, return_losses=True,
                                 share_prefix=True)
        print(f"predict_ids n_segments={n_segments}: shared vs unshared losses {float((l_s - l_u).abs().max()):.3e}")
        assert r_s.tolist() == r_u.tolist()
    assert r_s[0].tolist() == torch.argsort(want).tolist()   # (n_segments = 1 is the last one run: the oracle's order)


def test_score_candidates_ids_with_an_image(tiny_model):
    m, W, cfg, z = tiny_model
    ids, mask, image = _t(z["ids1"]), _t(z["mask1"]), _t(z["image"]).cuda()
    N = 4
    cand, cmask = _candidates(N, 52)
    cand[0, :6] = _t(z["new1"]).long()[0, :6]                # one candidate is the greedy continuation
    cmask[0] = True
    lp, counted = m.score_candidates_ids(ids, mask, image, None, cand, cmask)
    assert torch.equal(counted.cpu(), cmask) and lp.shape == (N, 6) and lp.dtype == torch.float32
    # == the engine on the same embeddings, bit for bit
    S = ids.shape[1]
    x = m._prompt_embeds(ids, image, m.n_query).view(1, S, -1)
    lp_e, counted_e = m.decoder.lm.score_continuations(x, mask, cand, cmask)
    assert torch.equal(lp, lp_e) and torch.equal(counted, counted_e)
    # ~ score_ids on the prompt repeated N times
    rep = m.score_ids(ids.expand(N, -1).contiguous(), mask.expand(N, -1).contiguous(), image.expand(N, *image.shape[1:]).contiguous(),
                      None, cand, cmask, via="prefill")
    d = float((rep["lp"] - lp)[cmask.cuda()].abs().max())
    lp_s, _ = m.score_candidates_ids(ids, mask, image, None, cand, cmask, share_prefix=True)
    d_s = float((rep["lp"] - lp_s)[cmask.cuda()].abs().max())
    print(f"score_candidates_ids vs score_ids on N copies: {d:.4e} (share_prefix: {d_s:.4e})")
    assert d <= ORACLE_TOL and d_s <= ORACLE_TOL
