"""GPU: scoring given text -- the kernel (emu_token_logprob_bf16) against its specification (emu_amd/scoring.py), the continuation
forward, the teacher-forced step, ``LlamaEngine.score`` against the oracle, ``Emu.predict_ids`` and ``EmuModel.score_ids``.

Measured bounds (profiles/scoring.md):

* Kernel.  On the inputs of ``kernel_case`` the fp32 specification (``dtype=float32``, CPU) deviates from the fp64 one by at most
  SPEC32_DEV = {lp 2.6e-6, lse 2.6e-6, kl 3.8e-6} (lp and lse absolute -- the largest are the +-60 rows', whose log-sum-exp of ~ 74
  has an fp32 ulp of 7.6e-6 --, kl relative to max(1, |kl|)); the largest over all cases is the figure, because one case's deviation
  can be small by luck.  The kernel is allowed 4x that: its sums run in another order.  Measured on MI355X against the fp64
  specification: lp 2.6e-6, lse 2.6e-6, kl 3.6e-6.
* Engine.  Per-token lp of ``score`` against the fp32 oracle on the tiny fixture (the bf16 engine against fp32 arithmetic on the
  same bf16 weights): measured 0.0229 (decode route) and 0.0452 (prefill route), the two routes 0.0311 apart; the bound ORACLE_TOL
  is twice the larger, 0.0905.
"""
import functools

import numpy as np
import pytest
import torch

from emu_amd import scoring
from tests import tiny

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
INF = float("inf")

# fp32 spec against fp64 spec on kernel_case's inputs, CPU (see the module docstring); the kernel gets 4x
SPEC32_DEV = {"lp": 2.6e-6, "lse": 2.6e-6, "kl": 3.8e-6}
# score() against the fp32 oracle on generate_tiny.npz: measured 0.0452 on MI355X (prefill route; decode 0.0229), bound = 2x
ORACLE_TOL = 0.0905


def _t(a):
    return torch.from_numpy(np.asarray(a))


def rel_err(got, want):
    got, want = got.float().cpu(), want.float().cpu()
    return float((got - want).norm() / want.norm().clamp_min(1e-12))


# ------------------------------------------------------------------------------------------------ 1. the kernel
VOCABS = (50, 1027, 32274)
KINDS = ("normal", "neg_inf", "equal", "pm60")


@functools.lru_cache(maxsize=None)
def kernel_case(V, kind):
    """Three rows of bf16 logits and three rows of DISTINCT reference logits (CPU), with their fp64 and fp32 specifications for the
    two target vectors of three rows; computed once and shared."""
    g = torch.Generator().manual_seed(V * 7 + KINDS.index(kind))
    x = (torch.randn(3, V, generator=g) * 3).to(BF16)
    r = (x.float() + torch.randn(3, V, generator=g)).to(BF16)
    if kind == "neg_inf":
        x[:, ::7] = -INF                                     # the target 0 among them: lp = -inf; kl = +inf against a finite r
        x[1, V // 2:] = -INF
        r[2, ::7] = -INF                                     # row 2: the reference rules out the same tokens: finite kl
    elif kind == "equal":
        x[:] = 1.5
        r[1] = -2.0
    elif kind == "pm60":
        x[0] += 60.0
        x[1] -= 60.0
        x[2, ::2] += 60.0
        x[2, 1::2] -= 60.0
        r[0] -= 60.0
        r[2, ::3] += 60.0
    targets = (torch.tensor([0, V - 1, -100]), torch.tensor([V, V // 2, 0]))
    spec = {}
    for ti, t in enumerate(targets):
        for dt in (torch.float64, torch.float32):
            spec[ti, dt] = scoring.reference_logprob(x, t, ref_logits=r, dtype=dt)
    return x, r, targets, spec


def _dev(got, want, key):
    """Largest deviation -- absolute for lp and lse, for kl relative to max(1, |kl|): the +-60 rows are 40 to 60 nats from their
    references --; infinities must coincide."""
    got, want = got.double().cpu(), want.double().cpu()
    fin = torch.isfinite(want)
    assert torch.equal(got[~fin], want[~fin]), (got, want)
    d = (got[fin] - want[fin]).abs()
    if key == "kl":
        d = d / want[fin].abs().clamp_min(1.0)
    return float(d.max()) if bool(fin.any()) else 0.0


def spec32_deviation(V, kind):
    """What SPEC32_DEV records: the fp32 specification against the fp64 one on this case's inputs."""
    _, _, targets, spec = kernel_case(V, kind)
    out = {"lp": 0.0, "lse": 0.0, "kl": 0.0}
    for ti in range(len(targets)):
        for k in out:
            out[k] = max(out[k], _dev(spec[ti, torch.float32][k], spec[ti, torch.float64][k], k))
    return out


def _place(t, offset, ld):
    """The rows of ``t`` [rows, V] on the device, ``ld`` elements apart, the base ``offset`` elements into a fresh allocation."""
    rows, V = t.shape
    buf = torch.full((offset + rows * ld + 8,), 7.0, dtype=BF16, device="cuda")
    view = buf[offset:offset + rows * ld].view(rows, ld)[:, :V]
    view.copy_(t)
    return view


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V", VOCABS)
def test_kernel_against_the_specification(V, kind):
    from emu_amd import ops
    x, r, targets, spec = kernel_case(V, kind)
    s32 = spec32_deviation(V, kind)
    worst = {"lp": 0.0, "lse": 0.0, "kl": 0.0}
    for rows in (1, 3):
        for off_x, ld_x, off_r, ld_r in ((0, V, 0, V), (1, V + 9, 0, V + 8), (0, V + 16, 1, V + 3)):
            dx, dr = _place(x[:rows], off_x, ld_x), _place(r[:rows], off_r, ld_r)
            for ti, t in enumerate(targets):
                want = spec[ti, torch.float64]
                tg = t[:rows].to(device="cuda", dtype=torch.int32)
                got = ops.token_logprob(dx, tg, ref_logits=dr)
                assert got["top1"].cpu().tolist() == want["top1"][:rows].tolist()
                assert got["agree"].cpu().bool().tolist() == want["agree"][:rows].tolist()
                counted = [0 <= int(v) < V for v in t[:rows]]
                assert counted == want["counted"][:rows].tolist()
                assert [float(v) == 0.0 for v, c in zip(got["lp"].cpu(), counted) if not c] == [True] * counted.count(False)
                for k in worst:
                    worst[k] = max(worst[k], _dev(got[k], want[k][:rows], k))
                # without a reference: the same lp / lse / top1 bit for bit, kl and agree absent
                alone = ops.token_logprob(dx, tg)
                assert set(alone) == {"lp", "lse", "top1"}
                for k in alone:
                    assert torch.equal(alone[k], got[k]), k
                # identical rows: kl == 0 and agree == 1, exactly
                same = ops.token_logprob(dx, tg, ref_logits=_place(x[:rows], off_r, ld_r))
                assert same["kl"].cpu().tolist() == [0.0] * rows and same["agree"].cpu().tolist() == [1] * rows
                # two launches on the same inputs are bit-identical
                again = ops.token_logprob(dx, tg, ref_logits=dr)
                for k in got:
                    assert torch.equal(again[k].view(torch.int32), got[k].view(torch.int32)), k
    print(f"kernel V={V} {kind}: fp32 spec vs fp64 {s32}, kernel vs fp64 {worst}")
    for k in worst:
        assert s32[k] <= SPEC32_DEV[k], (k, s32)             # the recorded figure covers this case
        assert worst[k] <= 4 * SPEC32_DEV[k], (k, worst, SPEC32_DEV)


def test_kernel_reads_step_and_targets_from_the_device():
    from emu_amd import ops
    V = 1027
    x, _, _, _ = kernel_case(V, "normal")
    dx = x.cuda()
    tg = torch.tensor([[0, 5, -100], [V - 1, 9, 3], [7, V, 1]], dtype=torch.int32, device="cuda")
    out = {k: torch.full((3, 3), -7, dtype=dt, device="cuda") for k, dt in (("lp", torch.float32), ("lse", torch.float32),
                                                                            ("top1", torch.int32))}
    step = torch.tensor([1], dtype=torch.int32, device="cuda")
    ops.token_logprob(dx, tg, step_dev=step, out=out)
    want = ops.token_logprob(dx, tg[1].contiguous())
    for k in out:
        assert torch.equal(out[k][1], want[k]) and bool((out[k][0] == -7).all()) and bool((out[k][2] == -7).all()), k
    # every output pointer may be NULL
    only = {"lp": torch.zeros(3, dtype=torch.float32, device="cuda")}
    ops.token_logprob(dx, tg[1].contiguous(), out=only)
    assert torch.equal(only["lp"], want["lp"])


def test_kernel_refusals_write_nothing():
    from emu_amd import ops
    from emu_amd._lib import lib
    V = 50
    x = kernel_case(V, "normal")[0].cuda()
    tg = torch.zeros(3, dtype=torch.int32, device="cuda")
    poison = {k: torch.full((3,), -7, dtype=dt, device="cuda") for k, dt in
              (("lp", torch.float32), ("lse", torch.float32), ("top1", torch.int32), ("kl", torch.float32), ("agree", torch.int32))}

    def call(logits=x.data_ptr(), ld=V, rows=3, vocab=V, targets=tg.data_ptr()):
        return lib().emu_token_logprob_bf16(logits, ld, rows, vocab, targets, 3, None, x.data_ptr(), V, poison["lp"].data_ptr(),
                                            poison["lse"].data_ptr(), poison["top1"].data_ptr(), poison["kl"].data_ptr(),
                                            poison["agree"].data_ptr(), 3, ops.stream(x))
    assert call(logits=None) == -22
    assert call(targets=None) == -22
    assert call(ld=V - 1) == -22
    assert call(rows=0) == -22
    assert call(vocab=0) == -22
    torch.cuda.synchronize()
    for k, v in poison.items():
        assert bool((v == -7).all()), k
    assert call() == 0
    torch.cuda.synchronize()
    assert all(bool((v != -7).all()) for v in poison.values())


# ------------------------------------------------------------------------------------------------ the tiny models
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


def test_continuation_forward_on_top_of_the_cache(tiny_model):
    """prefill(S = 24), then ONE forward of 9 rows per batch element on top == rows 24..32 of prefill(S = 33); B = 2, one row
    left-padded.  The bound is test_decode_matches_prefill's for one row."""
    m, W, cfg, _ = tiny_model
    lm = m.decoder.lm
    g = torch.Generator().manual_seed(5)
    S, n, H = 24, 9, cfg.llama.hidden
    x = (torch.randn(2, S + n, H, generator=g) * 0.5).to(BF16).cuda()
    mask = torch.ones(2, S + n, dtype=torch.long)
    mask[1, :5] = 0
    full, _, _ = lm.prefill(x, mask)
    want = full[:, S:, :].clone()
    _, kstart, pos = lm.prefill(x[:, :S].contiguous(), mask[:, :S])
    hid = x[:, S:, :].reshape(2 * n, H).contiguous().clone()
    ar = torch.arange(n, device="cuda", dtype=torch.int32)
    lm.forward(hid, 2, n, (pos[:, None] + ar[None]).reshape(-1).contiguous(), (S + ar)[None].expand(2, -1).reshape(-1).contiguous(),
               kstart, ctx=S + n)
    e = rel_err(hid.view(2, n, H), want)
    print(f"continuation forward vs prefill rows: {e:.3e}")
    assert e < 1.5e-2


def _text_prompts(z, B):
    """B left-padded text-only prompts from the fixture's ragged pair (B = 3: a third row, the first with one token changed)."""
    ids, mask = _t(z["ids2"]).clone(), _t(z["mask2"]).clone()
    if B == 1:
        return ids[:1], mask[:1]
    if B == 3:
        extra = ids[:1].clone()
        extra[0, -1] = 523
        return torch.cat([ids, extra]), torch.cat([mask, mask[:1]])
    return ids, mask


@pytest.mark.parametrize("B", (1, 3))
def test_decode_route_exact_invariants(tiny_model, B):
    from emu_amd import ops
    m, W, cfg, z = tiny_model
    lm = m.decoder.lm
    ids, mask = _text_prompts(z, B)
    S, T = ids.shape[1], 6
    x = m._prompt_embeds(ids, None, m.n_query).view(B, S, -1)
    new = lm.greedy_generate(x, mask, T, min_len=0, stop_on_eos=False)              # raw arg-max ids, nothing suppressed
    cmask = torch.ones(B, T, dtype=torch.bool)
    if B == 3:
        cmask[1, 4:] = False                                                         # one row ends early on an ignored target
    got = lm.score(x, mask, new, cmask, via="decode")
    fed_ok = torch.ones(B, T, dtype=torch.bool)                                      # rows whose input was the real token
    if B == 3:
        fed_ok[1, 5:] = False
    assert torch.equal(got["top1"].cpu()[fed_ok], new.cpu()[fed_ok])
    assert torch.equal(got["counted"].cpu(), cmask)
    assert bool((got["lp"].cpu()[~cmask] == 0).all()) and bool((got["lp"].cpu()[cmask] < 0).all())
    # hipGraph replay == eager launches, bit for bit
    graph = lm.score(x, mask, new, cmask, via="decode", use_graph=True)
    for k in ("lp", "lse", "top1"):
        assert torch.equal(graph[k], got[k]), k
    # == the kernel on the logits of host-driven steps
    s_max = lm.kv_capacity(S + T)
    hidden, kstart, pos = lm.prefill(x, mask, s_max)
    tg = new.to(torch.int32).masked_fill(~cmask.cuda(), -100)
    fed = tg.clamp(min=0)
    lps = [ops.token_logprob(lm.logits(hidden[:, -1, :]), tg[:, 0].contiguous())["lp"]]
    for t in range(1, T):
        e = lm.embed_tokens(fed[:, t - 1:t]).view(B, -1)
        row = lm.decode_embeds(e, pos + (t - 1), S + t - 1, kstart)
        lps.append(ops.token_logprob(lm.logits(row), tg[:, t].contiguous())["lp"])
    assert torch.equal(torch.stack(lps, 1), got["lp"])


def _oracle_lp(W, cfg, x, mask, cont, positions="generate"):
    """fp32 log-probabilities of the tokens ``cont`` [B, T] behind the left-padded prefix embeddings ``x`` [B, S, H]."""
    from oracle import emu2_ref as R
    B, S, _ = x.shape
    T = cont.shape[1]
    full = torch.cat([x.float(), R.embed_tokens(cont[:, :-1].clamp(min=0), W)], dim=1)
    am = torch.cat([mask.long(), torch.ones(B, T - 1, dtype=torch.long)], dim=1)
    pos = (am.cumsum(-1) - 1).masked_fill(am == 0, 1) if positions == "generate" else None
    h = R.llama_model(full, am, W, cfg.llama, position_ids=pos)
    logits = torch.nn.functional.linear(h[:, S - 1:], W["decoder.lm.lm_head.weight"]).float()
    return torch.log_softmax(logits, -1).gather(2, cont.clamp(min=0)[..., None])[..., 0]


def _score_fixture(tiny_model):
    m, W, cfg, z = tiny_model
    ids, mask = _text_prompts(z, 2)
    g = torch.Generator().manual_seed(11)
    cont = torch.cat([_t(z["new2"])[:1].long(), torch.randint(3, 32000, (1, 6), generator=g)])     # the greedy ids and random ones
    cmask = torch.ones(2, 6, dtype=torch.bool)
    cmask[1, 4:] = False
    x = m._prompt_embeds(ids, None, m.n_query).view(2, ids.shape[1], -1)
    return m, W, cfg, x, mask, cont, cmask


def test_score_against_the_oracle_both_routes(tiny_model):
    m, W, cfg, x, mask, cont, cmask = _score_fixture(tiny_model)
    lm = m.decoder.lm
    want = _oracle_lp(W, cfg, x.cpu(), mask, cont)
    dec = lm.score(x, mask, cont, cmask, via="decode")
    pre = lm.score(x, mask, cont, cmask, via="prefill", return_logits=True)
    d_dec = float((dec["lp"].cpu() - want)[cmask].abs().max())
    d_pre = float((pre["lp"].cpu() - want)[cmask].abs().max())
    d_routes = float((dec["lp"] - pre["lp"]).abs().max())
    print(f"score vs oracle: decode {d_dec:.4e}, prefill {d_pre:.4e}, decode vs prefill {d_routes:.4e}")
    assert d_dec <= ORACLE_TOL and d_pre <= ORACLE_TOL       # measured 0.0229 / 0.0452 on MI355X; the bound is twice the larger
    assert d_routes <= ORACLE_TOL                            # measured 0.0311
    for r in (dec, pre):
        assert torch.equal(r["counted"].cpu(), cmask) and bool((r["lp"].cpu()[~cmask] == 0).all())
    assert pre["logits"].shape == (2, 6, lm.vocab) and pre["logits"].dtype == BF16
    # the returned logits are the scored ones
    from emu_amd import ops
    tg = cont.to(torch.int32).masked_fill(~cmask, -100).cuda()
    again = ops.token_logprob(pre["logits"].reshape(12, -1), tg.reshape(-1))
    assert torch.equal(again["lp"].view(2, 6), pre["lp"])


@pytest.mark.parametrize("mode", ("fp4", "fp8"))
def test_decode_route_scores_the_active_weight_stream(tiny_model, mode):
    m, W, cfg, x, mask, cont, cmask = _score_fixture(tiny_model)
    lm = m.decoder.lm
    base = lm.score(x, mask, cont, cmask, via="decode", return_logits=True)
    if mode == "fp4":
        lm.quantize_fp4()
        switch = lm.use_fp4
    else:
        lm.quantize_fp8()
        switch = lm.use_fp8
    switch(True)
    try:
        got = lm.score(x, mask, cont, cmask, via="decode", reference_logits=base["logits"])
    finally:
        switch(False)
    assert not torch.equal(got["lp"], base["lp"])            # the stream really was scored
    kl = got["kl"].cpu()
    print(f"{mode}: mean |dlp| {float((got['lp'] - base['lp']).abs().mean()):.4f}, kl mean {float(kl.mean()):.4e} max {float(kl.max()):.4e}, "
          f"top-1 agreement {float(got['agree'].float().mean()):.2f}")
    assert bool(torch.isfinite(kl).all()) and bool((kl > 0).all())
    assert got["agree"].dtype == torch.bool and got["agree"].shape == (2, 6)
    again = lm.score(x, mask, cont, cmask, via="decode")
    assert torch.equal(again["lp"], base["lp"])              # switching back restores the bf16 stream


# ------------------------------------------------------------------------------------------------ 5. Emu.predict_ids
# six candidates of 1-4 tokens, chosen on the CPU: in the oracle's fp32 losses every adjacent gap in sorted order exceeds twice the
# per-loss deviation bound, for one segment (smallest gap 0.149) and for two (0.0557, bound 2 * 0.0259); the test asserts it
PREDICT_CANDS = [[17], [40, 9], [5, 33, 21], [12, 12, 50, 7], [61, 2], [28, 44, 3]]


def _emu1_fixture(golden_dir):
    from oracle import emu1_ref as E, emu2_ref as R
    z = tiny.load(golden_dir, "emu1_generate_tiny.npz")
    v, t5, l, vocab, W, cfg = tiny.emu1_generate_from(z)
    ids, mask, img = _t(z["ids"]), _t(z["mask"]), _t(z["image"])
    return z, v, t5, l, vocab, W, cfg, ids, mask, img


def emu1_oracle_losses(golden_dir, cands, n_segments):
    """The oracle's fp32 candidate losses: per-token log-probabilities from R.llama_model + log_softmax on prompt + candidate
    (positions arange), then the reference's mean over its segment's padded width."""
    from oracle import emu1_ref as E, emu2_ref as R
    z, v, t5, l, vocab, W, cfg, ids, mask, img = _emu1_fixture(golden_dir)
    Wb = R.bf16_round(W)
    x = R.embed_tokens(ids, Wb)
    e = E.encode_image(img, Wb, cfg)
    x = R.scatter_image_embeds(x, ids, e.reshape(-1, e.shape[-1]))
    N, Tc, S = len(cands), max(len(c) for c in cands), ids.shape[1]
    cand = torch.full((N, Tc), -100, dtype=torch.int64)
    for i, c in enumerate(cands):
        cand[i, :len(c)] = torch.tensor(c)
    lp = _oracle_lp(Wb, cfg, x.expand(N, -1, -1), mask.expand(N, -1), cand, positions="arange")
    counted = cand >= 0
    losses = torch.empty(N)
    for a, b in scoring.split_segments(N, n_segments):
        losses[a:b] = scoring.reference_candidate_losses(lp[a:b], counted[a:b], S, max(len(c) for c in cands[a:b]))
    return losses, cand, counted


@pytest.mark.parametrize("n_segments", (1, 2))
def test_emu1_predict_ids_ranks_as_the_oracle(golden_dir, n_segments):
    from emu_amd.emu1 import Emu
    z, v, t5, l, vocab, W, cfg, ids, mask, img = _emu1_fixture(golden_dir)
    want, cand, counted = emu1_oracle_losses(golden_dir, PREDICT_CANDS, n_segments)
    S = ids.shape[1]
    # a loss is a sum of at most 4 per-token lp over S + Tmax - 1 positions: its deviation is bounded by 4 * ORACLE_TOL / (S + Tmax - 1)
    tol = 4 * ORACLE_TOL / S
    gaps = want.sort().values.diff()
    assert bool((gaps > 2 * tol).all()), (gaps.tolist(), tol)                       # every pair is decidable: none is left out
    m = Emu(v, l, t5, vocab=vocab, device="cuda")
    m.load_state_dict(W, strict=True)
    ranks, losses = m.predict_ids(ids, mask, img.cuda(), cand.clamp(min=0), counted, n_segments=n_segments, return_losses=True)
    d = float((losses - want).abs().max())
    # measured on MI355X: 3.4e-3 (one segment), 3.3e-3 (two)
    print(f"predict_ids n_segments={n_segments}: losses vs oracle {d:.3e} (bound {tol:.3e}), smallest gap {float(gaps.min()):.3e}")
    assert ranks.shape == (1, len(PREDICT_CANDS)) and ranks.dtype == torch.int64
    assert ranks[0].tolist() == torch.argsort(want).tolist()
    assert d <= tol
    # the decode route ranks the same
    ranks_d = m.predict_ids(ids, mask, img.cuda(), cand.clamp(min=0), counted, n_segments=n_segments, via="decode")
    assert ranks_d.tolist() == ranks.tolist()


# ------------------------------------------------------------------------------------------------ 6. EmuModel.score_ids
def test_score_ids_with_an_image_equals_the_engine_on_the_same_embeddings(tiny_model):
    m, W, cfg, z = tiny_model
    ids, mask, image = _t(z["ids1"]), _t(z["mask1"]), _t(z["image"]).cuda()
    cont = _t(z["new1"]).long()[:, :6]
    cmask = torch.ones_like(cont, dtype=torch.bool)
    cmask[0, 5:] = False
    got = m.score_ids(ids, mask, image, None, cont, cmask, via="decode", use_graph=False)
    x = m._prompt_embeds(ids, image, m.n_query).view(1, ids.shape[1], -1)
    want = m.decoder.lm.score(x, mask, cont, cmask, via="decode")
    assert set(got) == set(want) == {"lp", "counted", "lse", "top1"}
    for k in want:
        assert torch.equal(got[k], want[k]), k
