"""GPU tests of the optional MXFP4 decode weight stream (4-bit E2M1 elements, one E8M0 scale per 32: emu_amd/mxfp4.py).

Not a reference feature.  Every dequantised MXFP4 value is exact in bf16, so "the fp4 stream" and "the bf16 stream loaded with
the dequantised weights" compute the same function: the tests pin (a) the device quantiser byte for byte against the host
definition, (b) the decode of every code in every nibble / byte position exactly, (c, d) the GEMV with its epilogues against a
torch product of the exact weights at the fp8 stream's bounds, (e) the rejections, (f, g) the engine against the CPU oracle and
against a twin engine that holds the dequantised weights as bf16, (h) the accuracy against the bf16 stream on the margin
fixture's prompts -- measured and printed, asserted only where no number is needed -- and (i) loading prepared tensors.
"""
import pytest
import torch

from tests import tiny
from tests.fp4_common import BF16, _f32, _tiny_model, bfr, rel_err, tiny_fp4  # noqa: F401 (tiny_fp4: the fixture, used by name)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ (a) quantiser
@pytest.mark.parametrize("N,K", [(64, 256), (37, 512), (8, 6656)])
def test_quantiser_matches_host_definition_byte_for_byte(N, K):
    from emu_amd import mxfp4, ops
    g = torch.Generator().manual_seed(N * 7 + K)
    w = (torch.randn(N, K, generator=g) * 0.05).to(BF16)
    w[0, :8] = torch.tensor([0.0, -0.0, 1e-39, -3e-40, 2.0, 9.2e-41, -1e-38, 1.0]).to(BF16)    # zeros, bf16 denormals
    w[1, :32] = 0                                                                               # a zero block
    w[1, 3] = -0.0
    w[2, 32:64] = torch.tensor([1e-39, -2e-39, 4e-40] + [0.0] * 29).to(BF16)                    # a block of denormals only
    w[3, :6] = torch.tensor([6.0, 2.5, -3.5, 0.25, 5.0, -1.25]).to(BF16)                        # exact ties under scale 1
    w[3, 6:32] = 0.5
    w[4, :4] = torch.tensor([7.5, -7.0, 0.1, 3.0e38]).to(BF16)                                  # saturation, the top exponent
    q, sc = ops.quantize_mxfp4_rows(w.cuda())
    qr, sr = mxfp4.quantize_rows(w)
    assert q.dtype == sc.dtype == torch.uint8 and q.shape == (N, K // 2) and sc.shape == (N, K // 32)
    assert torch.equal(sc.cpu(), sr)
    got, want = mxfp4.unpack_codes(q.cpu()), mxfp4.unpack_codes(qr)
    zero = (want & 7) == 0                                   # sign nibbles of zero compare as values
    assert torch.equal(got & 7, want & 7)
    assert torch.equal(got[~zero], want[~zero])
    assert torch.equal(mxfp4.dequantize(q.cpu(), sc.cpu()), mxfp4.dequantize(qr, sr))
    # ... and the device kernel keeps the sign of zero too
    assert torch.equal(q.cpu(), qr)


def test_quantiser_rejects_non_finite():
    from emu_amd import ops
    from emu_amd._lib import EmuHipError
    w = torch.zeros(4, 64, dtype=BF16)
    w[2, 40] = float("inf")
    with pytest.raises(EmuHipError):
        ops.quantize_mxfp4_rows(w.cuda())


# ------------------------------------------------------------------------------------------------ (b) decode, exhaustive
def test_decode_exhaustive():
    """All 16 codes in every nibble and byte position of a block, under scale bytes spanning the clamped range: with one-hot
    x = 1.0 every output is a single product, so it must equal the host dequantisation exactly (this pins which nibble of a byte
    v_cvt_scalef32_pk_f32_fp4 puts in which result lane and how it reads its scale operand)."""
    from emu_amd import mxfp4, ops
    scale_bytes = [1, 2, 60, 126, 127, 128, 200, 251, 252]
    K = 32 * len(scale_bytes)
    N = 16 * 32                                              # row n: code n % 16 at position n // 16 of EVERY block, others differ
    codes = torch.empty(N, K, dtype=torch.uint8)
    pos = torch.arange(K) % 32
    for n in range(N):
        c, p = n % 16, n // 16
        codes[n] = ((pos * 5 + 3 + n) % 16).to(torch.uint8)  # background: all codes, position-dependent
        codes[n, pos == p] = c
    packed = mxfp4.pack_codes(codes)
    scales = torch.tensor(scale_bytes, dtype=torch.uint8).repeat(N, 1)
    want = mxfp4.dequantize(packed, scales)                  # [N, K]
    assert torch.equal(want.to(BF16).float(), want)
    p_d, s_d = packed.cuda(), scales.cuda()
    eye = torch.eye(K, dtype=BF16)
    got = torch.empty(K, N)
    for k0 in range(0, K, 2):                                # M = 2 rows per call, and M = 1 for the first block
        got[k0:k0 + 2] = ops.linear_fp4w(eye[k0:k0 + 2].cuda(), p_d, s_d).float().cpu()
    assert torch.equal(got, want.t())
    for k in range(32):
        assert torch.equal(ops.linear_fp4w(eye[k:k + 1].cuda(), p_d, s_d).float().cpu()[0], want[:, k])


# ------------------------------------------------------------------------------------------------ (c) plain and residual
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("N,K", [(512, 256), (1000, 6656), (4100, 512), (32274, 256), (1024, 17920), (2048, 896), (2048, 2240)])
def test_linear_fp4w_plain_and_resid(M, N, K):
    from emu_amd import mxfp4, ops
    g = torch.Generator().manual_seed(M + N + K)
    w = (torch.randn(N, K, generator=g) * 0.03).to(BF16)
    x = (torch.randn(M, K, generator=g)).to(BF16)
    res = (torch.randn(M, N, generator=g)).to(BF16)
    q, sc = ops.quantize_mxfp4_rows(w.cuda())
    wd = mxfp4.dequantize(q.cpu(), sc.cpu())
    want = bfr(x.float() @ wd.T)
    got = ops.linear_fp4w(x.cuda(), q, sc)
    e1 = rel_err(got, want)
    got = ops.linear_fp4w(x.cuda(), q, sc, res=res.cuda(), epi=ops.EPI_RESID)
    e2 = rel_err(got, bfr(want + res.float()))
    print(f"fp4 linear M={M} N={N} K={K}: rel L2 plain {e1:.2e} resid {e2:.2e}")
    assert e1 < 4e-3
    assert e2 < 4e-3


def test_linear_fp4w_bias():
    from emu_amd import mxfp4, ops
    g = torch.Generator().manual_seed(5)
    N, K = 300, 512
    w = (torch.randn(N, K, generator=g) * 0.03).to(BF16)
    x = torch.randn(2, K, generator=g).to(BF16)
    bias = torch.randn(N, generator=g).to(BF16)
    q, sc = ops.quantize_mxfp4_rows(w.cuda())
    want = bfr(x.float() @ mxfp4.dequantize(q.cpu(), sc.cpu()).T + bias.float())
    assert rel_err(ops.linear_fp4w(x.cuda(), q, sc, bias=bias.cuda()), want) < 4e-3


# ------------------------------------------------------------------------------------------------ (d) fused norm, SwiGLU
@pytest.mark.parametrize("M", [1, 2])
def test_linear_fp4w_fused_norm_and_swiglu(M):
    from emu_amd import mxfp4, ops
    N, K, eps = 2 * 1120, 6656, 1e-5
    g = torch.Generator().manual_seed(11 + M)
    w = (torch.randn(N, K, generator=g) * 0.02).to(BF16)
    x = (torch.randn(M, K, generator=g) * 2).to(BF16)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(BF16)
    q, sc = ops.quantize_mxfp4_rows(w.cuda())
    wd = mxfp4.dequantize(q.cpu(), sc.cpu())
    xf = x.float()
    xn = bfr(nw.float() * bfr(xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)))
    y = bfr(xn @ wd.T)
    got = ops.linear_fp4w(x.cuda(), q, sc, norm_w=nw.cuda(), eps=eps)
    e1 = rel_err(got, y)
    gate, up = y[:, 0::2], y[:, 1::2]                                      # packed rows interleave gate/up
    want = bfr(bfr(torch.nn.functional.silu(gate)) * up)
    got = ops.linear_fp4w(x.cuda(), q, sc, norm_w=nw.cuda(), eps=eps, epi=ops.EPI_SWIGLU)
    assert got.shape == (M, N // 2)
    e2 = rel_err(got, want)
    print(f"fp4 linear fused norm M={M}: rel L2 {e1:.2e}, with SwiGLU {e2:.2e}")
    assert e1 < 5e-3
    assert e2 < 8e-3


# ------------------------------------------------------------------------------------------------ (e) rejections
def test_fp4_rejects_prefill_rows_and_bad_k():
    from emu_amd import ops
    from emu_amd._lib import EmuHipError
    q = torch.zeros(64, 128, dtype=torch.uint8, device="cuda")
    sc = torch.full((64, 8), 127, dtype=torch.uint8, device="cuda")
    ops.linear_fp4w(torch.zeros(2, 256, dtype=BF16, device="cuda"), q, sc)
    with pytest.raises(EmuHipError):
        ops.linear_fp4w(torch.zeros(3, 256, dtype=BF16, device="cuda"), q, sc)           # > 2 rows: bf16 territory
    q48 = torch.zeros(64, 32, dtype=torch.uint8, device="cuda")
    sc48 = torch.full((64, 2), 127, dtype=torch.uint8, device="cuda")
    with pytest.raises(EmuHipError):
        ops.linear_fp4w(torch.zeros(1, 48, dtype=BF16, device="cuda"), q48, sc48)         # K % 32 != 0


def test_use_fp4_needs_registration_and_excludes_fp8(golden_dir):
    from emu_amd import mxfp4
    from emu_amd._lib import EmuHipError, check, lib
    m, *_ = _tiny_model(golden_dir)
    lm = m.decoder.lm
    with pytest.raises(EmuHipError):                                                      # nothing registered yet
        check(lib().emu_llama_use_fp4(lm.handle, 1), "emu_llama_use_fp4", lm.ctx.handle)
    lm.load_fp4("0.wo", *mxfp4.quantize_rows(lm._keep["0.wo"].cpu()))
    with pytest.raises(EmuHipError):                                                      # one matrix is not a model
        check(lib().emu_llama_use_fp4(lm.handle, 1), "emu_llama_use_fp4", lm.ctx.handle)
    lm.use_fp8(True)
    try:
        with pytest.raises(EmuHipError, match="exclusive"):
            lm.use_fp4(True)
        assert not getattr(lm, "fp4_decode", False)
    finally:
        lm.use_fp8(False)
    lm.use_fp4(True)
    try:
        with pytest.raises(EmuHipError, match="exclusive"):
            lm.use_fp8(True)
        assert not lm.fp8_decode
    finally:
        lm.use_fp4(False)
    with pytest.raises(ValueError):
        lm.load_fp4("0.wo", torch.zeros(3, 3, dtype=torch.uint8), torch.zeros(3, 1, dtype=torch.uint8))
    with pytest.raises(KeyError):
        lm.load_fp4("0.ln1", torch.zeros(3, 3, dtype=torch.uint8), torch.zeros(3, 1, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------ engine
def test_engine_dequantised_weights_match_host_definition(tiny_fp4):                     # (f)
    m, W, W4, cfg = tiny_fp4
    lm = m.decoder.lm
    lm.quantize_fp4()
    assert torch.equal(lm.fp4_dequantized("lm_head").cpu(), W4["decoder.lm.lm_head.weight"])
    assert torch.equal(lm.fp4_dequantized("0.wo").cpu(), W4["decoder.lm.model.layers.0.self_attn.o_proj.weight"])
    assert torch.equal(lm.fp4_dequantized("1.wdown").cpu(), W4["decoder.lm.model.layers.1.mlp.down_proj.weight"])
    bf16_bytes = lm.weight_bytes_per_token()
    lm.use_fp4(True)
    try:
        assert lm.weight_bytes_per_token() * 64 == bf16_bytes * 17
    finally:
        lm.use_fp4(False)


def test_fp4_decode_step_matches_oracle(tiny_fp4):                                       # (f)
    """bf16 prefill, then ONE cached step through the fp4 stream == oracle step on the dequantised weights."""
    from oracle import emu2_ref as R
    m, W, W4, cfg = tiny_fp4
    lm = m.decoder.lm
    g = torch.Generator().manual_seed(5)
    S = 24
    x = (torch.randn(2, S + 1, cfg.llama.hidden, generator=g) * 0.5).to(BF16)
    mask = torch.ones(2, S, dtype=torch.long)
    cache = R.KVCache(cfg.llama.layers)
    xf = x.float()
    R.llama_model(xf[:, :S].to(BF16), mask, R.cast_weights(W, BF16), cfg.llama, cache=cache, final_norm=False)
    mask1 = torch.ones(2, S + 1, dtype=torch.long)
    want = R.llama_model(xf[:, S:], mask1, R.cast_weights(W4, torch.float32), cfg.llama, cache=_f32(cache),
                         final_norm=False)[:, 0]
    try:
        lm.use_fp4(True)
        _, kstart, pos = lm.prefill(x[:, :S].contiguous().cuda(), mask)
        got = lm.decode_embeds(x[:, S].contiguous().cuda(), pos, S, kstart)
        e_h = rel_err(got, want)
        logits = lm.logits(got)
        h = R.rms_norm(want, W["decoder.lm.model.norm.weight"].float(), cfg.llama.rms_eps)
        wl = h @ W4["decoder.lm.lm_head.weight"].T
        e_l = rel_err(logits, wl)
    finally:
        lm.use_fp4(False)
    print(f"fp4 decode step vs oracle: hidden {e_h:.2e}, logits {e_l:.2e}")
    assert e_h < 2e-2
    assert e_l < 2.5e-2


def test_fp4_greedy_equals_twin_engine_graph_equals_eager(tiny_fp4, golden_dir):         # (g)
    """The fp4 stream and the bf16 stream loaded with the dequantised weights compute the same function.  Two more models are
    loaded with the dequantised weights as ordinary bf16 weights: one runs the fp4 stream (quantising dequantised weights returns
    the same bytes, so its 4-bit tensors are those of the original engine, and its bf16 prefill sees the same weights as the
    twin's), the twin runs the bf16 stream.  Greedy ids must be equal; a first divergence of a row is allowed only where the
    twin's top-2 logit margin is below 0.08, and comparison of that row stops there.  On the original engine hipGraph replay
    equals eager launches, and switching the stream off restores the fixture's ids."""
    from emu_amd import EmuModel, TextDecoderCfg
    from oracle import emu2_ref as R
    m, W, W4, cfg = tiny_fp4
    lm = m.decoder.lm
    z = tiny.load(golden_dir, "generate_tiny.npz")
    v, l, vocab, _ = tiny.weights_from(z)
    ids, mask = torch.from_numpy(z["ids2"]), torch.from_numpy(z["mask2"])
    n_new, B, S = 6, ids.shape[0], ids.shape[1]
    m4 = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda")
    m4.load_state_dict(W4, strict=True)
    twin = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda")
    twin.load_state_dict(W4, strict=True)
    lm.quantize_fp4()
    lm4 = m4.decoder.lm
    lm4.quantize_fp4()
    for key in lm._fp4_keys():                                               # the same 4-bit tensors as the original engine's
        assert torch.equal(lm4._fp4[key][0], lm._fp4[key][0]) and torch.equal(lm4._fp4[key][1], lm._fp4[key][1]), key
    try:
        lm4.use_fp4(True)
        got = m4.generate_ids(ids, mask, None, max_new_tokens=n_new, stop_on_eos=False).cpu()
    finally:
        lm4.use_fp4(False)
    # the twin: its own greedy ids, and its logits along them (teacher-forced with its own ids) for the top-2 margins
    want = twin.generate_ids(ids, mask, None, max_new_tokens=n_new, stop_on_eos=False).cpu()
    tl = twin.decoder.lm
    x = twin._prompt_embeds(ids, None, twin.n_query)
    hidden, kstart, pos = tl.prefill(x.view(B, S, -1), mask)
    logits = [tl.logits(hidden[:, -1, :].contiguous()).float().cpu()]
    for i in range(n_new - 1):
        e = tl.embed_tokens(want[:, i:i + 1].cuda()).view(B, -1)
        logits.append(tl.logits(tl.decode_embeds(e, pos + i, S + i, kstart)).float().cpu())
    for b in range(B):
        for i in range(n_new):
            if int(got[b, i]) != int(want[b, i]):
                row = logits[i][b].clone()
                if i < 1:
                    row[R.EOS_ID] = -float("inf")
                t2 = row.topk(2)
                assert int(t2.indices[0]) == int(want[b, i])
                margin = float(t2.values[0] - t2.values[1])
                assert margin < 0.08, f"row {b} diverged from the twin at step {i} with top-2 margin {margin:.3f}"
                break
    # the original engine (bf16 prefill on the original weights, then the fp4 stream): graph replay == eager
    try:
        lm.use_fp4(True)
        m.use_graph = False
        eager = m.generate_ids(ids, mask, None, max_new_tokens=n_new, stop_on_eos=False).cpu()
        m.use_graph = True
        graph = m.generate_ids(ids, mask, None, max_new_tokens=n_new, stop_on_eos=False).cpu()
        again = m.generate_ids(ids, mask, None, max_new_tokens=n_new, stop_on_eos=False).cpu()
    finally:
        lm.use_fp4(False)
    assert eager.tolist() == graph.tolist() == again.tolist()
    bf16_ids = m.generate_ids(ids, mask, None, max_new_tokens=n_new, stop_on_eos=False)
    assert bf16_ids.cpu().tolist() == z["new2"].tolist()                    # switching back restores the bf16 stream


def test_fp4_accuracy_against_bf16_stream_on_the_margin_fixture(tiny_fp4, golden_dir):   # (h)
    """Measured, not promised.  Prompts of generate_margin_tiny.npz, the bf16 run's tokens teacher-forced into both streams, 8 steps,
    2 rows; synthetic weights (random-init logits say nothing about a trained model).  Measured on MI355X (profiles/fp4_decode.md):
    relative L2 of the fp4 logits against the bf16 stream per step and the arg-max agreement -- printed here, asserted are only
    finiteness and that no decision flips whose bf16 top-2 margin exceeds the largest logit change of its row."""
    m, W, W4, cfg = tiny_fp4
    lm = m.decoder.lm
    zm = tiny.load(golden_dir, "generate_margin_tiny.npz")
    ids, mask = torch.from_numpy(zm["pen_ids"]), torch.from_numpy(zm["pen_mask"])
    rel, agree, margin, change = fp4_vs_bf16_teacher_forced(m, ids, mask, 8)
    print("fp4 vs bf16 logits, relative L2 per step:", ["%.4f" % r for r in rel])
    print("arg-max agreement: %d of %d" % (int(agree.sum()), agree.numel()))
    assert all(r == r and r != float("inf") for r in rel)
    assert bool(((margin <= change) | agree).all()), (margin.tolist(), change.tolist(), agree.tolist())


def fp4_vs_bf16_teacher_forced(m, ids, mask, n_new):
    """Logits of the bf16 and the fp4 stream with the bf16 run's greedy tokens fed to both (prefill is bf16 in both, so step 0
    differs by the head alone): per-step relative L2, arg-max agreement [B, n_new], bf16 top-2 margins and largest logit changes."""
    lm = m.decoder.lm
    B, S = ids.shape
    teacher = m.generate_ids(ids, mask, None, max_new_tokens=n_new, stop_on_eos=False).cpu()
    x = m._prompt_embeds(ids, None, m.n_query)

    def run(fp4):
        lm.use_fp4(fp4)
        try:
            hidden, kstart, pos = lm.prefill(x.view(B, S, -1), mask)
            out = [lm.logits(hidden[:, -1, :].contiguous()).float().cpu()]
            for i in range(n_new - 1):
                e = lm.embed_tokens(teacher[:, i:i + 1].cuda()).view(B, -1)
                out.append(lm.logits(lm.decode_embeds(e, pos + i, S + i, kstart)).float().cpu())
        finally:
            lm.use_fp4(False)
        return torch.stack(out, 1)
    lb, lf = run(False), run(True)
    assert bool(torch.isfinite(lf).all())
    d = lf - lb
    rel = [float(d[:, i].norm() / lb[:, i].norm()) for i in range(n_new)]
    agree = lf.argmax(-1) == lb.argmax(-1)
    t2 = lb.topk(2, -1).values
    return rel, agree, t2[..., 0] - t2[..., 1], d.abs().amax(-1)


def test_load_fp4_prepared_tensors_give_the_same_ids(tiny_fp4, golden_dir):              # (i)
    from emu_amd import mxfp4
    m, W, W4, cfg = tiny_fp4
    z = tiny.load(golden_dir, "generate_tiny.npz")
    ids, mask = torch.from_numpy(z["ids2"]), torch.from_numpy(z["mask2"])
    lm = m.decoder.lm
    try:
        lm.use_fp4(True)
        want = m.generate_ids(ids, mask, None, max_new_tokens=6, stop_on_eos=False).cpu()
    finally:
        lm.use_fp4(False)
    m2, *_ = _tiny_model(golden_dir)
    lm2 = m2.decoder.lm
    for key in lm2._fp4_keys():
        src = lm2.lm_head if key == "lm_head" else lm2._keep[key]
        p, s = mxfp4.quantize_rows(src.cpu())                # prepared on the host
        lm2.load_fp4(key, p, s)
        assert torch.equal(lm2._fp4[key][0].cpu(), lm._fp4[key][0].cpu()) and torch.equal(lm2._fp4[key][1].cpu(), lm._fp4[key][1].cpu())
    try:
        lm2.use_fp4(True)                                    # nothing left to quantise on the device
        got = m2.generate_ids(ids, mask, None, max_new_tokens=6, stop_on_eos=False).cpu()
    finally:
        lm2.use_fp4(False)
    assert got.tolist() == want.tolist()
