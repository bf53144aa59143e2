"""GPU tests of the few-row MXFP4 weight stream on the matrix cores (csrc/gemv_fp4_thin.hip, ``ops.linear_fp4w_thin``,
``LlamaEngine.use_fp4(True, wide=True)``): steps of 3..16 rows -- the default 5-beam search, batches, contrastive search.

Every dequantised MXFP4 value is exact in bf16, so the MFMA sees exact weights: (a) the decode of every code in every nibble /
byte position through the conversion and the MFMA, exactly; (b) the linear with its epilogues against the host definition at the
bounds tests/test_gpu_fp4.py uses for the same arithmetic; (c) the rejections; (d) an engine step of 5 and of 16 rows against the
CPU oracle, with a witness that the 4-bit bytes were what streamed, and mode 1 unchanged; (e) 5-beam search against a twin engine
holding the dequantised weights as bf16; (f) the vocabulary-sharded head.

Observed on MI355X for bf16-denormal products (scale bytes 1 and 2 in (a), test_decode_denormal_products): all 2048 of them come
out exact -- neither v_cvt_scalef32_pk_bf16_fp4 nor the bf16 MFMA flushes them, as mxfp4.dequantize does not.
"""
import pytest
import torch

from tests import tiny
from tests.fp4_common import BF16, _case, _f32, _gemv_profile, _tiny_model, bfr, rel_err, tiny_fp4  # noqa: F401 (tiny_fp4: the fixture)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ (a) decode, exhaustive
def _exhaustive(scale_bytes):
    """Row n: code n % 16 at position n // 16 of EVERY block (the other positions hold position-dependent codes); one block per
    scale byte.  Returns packed, scales, the host dequantisation [N, K] and the device outputs [K, N] for one-hot rows fed 16 at a time."""
    from emu_amd import mxfp4, ops
    K = 32 * len(scale_bytes)
    N = 16 * 32
    codes = torch.empty(N, K, dtype=torch.uint8)
    pos = torch.arange(K) % 32
    for n in range(N):
        c, p = n % 16, n // 16
        codes[n] = ((pos * 5 + 3 + n) % 16).to(torch.uint8)
        codes[n, pos == p] = c
    scales = torch.tensor(scale_bytes, dtype=torch.uint8).repeat(N, 1)
    # 4 * 2^126, 6 * 2^126 and 2 * 2^127 upwards exceed the largest fp32 / bf16 number: under scale bytes 253 and 254 the host value
    # of those codes is inf, and one inf anywhere in a weight row turns every other output of that row into 0 * inf = NaN in ANY dot
    # product.  Codes whose product is not a number keep their sign and fall back to magnitude 0 / 0.5 in those blocks, so every
    # byte, every position and every code whose product exists is still checked exactly.
    over = ~torch.isfinite(mxfp4.dequantize(mxfp4.pack_codes(codes), scales))
    codes[over] &= 0b1001
    packed = mxfp4.pack_codes(codes)
    want = mxfp4.dequantize(packed, scales)
    assert bool(torch.isfinite(want).all()) and torch.equal(want.to(BF16).float(), want)
    assert bool((over.reshape(N, -1, 32).any(-1).any(0) == (torch.tensor(scale_bytes) >= 253)).all())
    p_d, s_d = packed.cuda(), scales.cuda()
    eye = torch.eye(K, dtype=BF16).cuda()
    got = torch.empty(K, N)
    for k0 in range(0, K, 16):
        got[k0:k0 + 16] = ops.linear_fp4w_thin(eye[k0:k0 + 16], p_d, s_d).float().cpu()
    return want, got


def test_decode_exhaustive_mfma():
    """All 16 codes in every nibble and byte position of a block under 16 scale bytes whose products are all normal bf16 numbers:
    with one-hot x = 1.0 every output is a single product through v_cvt_scalef32_pk_bf16_fp4 and the MFMA, so it must equal the
    host dequantisation exactly (pins the nibble order, the byte select, how the scale operand is read, and the A / B k pairing)."""
    want, got = _exhaustive([3, 4, 60, 100, 125, 126, 127, 128, 129, 150, 200, 250, 251, 252, 253, 254])
    assert want.shape[1] == 512
    assert bool((want.abs()[want != 0] >= 2.0 ** -126).all())                   # every product is a normal bf16 number
    assert torch.equal(got, want.t())


def test_decode_denormal_products():
    """Scale bytes 1 and 2: products of magnitude 2^-127 .. 2^-126 * 0.75 are bf16 denormals.  Each output must equal the host
    value or be a zero of the right sign (the other scale bytes of the K = 256 row are normal and must be exact).
    Observed on MI355X: 2048 denormal products, all exact, none flushed (the count is printed)."""
    want, got = _exhaustive([1, 2, 127, 128, 129, 150, 200, 250])
    want = want.t()
    exact = got == want
    flushed = (got == 0) & (torch.signbit(got) == torch.signbit(want))
    denorm = (want != 0) & (want.abs() < 2.0 ** -126)
    print(f"bf16-denormal products: {int(denorm.sum())}, exact {int((exact & denorm).sum())}, flushed to signed zero {int((flushed & denorm & ~exact).sum())}")
    assert bool((exact | (flushed & denorm)).all())
    assert bool(exact[~denorm].all())


# ------------------------------------------------------------------------------------------------ (b) linear parity
def _differs_from_bf16_stream(x, wd, got, **kw):
    from emu_amd import ops
    ref = ops.linear(x.cuda(), wd.to(BF16).cuda(), **kw)
    return float((ref != got).float().mean())


@pytest.mark.parametrize("M", [3, 5, 8, 9, 16])
@pytest.mark.parametrize("N,K", [(16, 256), (37, 512), (1000, 6656), (64, 17920)])
def test_linear_fp4w_thin_plain_and_resid(M, N, K):
    from emu_amd import ops
    q, sc, wd = _case(N, K)
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(BF16)
    res = torch.randn(M, N, generator=g).to(BF16)
    want = bfr(x.float() @ wd.T)
    got = ops.linear_fp4w_thin(x.cuda(), q, sc)
    e1 = rel_err(got, want)
    d1 = _differs_from_bf16_stream(x, wd, got)
    got = ops.linear_fp4w_thin(x.cuda(), q, sc, res=res.cuda(), epi=ops.EPI_RESID)
    e2 = rel_err(got, bfr(want + res.float()))
    print(f"fp4 thin M={M} N={N} K={K}: rel L2 plain {e1:.2e} resid {e2:.2e}; elements differing from the bf16 stream {d1:.4f}")
    assert e1 < 4e-3
    assert e2 < 4e-3


def test_linear_fp4w_thin_bias():
    from emu_amd import ops
    N, K, M = 300, 512, 5
    q, sc, wd = _case(N, K)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, K, generator=g).to(BF16)
    bias = torch.randn(N, generator=g).to(BF16)
    want = bfr(x.float() @ wd.T + bias.float())
    assert rel_err(ops.linear_fp4w_thin(x.cuda(), q, sc, bias=bias.cuda()), want) < 4e-3


@pytest.mark.parametrize("M", [5, 16])
@pytest.mark.parametrize("N,K", [(38, 512), (2240, 6656)])
def test_linear_fp4w_thin_swiglu(M, N, K):
    from emu_amd import ops
    q, sc, wd = _case(N, K, 1)
    g = torch.Generator().manual_seed(11 + M + N)
    x = torch.randn(M, K, generator=g).to(BF16)
    y = bfr(x.float() @ wd.T)
    want = bfr(bfr(torch.nn.functional.silu(y[:, 0::2])) * y[:, 1::2])          # packed rows interleave gate / up
    got = ops.linear_fp4w_thin(x.cuda(), q, sc, epi=ops.EPI_SWIGLU)
    assert got.shape == (M, N // 2)
    e = rel_err(got, want)
    d = _differs_from_bf16_stream(x, wd, got, epi=ops.EPI_SWIGLU)
    print(f"fp4 thin SwiGLU M={M} N={N} K={K}: rel L2 {e:.2e}; elements differing from the bf16 stream {d:.4f}")
    assert e < 8e-3


# ------------------------------------------------------------------------------------------------ (c) rejections
def test_fp4_thin_rejections():
    from emu_amd import ops
    from emu_amd._lib import EmuHipError

    def args(M, N, K):
        return (torch.zeros(M, K, dtype=BF16, device="cuda"), torch.zeros(N, K // 2, dtype=torch.uint8, device="cuda"),
                torch.full((N, K // 32), 127, dtype=torch.uint8, device="cuda"))
    ops.linear_fp4w_thin(*args(16, 64, 256))
    ops.linear_fp4w_thin(*args(1, 64, 256))
    with pytest.raises(EmuHipError):
        ops.linear_fp4w_thin(*args(17, 64, 256))
    with pytest.raises(EmuHipError):
        ops.linear_fp4w_thin(*args(5, 64, 288))
    with pytest.raises(EmuHipError):
        ops.linear_fp4w_thin(*args(5, 64, 128))
    with pytest.raises(EmuHipError):
        ops.linear_fp4w_thin(*args(5, 63, 256), epi=ops.EPI_SWIGLU)
    with pytest.raises(EmuHipError):
        ops.linear_fp4w(*args(3, 64, 256))                                       # the VALU stream still ends at two rows


def test_use_fp4_wide_rejects_widths_not_multiple_of_256():
    from emu_amd import synth
    from emu_amd._lib import EmuHipError
    from emu_amd.conf.emu_conf import LlamaCfg
    from emu_amd.llama import EmuHipContext, LlamaEngine
    l = LlamaCfg(hidden_size=128, intermediate_size=256, num_attention_heads=1, num_hidden_layers=1)
    eng = LlamaEngine(l, 64, EmuHipContext(torch.device("cuda", 0)))
    eng.load_weights(synth.iter_synth(synth.llama_param_shapes(l, 64), device="cuda", dtype=BF16))
    assert eng.ready
    with pytest.raises(EmuHipError, match="multiples of 256"):
        eng.use_fp4(True, wide=True)
    assert not getattr(eng, "fp4_wide", False) and not getattr(eng, "fp4_decode", False)
    eng.use_fp4(True)                                                            # mode 1 takes multiples of 32
    eng.use_fp4(False)


# ------------------------------------------------------------------------------------------------ engine
@pytest.mark.parametrize("B", [5, 16])
def test_fp4_wide_step_matches_oracle_and_streams_the_4bit_set(tiny_fp4, B):                 # (d)
    """bf16 prefill of B rows, then ONE cached single-token step of B rows through the wide fp4 stream == the oracle's step on the
    dequantised weights; the GEMV profiler counts exactly the 4-bit bytes of the layers' matrices and the head."""
    from emu_amd import mxfp4
    from oracle import emu2_ref as R
    m, W, W4, cfg = tiny_fp4
    lm = m.decoder.lm
    g = torch.Generator().manual_seed(5 + B)
    S = 24
    x = (torch.randn(B, S + 1, cfg.llama.hidden, generator=g) * 0.5).to(BF16)
    mask = torch.ones(B, S, dtype=torch.long)
    cache = R.KVCache(cfg.llama.layers)
    xf = x.float()
    R.llama_model(xf[:, :S].to(BF16), mask, R.cast_weights(W, BF16), cfg.llama, cache=cache, final_norm=False)
    mask1 = torch.ones(B, S + 1, dtype=torch.long)
    want = R.llama_model(xf[:, S:], mask1, R.cast_weights(W4, torch.float32), cfg.llama, cache=_f32(cache), final_norm=False)[:, 0]
    out = {}

    def step():
        out["h"] = lm.decode_embeds(x[:, S].contiguous().cuda(), pos, S, kstart)
        out["l"] = lm.logits(out["h"])
    try:
        lm.use_fp4(True, wide=True)
        assert lm.fp4_wide
        fp4_bytes = lm.weight_bytes_per_token()
        _, kstart, pos = lm.prefill(x[:, :S].contiguous().cuda(), mask)
        wb, nl = _gemv_profile(step)
    finally:
        lm.use_fp4(False)
    assert not lm.fp4_wide
    e_h = rel_err(out["h"], want)
    h = R.rms_norm(want, W["decoder.lm.model.norm.weight"].float(), cfg.llama.rms_eps)
    e_l = rel_err(out["l"], h @ W4["decoder.lm.lm_head.weight"].T)
    print(f"fp4 wide step B={B} vs oracle: hidden {e_h:.2e}, logits {e_l:.2e}; profiler {wb:.0f} bytes in {nl} launches")
    assert e_h < 2e-2
    assert e_l < 2.5e-2
    mats = [lm._keep[f"{i}.{k}"] for i in range(cfg.llama.layers) for k in lm._FP4_KINDS] + [lm.lm_head]
    assert fp4_bytes == sum(t.shape[0] * mxfp4.bytes_per_row(t.shape[1]) for t in mats)
    assert wb == fp4_bytes and nl == len(mats)
    assert wb != sum(t.numel() * 2 for t in mats)


def test_fp4_narrow_mode_leaves_five_row_steps_on_bf16(tiny_fp4):                             # (d) mode 1 unchanged
    """With wide=False a 5-row step is bit-identical to an engine that never enabled fp4, and streams the bf16 bytes."""
    m, W, W4, cfg = tiny_fp4
    lm = m.decoder.lm
    B, S = 5, 24
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(B, S + 1, cfg.llama.hidden, generator=g) * 0.5).to(BF16)
    mask = torch.ones(B, S, dtype=torch.long)

    def run():
        _, kstart, pos = lm.prefill(x[:, :S].contiguous().cuda(), mask)
        out = {}

        def step():
            out["h"] = lm.decode_embeds(x[:, S].contiguous().cuda(), pos, S, kstart)
            out["l"] = lm.logits(out["h"])
        wb, _ = _gemv_profile(step)
        return out["h"].cpu(), out["l"].cpu(), wb
    h0, l0, wb0 = run()
    try:
        lm.use_fp4(True)
        h1, l1, wb1 = run()
    finally:
        lm.use_fp4(False)
    assert torch.equal(h0, h1) and torch.equal(l0, l1)
    assert wb0 == wb1 == sum(t.numel() * 2 for k, t in lm._keep.items() if k.split(".")[1] in lm._FP4_KINDS) + lm.lm_head.numel() * 2


def test_fp4_wide_beam_search_equals_twin_engine(tiny_fp4, golden_dir):                      # (e)
    """5-beam search through the wide fp4 stream against a twin engine that holds the dequantised weights as bf16 and runs the bf16
    stream (prefill sees the same weights in both).  Ids must be equal; a divergence is allowed only at a step where the twin's own
    gap between the candidates that swapped is below 0.08 (the bound of test_fp4_greedy_equals_twin_engine_graph_equals_eager) --
    measured here as the twin's gap, at that step, between the accumulated scores of the two continuations, the failure message
    prints it.  Twice the same ids; switching the stream off restores the fixture's bf16 beam ids."""
    from emu_amd import EmuModel, TextDecoderCfg
    m, W, W4, cfg = tiny_fp4
    z = tiny.load(golden_dir, "generate_tiny.npz")
    v, l, vocab, _ = tiny.weights_from(z)
    ids, mask = torch.from_numpy(z["ids2"]), torch.from_numpy(z["mask2"])
    n_new = 6
    kw = dict(max_new_tokens=n_new, num_beams=5, hf_semantics="5.x")
    m4 = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda")
    m4.load_state_dict(W4, strict=True)
    twin = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda")
    twin.load_state_dict(W4, strict=True)
    lm4 = m4.decoder.lm
    try:
        lm4.use_fp4(True, wide=True)
        got = m4.generate_ids(ids, mask, None, **kw).cpu()
        again = m4.generate_ids(ids, mask, None, **kw).cpu()
    finally:
        lm4.use_fp4(False)
    assert got.tolist() == again.tolist()
    want = twin.generate_ids(ids, mask, None, **kw).cpu()
    tl = twin.decoder.lm
    B, S = ids.shape
    for b in range(B):
        if got[b].tolist() == want[b].tolist():
            continue
        i = next(j for j in range(n_new) if int(got[b, j]) != int(want[b, j]))
        # the twin's accumulated log-probabilities of both sequences up to and including step i (teacher-forced, one row each)
        def score(seq):
            x = twin._prompt_embeds(ids[b:b + 1], None, twin.n_query)
            hidden, kstart, pos = tl.prefill(x.view(1, S, -1), mask[b:b + 1])
            lp = torch.log_softmax(tl.logits(hidden[:, -1, :].contiguous()).float(), -1)
            tot = float(lp[0, int(seq[0])])
            for j in range(i):
                e = tl.embed_tokens(seq[j:j + 1][None].cuda()).view(1, -1)
                lp = torch.log_softmax(tl.logits(tl.decode_embeds(e, pos + j, S + j, kstart)).float(), -1)
                tot += float(lp[0, int(seq[j + 1])])
            return tot
        gap = abs(score(want[b]) - score(got[b]))
        assert gap < 0.08, f"row {b} diverged from the twin at step {i}; the twin's gap between the two candidates is {gap:.3f}"
    # the original engine: the wide stream on and off again -> its own bf16 beam ids, and the real reference's ids on the fixture
    # whose 5-beam pruning margins are wide enough to pin them (tests/test_gpu_model.py::test_generate_beam_search)
    lm = m.decoder.lm
    before = m.generate_ids(ids, mask, None, **kw).cpu()
    try:
        lm.use_fp4(True, wide=True)
        m.generate_ids(ids, mask, None, **kw)
    finally:
        lm.use_fp4(False)
    assert m.generate_ids(ids, mask, None, **kw).cpu().tolist() == before.tolist()
    zm = tiny.load(golden_dir, "generate_margin_tiny.npz")
    b5 = m.generate_ids(torch.from_numpy(zm["b5_ids"]), torch.from_numpy(zm["b5_mask"]), torch.from_numpy(zm["image"]).cuda(),
                        max_new_tokens=int(zm["b5_n_new"]), num_beams=5, hf_semantics="5.x")
    assert b5.cpu().tolist() == zm["b5_new"].tolist()


def test_fp4_wide_head_shard_equals_whole_head(golden_dir):                                  # (f)
    """emu_llama_set_head_shard on a single-rank context: the engine is handed rows [r0, r1) of lm_head and of its 4-bit copy; the
    5-row mode-2 logits of those columns equal the unsharded mode-2 logits bit for bit, every other column is zero."""
    from emu_amd._lib import check, lib
    m, *_ = _tiny_model(golden_dir)
    lm = m.decoder.lm
    g = torch.Generator().manual_seed(3)
    hid = (torch.randn(5, lm.cfg.hidden_size, generator=g) * 0.5).to(BF16).cuda()
    lm.use_fp4(True, wide=True)
    try:
        whole = lm.logits(hid).cpu()
        r0, r1 = 4100, 4100 + 8075                                               # a ragged, unaligned slice of the vocabulary
        head = lm.lm_head[r0:r1].contiguous()
        q, sc = (t[r0:r1].contiguous() for t in lm._fp4["lm_head"])
        h = lm.handle
        check(lib().emu_llama_set_head(h, lm.final_norm.data_ptr(), head.data_ptr(), lm.embed.data_ptr(), lm.cos.data_ptr(),
                                       lm.sin.data_ptr()), "emu_llama_set_head")
        check(lib().emu_llama_set_head_fp4(h, q.data_ptr(), sc.data_ptr()), "emu_llama_set_head_fp4", lm.ctx.handle)
        check(lib().emu_llama_set_head_shard(h, r0, r1 - r0), "emu_llama_set_head_shard", lm.ctx.handle)
        out = {}
        wb, nl = _gemv_profile(lambda: out.update(l=lm.logits(hid)))
        shard = out["l"].cpu()
    finally:
        check(lib().emu_llama_set_head_shard(lm.handle, 0, -1), "emu_llama_set_head_shard", lm.ctx.handle)
        check(lib().emu_llama_set_head(lm.handle, lm.final_norm.data_ptr(), lm.lm_head.data_ptr(), lm.embed.data_ptr(),
                                       lm.cos.data_ptr(), lm.sin.data_ptr()), "emu_llama_set_head")
        lm._fp4_register("lm_head")
        lm.use_fp4(False)
    from emu_amd import mxfp4
    assert wb == (r1 - r0) * mxfp4.bytes_per_row(lm.cfg.hidden_size) and nl == 1
    assert torch.equal(shard[:, r0:r1], whole[:, r0:r1])
    assert not bool(shard[:, :r0].any()) and not bool(shard[:, r1:].any())
