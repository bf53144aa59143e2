"""The MXFP4 matrix-core kernels on reduction widths that are no multiple of 256 (``ops.linear_fp4w_mfma`` /
emu_linear_fp4w_mfma_bf16: csrc/gemv_fp4_thin.hip up to 16 rows, csrc/gemm_fp4.hip above, the last K stage partial), and the engine's
modes 2 and 3 on such widths.  A stage is 256 k = 8 MX blocks; K % 256 = 32 kb leaves kb = 1..7 valid blocks in the last one.

1. zero-extension identity: the result equals, bit for bit, the existing entry points' on the same problem extended to the next
   multiple of 256 with code 0, scale byte 127 and zero activations (same tiles, same summation order, the added products exactly 0);
2. position exactness: one-hot activations in the partial stage pick single dequantised weights, exactly;
3. poison: 0xFF bytes (NaN scales) and NaN activations behind every logical width change nothing;
4. against an fp64 reference at the per-rank widths of the 33B shape at TP = 8 / 4;
5. rejections;
6. a LLaMA engine with hidden 384 and ffn 608 in modes 2 and 3 against a twin bf16 engine on the dequantised weights.
"""
import pytest
import torch

from tests.fp4_common import BF16, _case, _gemv_profile, bfr, rel_err

pytestmark = pytest.mark.gpu

KS = [288, 384, 416, 480, 608, 896, 2240]          # kb = 1, 4, 5, 7, 3, 4, 6: one block, the ku = 0 half, the half boundary, the shards
MS = [1, 5, 8, 9, 16, 17, 33, 65, 130]             # thin <32,8,5> / <32,16,4>, GEMM 64 x 32 / 64 x 64 / 64 x 128 (two row tiles)


def _x(M, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, K, generator=g).to(BF16), g


def _extended(x, q, sc, K):
    """The problem at the next multiple of 256: code 0, scale byte 127, zero activations."""
    K2 = -(-K // 256) * 256
    M, N = x.shape[0], q.shape[0]
    x2 = torch.cat([x, torch.zeros(M, K2 - K, dtype=BF16, device=x.device)], 1).contiguous()
    q2 = torch.cat([q, torch.zeros(N, (K2 - K) // 2, dtype=torch.uint8, device=q.device)], 1).contiguous()
    sc2 = torch.cat([sc, torch.full((N, (K2 - K) // 32), 127, dtype=torch.uint8, device=sc.device)], 1).contiguous()
    return x2, q2, sc2


# ------------------------------------------------------------------------------------------------ 1. zero-extension identity
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K", KS)
def test_tail_equals_the_zero_extended_problem(M, K):
    from emu_amd import ops
    old = ops.linear_fp4w_thin if M <= 16 else ops.linear_fp4w_gemm
    for N in (37, 64):
        for epi in (ops.EPI_NONE, ops.EPI_RESID, ops.EPI_SWIGLU):
            n = 38 if epi == ops.EPI_SWIGLU and N == 37 else N
            q, sc, _ = _case(n, K)
            x, g = _x(M, K, 7 * M + n + K + epi)
            x = x.cuda()
            kw = dict(epi=epi)
            if epi == ops.EPI_RESID:
                kw["res"] = torch.randn(M, n, generator=g).to(BF16).cuda()
            got = ops.linear_fp4w_mfma(x, q, sc, **kw)
            want = old(*_extended(x, q, sc, K), **kw)
            assert got.shape == want.shape
            assert torch.equal(got, want), (M, n, K, epi, float((got != want).float().mean()))


# ------------------------------------------------------------------------------------------------ 2. position exactness
def test_one_hot_rows_in_the_partial_stage_pick_single_weights():
    from emu_amd import ops
    N, K, M = 37, 480, 224
    q, sc, wd = _case(N, K)
    x = torch.zeros(M, K, dtype=BF16)
    x[torch.arange(M), 256 + torch.arange(M)] = 1.0
    x = x.cuda()
    want = wd[:, 256:].T.contiguous()                                            # [m, n] = dequantised W[n, 256 + m], exact in bf16
    got = ops.linear_fp4w_mfma(x, q, sc).float().cpu()                           # the GEMM, 64 x 128 tiles
    assert torch.equal(got, want)
    thin = torch.cat([ops.linear_fp4w_mfma(x[r:r + 16].contiguous(), q, sc) for r in range(0, M, 16)]).float().cpu()
    assert torch.equal(thin, want)


# ------------------------------------------------------------------------------------------------ 3. poison
@pytest.mark.parametrize("M", [5, 40])
@pytest.mark.parametrize("K", [288, 2240])
def test_bytes_past_the_logical_widths_do_not_matter(M, K):
    from emu_amd import mxfp4, ops
    N = 37
    q, sc, _ = _case(N, K)
    x, _ = _x(M, K, 3 * M + K)
    tight = ops.linear_fp4w_mfma(x.cuda(), q, sc)
    qb = torch.full((N, K // 2 + 32), 0xFF, dtype=torch.uint8, device="cuda")
    qb[:, :K // 2] = q
    sb = torch.full((N, mxfp4.scale_stride(K) + 8), 0xFF, dtype=torch.uint8, device="cuda")      # the padding of the rule is NaN too
    sb[:, :K // 32] = sc
    xb = torch.full((M, K + 64), float("nan"), dtype=BF16, device="cuda")
    xb[:, :K] = x.cuda()
    qv, sv, xv = qb[:, :K // 2], sb[:, :K // 32], xb[:, :K]
    assert (qv.stride(0), sv.stride(0), xv.stride(0)) == (K // 2 + 32, mxfp4.scale_stride(K) + 8, K + 64)
    got = ops.linear_fp4w_mfma(xv, qv, sv)
    assert bool(torch.isfinite(got.float()).all())
    assert torch.equal(got, tight)


# ------------------------------------------------------------------------------------------------ 4. against fp64
@pytest.mark.parametrize("M", [5, 16, 20, 70])
@pytest.mark.parametrize("K", [896, 2240, 4480])
def test_tail_against_fp64(M, K):
    from emu_amd import ops
    N = 70
    q, sc, wd = _case(N, K)
    x, g = _x(M, K, M + N + K)
    res = torch.randn(M, N, generator=g).to(BF16)
    y = (x.double() @ wd.double().T).float()
    want = bfr(y)
    e1 = rel_err(ops.linear_fp4w_mfma(x.cuda(), q, sc), want)
    e2 = rel_err(ops.linear_fp4w_mfma(x.cuda(), q, sc, res=res.cuda(), epi=ops.EPI_RESID), bfr(want + res.float()))
    want_s = bfr(bfr(torch.nn.functional.silu(want[:, 0::2])) * want[:, 1::2])   # packed rows interleave gate / up
    got_s = ops.linear_fp4w_mfma(x.cuda(), q, sc, epi=ops.EPI_SWIGLU)
    assert got_s.shape == (M, N // 2)
    e3 = rel_err(got_s, want_s)
    print(f"fp4 tail M={M} N={N} K={K}: rel L2 plain {e1:.2e} resid {e2:.2e} SwiGLU {e3:.2e}")
    assert e1 < 4e-3
    assert e2 < 4e-3
    assert e3 < 8e-3


# ------------------------------------------------------------------------------------------------ 5. rejections
def test_fp4_mfma_rejections():
    from emu_amd import mxfp4, ops
    from emu_amd._lib import EmuHipError, lib

    def args(M, N, K):
        return (torch.zeros(M, K, dtype=BF16, device="cuda"), torch.zeros(N, K // 2, dtype=torch.uint8, device="cuda"),
                torch.full((N, K // 32), 127, dtype=torch.uint8, device="cuda"))
    for M in (1, 16, 17, 200):
        ops.linear_fp4w_mfma(*args(M, 64, 256))
        ops.linear_fp4w_mfma(*args(M, 64, 288))
    with pytest.raises(EmuHipError):
        ops.linear_fp4w_mfma(*args(5, 64, 128))                                  # K < 256
    x, q, sc = args(5, 64, 288)
    with pytest.raises(EmuHipError):                                             # K = 272 is no multiple of 32
        ops.linear_fp4w_mfma(x[:, :272].contiguous(), q[:, :136].contiguous(), sc)
    with pytest.raises(EmuHipError):
        ops.linear_fp4w_mfma(*args(20, 63, 288), epi=ops.EPI_SWIGLU)             # SwiGLU with odd N
    with pytest.raises(EmuHipError):
        ops.linear_fp4w_mfma(*args(20, 64, 288), epi=ops.EPI_RESID)              # residual epilogue without res
    sc34 = torch.full((64, 34), 127, dtype=torch.uint8, device="cuda")[:, :28]   # K = 896: wide enough (32), but lds % 4 != 0
    with pytest.raises(EmuHipError):
        ops.linear_fp4w_mfma(*args(5, 64, 896)[:2], sc34)
    # through the C ABI: the scale stride of the rule, and misaligned pointers
    M, N, K = 20, 64, 896
    x, q, _ = args(M + 1, N + 1, K)
    sc = torch.full((N + 1, mxfp4.scale_stride(K)), 127, dtype=torch.uint8, device="cuda")
    out = torch.empty(M, N, dtype=BF16, device="cuda")

    def call(xp, qp, sp, lds, rows=M):
        return lib().emu_linear_fp4w_mfma_bf16(xp, qp, sp, None, None, out.data_ptr(), rows, N, K, K, K // 2, lds, 0, N, ops.EPI_NONE,
                                               ops.stream(out))
    for rows in (5, M):
        assert call(x.data_ptr(), q.data_ptr(), sc.data_ptr(), 32, rows) == 0
        assert call(x.data_ptr(), q.data_ptr(), sc.data_ptr(), K // 32, rows) == -22     # 28: the last stage's window would leave the row
        assert call(x.data_ptr() + 2, q.data_ptr(), sc.data_ptr(), 32, rows) == -22
        assert call(x.data_ptr(), q.data_ptr() + 8, sc.data_ptr(), 32, rows) == -22
        assert call(x.data_ptr(), q.data_ptr(), sc.data_ptr() + 2, 32, rows) == -22
        assert call(x.data_ptr(), q.data_ptr(), sc.data_ptr(), 30, rows) == -22
    # the two older entry points keep refusing a partial stage, whatever the stride
    for sym, rows in (("emu_linear_fp4w_thin_bf16", 5), ("emu_linear_fp4w_gemm_bf16", M)):
        assert getattr(lib(), sym)(x.data_ptr(), q.data_ptr(), sc.data_ptr(), None, None, out.data_ptr(), rows, N, K, K, K // 2, 32, 0, N,
                                   ops.EPI_NONE, ops.stream(out)) == -22
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. engine
def _engines():
    """An engine and its twin on the same weights: every matrix already a dequantised MXFP4 matrix (quantising it again returns
    the same bytes), so the 4-bit kernels and the twin's bf16 kernels see the same numbers."""
    from emu_amd import mxfp4, synth
    from emu_amd.conf.emu_conf import LlamaCfg
    from emu_amd.llama import EmuHipContext, LlamaEngine
    l = LlamaCfg(hidden_size=384, intermediate_size=608, num_attention_heads=3, num_hidden_layers=2)
    items = []
    for name, t in synth.iter_synth(synth.llama_param_shapes(l, 64), device="cpu", dtype=BF16):
        if t.dim() == 2 and "embed_tokens" not in name:          # blocks run along K inside a row: they commute with the row packing
            t = mxfp4.dequantize(*mxfp4.quantize_rows(t)).to(BF16)
        items.append((name, t.cuda()))
    ctx = EmuHipContext(torch.device("cuda", 0))
    engs = []
    for _ in range(2):
        e = LlamaEngine(l, 64, ctx)
        e.load_weights(items)
        assert e.ready
        engs.append(e)
    return l, engs[0], engs[1]


def test_engine_modes_2_and_3_on_widths_that_are_no_multiple_of_256():
    """hidden 384 (qkv, gate/up and the head: 256 + 128), heads x head_dim 384 (o_proj), ffn 608 (down: 2 x 256 + 96).  Tolerances:
    those of tests/test_gpu_fp4_gemm.py::test_fp4_all_rows_equals_twin_engine (hidden states 2e-2) and of the oracle comparisons of
    the same modules (logits 2.5e-2)."""
    from emu_amd import mxfp4
    l, eng, twin = _engines()
    H, S, P, NB = l.hidden_size, 24, 4, 5
    g = torch.Generator().manual_seed(31)
    x1 = (torch.randn(1, S, H, generator=g) * 0.5).to(BF16).cuda()               # a 24-row prefill
    x5 = (torch.randn(5, S + 1, H, generator=g) * 0.5).to(BF16).cuda()           # 5 rows: prefill, then the cached step of a 5-beam search
    x4 = (torch.randn(P, S, H, generator=g) * 0.5).to(BF16).cuda()               # 4 prompts fanned out to 20 beam rows
    step_in = (torch.randn(P * NB, H, generator=g) * 0.5).to(BF16).cuda()
    ones = lambda b: torch.ones(b, S, dtype=torch.long)
    prompts = (torch.randn(3, 9, H, generator=g) * 0.5).to(BF16).cuda()          # greedy on 3 rows: every step is a thin-kernel step
    pmask = torch.ones(3, 9, dtype=torch.long)

    def record(e, profile=False):
        out, prof = {}, {}
        h, _, _ = e.prefill(x1, ones(1))
        out["prefill"], out["prefill_logits"] = h.reshape(S, H).clone(), e.logits(h.reshape(S, H).contiguous())
        _, kstart, pos = e.prefill(x5[:, :S].contiguous(), ones(5))

        def step5():
            out["step5"] = e.decode_embeds(x5[:, S].contiguous(), pos, S, kstart)
            out["step5_logits"] = e.logits(out["step5"])
        prof["step5"] = _gemv_profile(step5) if profile else step5()
        s_max = e.kv_capacity(S + 1)
        _, kstart, pos = e.prefill(x4, ones(P), s_max)
        e.fan_out_kv(P, NB, S, s_max)
        pos20, ks20 = pos.repeat_interleave(NB).contiguous(), kstart.repeat_interleave(NB).contiguous()

        def step20():
            out["step20"] = e.decode_embeds(step_in, pos20, S, ks20)
            out["step20_logits"] = e.logits(out["step20"])
        try:
            prof["step20"] = _gemv_profile(step20) if profile else step20()
        finally:
            e.set_kv_share(0, 0)
        return {k: v.cpu() for k, v in out.items()}, prof

    def greedy(e, graph):
        return e.greedy_generate(prompts, pmask, 6, use_graph=graph, stop_on_eos=False).cpu()
    want, _ = record(twin)
    mats = [eng._keep[f"{i}.{k}"] for i in range(l.num_hidden_layers) for k in eng._FP4_KINDS] + [eng.lm_head]
    bytes_4bit = sum(t.shape[0] * mxfp4.bytes_per_row(t.shape[1]) for t in mats)
    widths = sorted({t.shape[1] for t in mats})
    assert widths == [384, 608]
    # ---- mode 2: the 5-row step runs the thin kernel, everything wider stays bf16
    eng.use_fp4(True, wide=True)
    assert eng.fp4_wide and not eng.fp4_all
    for key in eng._fp4_keys():                                                  # registered at the padded stride; dequantisation unchanged
        q, sc = eng._fp4[key]
        assert sc.shape[1] == sc.stride(0) == mxfp4.scale_stride(q.shape[1] * 2)
        src = eng.lm_head if key == "lm_head" else eng._keep[key]
        assert torch.equal(eng.fp4_dequantized(key).to(BF16), src)
    got2, prof2 = record(eng, profile=True)
    assert prof2["step5"] == (bytes_4bit, len(mats))                             # every matrix once, at its 4-bit size: the 4-bit kernels ran
    assert greedy(eng, True).tolist() == greedy(eng, False).tolist()
    # ---- mode 3: the prefill, the 20-row step and their logits run the 4-bit GEMM
    eng.use_fp4(True, wide=True, all_rows=True)
    got3, prof3 = record(eng, profile=True)
    assert prof3["step5"] == (bytes_4bit, len(mats)) and prof3["step20"] == (bytes_4bit, len(mats))
    for name, got in (("mode 2", got2), ("mode 3", got3)):
        errs = {k: rel_err(got[k], want[k]) for k in want}
        print(f"fp4 tail engine, {name} vs the twin bf16 engine: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v < (2.5e-2 if k.endswith("logits") else 2e-2), (name, k, v)
    # ---- release_bf16 changes no output bit
    before, _ = record(eng)
    eager, graph = greedy(eng, False), greedy(eng, True)
    assert eager.tolist() == graph.tolist()
    eng.release_bf16()
    after, _ = record(eng)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert greedy(eng, False).tolist() == eager.tolist() and greedy(eng, True).tolist() == eager.tolist()
    assert eng.weight_bytes_per_token() == bytes_4bit
    assert tuple(eng.fp4_dequantized("0.wdown").shape) == (384, 608)


def test_narrow_model_is_still_refused_and_says_the_rule():
    from emu_amd import synth
    from emu_amd._lib import EmuHipError
    from emu_amd.conf.emu_conf import LlamaCfg
    from emu_amd.llama import EmuHipContext, LlamaEngine
    l = LlamaCfg(hidden_size=128, intermediate_size=256, num_attention_heads=1, num_hidden_layers=1)
    eng = LlamaEngine(l, 64, EmuHipContext(torch.device("cuda", 0)))
    eng.load_weights(synth.iter_synth(synth.llama_param_shapes(l, 64), device="cuda", dtype=BF16))
    with pytest.raises(EmuHipError, match="at least 256 that are multiples of 32"):
        eng.use_fp4(True, wide=True, all_rows=True)
