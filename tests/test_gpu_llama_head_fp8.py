"""GPU: the LLaMA head under ``use_fp8(True, prefill=True)``.  The layers' rule (csrc/engine.hip: weight_kernel) names the W8A8 GEMM
for 17 rows and more in that mode, and the head has none: it must run the bf16 head there, the fp8 stream for 1..2 rows and bf16 in
between.  Engine logits == the same kernel called through ``ops`` on the same rows, bit for bit, at the smallest shape the kernels
take (hidden 256, 2 heads of 128, ffn 256, 2 layers; every width a multiple of 128, so the mode's GEMM rule applies; a vocabulary
that is no multiple of 64)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def fp8_prefill_engine():
    from emu_amd import synth
    from emu_amd.conf.emu_conf import LlamaCfg
    from emu_amd.llama import EmuHipContext, LlamaEngine
    cfg = LlamaCfg(hidden_size=256, intermediate_size=256, num_attention_heads=2, num_hidden_layers=2)
    eng = LlamaEngine(cfg, 160, EmuHipContext(torch.device("cuda", 0)))
    eng.load_weights(synth.iter_synth(synth.llama_param_shapes(cfg, 160), seed=5, device="cuda", dtype=BF16))
    eng.use_fp8(True, prefill=True)
    yield eng
    eng.use_fp8(False)


@pytest.mark.parametrize("rows", [1, 2, 3, 16, 17])
def test_head_in_fp8_prefill_mode_runs_the_documented_kernel(fp8_prefill_engine, rows):
    from emu_amd import ops
    eng = fp8_prefill_engine
    g = torch.Generator().manual_seed(rows)
    h = (torch.randn(rows, eng.cfg.hidden_size, generator=g) * 0.5).to(BF16).cuda()
    got = eng.logits(h)
    if rows <= 2:                                    # the e4m3 copy of the head, the final RMSNorm fused into the stream
        q, sc = eng._fp8["lm_head"]
        want = ops.linear_fp8w(h, q, sc, norm_w=eng.final_norm, eps=eng.cfg.rms_norm_eps)
    else:                                            # the bf16 head on the normalised rows.  (At 17 rows the rule says Fp8Gemm and
        # llama_head demotes it to bf16; linear_w serves no Fp8Gemm and would answer -22, so logits() returning at all is the proof.)
        want = ops.linear(ops.rmsnorm(h, eng.final_norm, eng.cfg.rms_norm_eps), eng.lm_head)
    assert got.shape == (rows, 160) and bool(torch.isfinite(got.float()).all())
    assert torch.equal(got, want)
