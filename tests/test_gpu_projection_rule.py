"""GPU: the engine asks the exported rule (emu_llama_projection_kernel) with the facts include/emu_hip.h documents.  One small engine
(hidden 256, ffn 512, 2 heads, 2 layers, vocabulary 1024; its packed sets made under emu_gemm_tune bit 17) under every weight mode at
1, 2, 5, 20 and 65 rows: the bytes and launches the weight-stream profiler counts over one forward plus logits must be the sum, over
the four projections of every layer and the head, of the price of the kernel the rule names for that matrix at that site."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
BLOCK_ONLY = 1 << 17                    # emu_gemm_tune: small matrices reach the block kernel's one-row forms (tests/test_gpu_bf16_pack.py)
NONE, RESID, SWIGLU = 0, 1, 2
H, HD, FL, VOCAB, LAYERS, S = 256, 256, 512, 1024, 2, 8
ROWS = (1, 2, 5, 20, 65)
# name -> (fp8 mode, fp4 mode, pack, pack_wide, the L2-warm mask as set)
CONFIGS = {
    "bf16": (0, 0, 0, 0, 0), "pack": (0, 0, 1, 0, 0), "pack+wide": (0, 0, 1, 1, 0), "pack, warm mask 1": (0, 0, 1, 0, 1),
    "fp8 1": (1, 0, 0, 0, 0), "fp8 3": (3, 0, 0, 0, 0), "fp8 5": (5, 0, 0, 0, 0), "fp8 6": (6, 0, 0, 0, 0),
    "fp4 1": (0, 1, 0, 0, 0), "fp4 2": (0, 2, 0, 0, 0), "fp4 3": (0, 3, 0, 0, 0),
}


@pytest.fixture(scope="module")
def engine():
    from emu_amd import synth
    from emu_amd._lib import lib
    from emu_amd.conf.emu_conf import LlamaCfg
    from emu_amd.llama import EmuHipContext, LlamaEngine
    cfg = LlamaCfg(hidden_size=H, intermediate_size=FL, num_attention_heads=2, num_hidden_layers=LAYERS)
    dev = torch.device("cuda", 0)
    eng = LlamaEngine(cfg, VOCAB, EmuHipContext(dev, 0, 1))
    eng.load_weights(synth.iter_synth(synth.llama_param_shapes(cfg, VOCAB), seed=3, device=dev, dtype=BF16))
    lib().emu_gemm_tune(BLOCK_ONLY)
    try:
        assert eng.pack_bf16(tune=BLOCK_ONLY)[0] == 4               # o_proj and down of both layers, two rows per group
        eng.quantize_fp8()
        yield eng
    finally:
        lib().emu_gemm_tune(0)


def price(kernel, rows, N, K, set_rows):
    """(bytes, launches) of one launch of `kernel` over [N, K] under the weight-stream profiler (include/emu_hip.h)."""
    from emu_amd import bf16pack
    if kernel == 0:
        return (2 * N * K, 1) if rows <= 8 else (0, 0)              # the stream; 20 and 65 rows: the GEMM
    if kernel in (1, 7, 9):
        return N * K, 1
    if kernel in (3, 4, 5):
        return N * (K // 2 + K // 32), 1
    if kernel in (6, 8):
        return bf16pack.packed_bytes(N, K, set_rows), 1
    assert kernel == 2
    return 0, 0


def expected(eng, L, config, rows):
    from emu_amd._lib import ProjectionC
    fp8, fp4, pack, wide, warm = CONFIGS[config]
    call = L.emu_llama_weight_kernel(fp8, fp4, rows, H, HD, FL)
    norm = int(call in (1, 3) or rows == 1)                        # what the forward fuses into the qkv and gate/up streams
    plan_warm = warm if rows == 1 and call == 0 else 0             # the boundaries the default one-row bf16 step carries
    sites = [(f"{i}.{key}", N, K, n, epi, 0, plan_warm) for i in range(LAYERS)
             for key, N, K, n, epi in (("wqkv", 3 * HD, H, norm, NONE), ("wo", H, HD, 0, RESID), ("wgu", 2 * FL, H, norm, SWIGLU), ("wdown", H, FL, 0, RESID))]
    sites.append(("lm_head", VOCAB, H, 0, NONE, 1, warm))
    total, launches = 0, 0
    for key, N, K, n, epi, head, warm_mask in sites:
        set_rows = eng._pack[key]["rows"] if key in eng._pack else 0
        q = ProjectionC(fp8=fp8, fp4=fp4, pack=pack, pack_wide=wide, rows=rows, hidden=H, heads_dim_local=HD, ffn_local=FL, N=N, K=K, norm=n,
                        epi=epi, has_fp8=1, pack_rows=set_rows, set_n=N if set_rows else 0, set_k=K if set_rows else 0, warm_mask=warm_mask,
                        tune=BLOCK_ONLY, head=head, ws_fits=1)
        k = L.emu_llama_projection_kernel(C.byref(q))
        assert 0 <= k <= 9, (key, k)
        b, n_launch = price(k, rows, N, K, set_rows)
        total, launches = total + b, launches + n_launch
    return total, launches


def measured(eng, L, rows):
    from emu_amd._lib import check
    g = torch.Generator().manual_seed(rows)
    x = (torch.randn(rows, S + 1, H, generator=g) * 0.1).to(BF16).to(eng.device)
    _, kstart, pos = eng.prefill(x[:, :S].contiguous(), torch.ones(rows, S, dtype=torch.long), eng.kv_capacity(S + 8))
    check(L.emu_profile_gemv(1), "emu_profile_gemv")
    try:
        eng.logits(eng.decode_embeds(x[:, S].contiguous(), pos, S, kstart))
        torch.cuda.synchronize()
        ms, wb, nl = C.c_double(), C.c_double(), C.c_long()
        check(L.emu_profile_gemv_read(C.byref(ms), C.byref(wb), C.byref(nl)), "emu_profile_gemv_read")
    finally:
        L.emu_profile_gemv(0)
    return wb.value, nl.value


@pytest.mark.parametrize("config", list(CONFIGS))
def test_profiler_counts_what_the_exported_rule_prices(engine, config):
    from emu_amd._lib import lib
    eng, L = engine, lib()
    fp8, fp4, pack, wide, warm = CONFIGS[config]
    eng.use_fp8(False)
    eng.use_fp4(False)
    eng.use_bf16_pack(bool(pack))
    eng.use_bf16_pack_wide(bool(wide))
    eng.set_l2_warm(warm)
    if fp8:
        eng.use_fp8(True, prefill=fp8 == 6, wide=fp8 >= 3, mid=fp8 >= 5)
    if fp4:
        eng.use_fp4(True, wide=fp4 >= 2, all_rows=fp4 == 3)
    seen = {rows: (measured(eng, L, rows), expected(eng, L, config, rows)) for rows in ROWS}
    print(config, seen)
    for rows, (got, want) in seen.items():
        assert got == want, (config, rows, got, want)
