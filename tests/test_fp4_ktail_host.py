"""Host-side checks of the MXFP4 matrix-core kernels' partial last K stage (no GPU): the new entry point in the binding and the
public header, the scale row stride rule and its padding helper, the per-rank reduction widths of the 33B shape at TP = 1 / 2 / 4 / 8,
and the ABI version, which an added symbol leaves alone."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mfma_symbol_has_the_thin_streams_prototype():
    from emu_amd import _lib
    protos = next(v for v in vars(_lib).values() if isinstance(v, dict) and "emu_version" in v)
    assert protos["emu_linear_fp4w_mfma_bf16"] == protos["emu_linear_fp4w_thin_bf16"]
    header = open(os.path.join(ROOT, "include", "emu_hip.h")).read()

    def params(name):
        m = re.search(r"^int " + name + r"\((.*?)\);", header, re.M | re.S)
        assert m, name
        return " ".join(m.group(1).split())
    assert params("emu_linear_fp4w_mfma_bf16") == params("emu_linear_fp4w_thin_bf16")


def test_abi_version_is_still_6():
    from emu_amd import _lib
    assert _lib.ABI_VERSION == 6
    src = open(os.path.join(ROOT, "emu_amd", "csrc", "engine.hip")).read()
    assert re.search(r"int emu_version\(void\) \{ return 6; \}", src)


@pytest.mark.parametrize("K,stride", [(256, 8), (288, 16), (896, 32), (2240, 72), (4480, 144), (6656, 208)])
def test_scale_stride(K, stride):
    from emu_amd import mxfp4
    assert mxfp4.scale_stride(K) == stride
    assert stride % 4 == 0 and stride >= K // 32 and stride >= 8 * (-(-K // 256))     # whole stages of 8 bytes, 4-byte DMA
    # the C side states the same rule
    src = open(os.path.join(ROOT, "emu_amd", "csrc", "kernels.h")).read()
    assert "inline int fp4_scale_stride(int K) { return K % 256 == 0 ? K / 32 : 8 * ((K + 255) / 256); }" in src


@pytest.mark.parametrize("K", [256, 288, 896, 2240])
def test_pad_scales_round_trips(K):
    from emu_amd import mxfp4
    g = torch.Generator().manual_seed(K)
    sc = torch.randint(0, 255, (5, K // 32), generator=g, dtype=torch.uint8)
    p = mxfp4.pad_scales(sc, K)
    assert p.dtype == torch.uint8 and tuple(p.shape) == (5, mxfp4.scale_stride(K)) and p.is_contiguous()
    assert torch.equal(p[:, :K // 32], sc)
    assert bool((p[:, K // 32:] == 127).all())
    q = torch.randint(0, 256, (5, K // 2), generator=g, dtype=torch.uint8)
    assert torch.equal(mxfp4.dequantize(q, p[:, :K // 32]), mxfp4.dequantize(q, sc))    # dequantize keeps taking [N, K/32]
    with pytest.raises(ValueError):
        mxfp4.pad_scales(sc[:, :-1], K)
    with pytest.raises(ValueError):
        mxfp4.pad_scales(sc.to(torch.int32), K)


@pytest.mark.parametrize("tp", [1, 2, 4, 8])
def test_33b_shard_widths_are_multiples_of_32_from_256_up(tp):
    from emu_amd.conf.emu_conf import LlamaCfg
    from emu_amd.tp import ShardPlan
    l = LlamaCfg()
    for rank in (0, tp - 1):
        p = ShardPlan(l.hidden_size, l.num_attention_heads, l.head_dim, l.intermediate_size, tp, rank)
        widths = {"hidden": l.hidden_size, "o_proj": p.heads_local * l.head_dim, "down": p.ffn_local}
        for name, K in widths.items():
            assert K % 32 == 0 and K >= 256, (tp, name, K)
    if tp == 8:
        assert (widths["o_proj"], widths["down"]) == (896, 2240)                          # 3 x 256 + 128, 8 x 256 + 192
    if tp == 4:
        assert widths["down"] == 4480                                                     # 17 x 256 + 128
