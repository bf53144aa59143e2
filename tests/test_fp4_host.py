"""CPU tests of the MXFP4 weight format (emu_amd/mxfp4.py: the definition the HIP kernels are pinned against) and of the host
arithmetic around the optional fp4 decode stream."""
import os
import re

import pytest
import torch

from emu_amd import mxfp4

BF16 = torch.bfloat16
GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def block(vals, fill=0.0):
    """One [1, 32] row whose first elements are ``vals``."""
    w = torch.full((1, 32), fill, dtype=torch.float32)
    w[0, :len(vals)] = torch.tensor(vals, dtype=torch.float32)
    return w


def codes_of(w):
    p, s = mxfp4.quantize_rows(w)
    return mxfp4.unpack_codes(p)[0].tolist(), s[0].tolist()


def test_every_code_is_produced_and_decoded():
    vals = GRID + [-v for v in GRID]                       # amax = 6 -> e = 0, scale byte 127
    codes, sc = codes_of(block(vals))
    assert sc == [127]
    assert codes[:16] == list(range(16))                   # magnitude index, sign bit 8 (-0 keeps its sign: code 8)
    p, s = mxfp4.quantize_rows(block(vals))
    d = mxfp4.dequantize(p, s)
    assert torch.equal(d[0, :16], torch.tensor(vals))
    assert bool(torch.signbit(d[0, 8]))                    # -0 decodes to -0
    assert torch.equal(mxfp4.decode_codes(torch.arange(16, dtype=torch.uint8)), torch.tensor(vals))


def test_ties_go_to_the_even_code():
    # midpoints of the grid under scale 1 (a 6 in the block pins e = 0)
    mids = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0, 2, 2, 4, 4, 6, 6]
    codes, sc = codes_of(block([6.0] + mids + [-m for m in mids]))
    assert sc == [127]
    assert codes[1:8] == want
    assert codes[8:15] == [c | 8 for c in want]
    # just off the midpoints: nearest wins
    eps = 2.0 ** -12
    codes, _ = codes_of(block([6.0] + [m + eps for m in mids] + [m - eps for m in mids]))
    assert codes[1:8] == [1, 2, 3, 4, 5, 6, 7]
    assert codes[8:15] == [0, 1, 2, 3, 4, 5, 6]


def test_values_between_6_and_8_saturate():
    for amax in (6.5, 7.0, 7.96875):
        for k in (-20, 0, 9):
            codes, sc = codes_of(block([amax * 2.0 ** k, -amax * 2.0 ** k, 4.0 * 2.0 ** k]))
            assert sc == [127 + k]                         # amax / 2^e in [4, 8)
            assert codes[:3] == [7, 15, 6]


def test_zero_block_and_scale_rule():
    p, s = mxfp4.quantize_rows(torch.zeros(2, 64))
    assert s.tolist() == [[127, 127], [127, 127]] and int(p.max()) == 0
    w = torch.zeros(1, 64)
    w[0, 0] = -0.0
    w[0, 40] = 3.0                                         # floor(log2 3) = 1 -> e = -1
    p, s = mxfp4.quantize_rows(w)
    assert s.tolist() == [[127, 126]]
    c = mxfp4.unpack_codes(p)[0]
    assert int(c[0]) == 8 and int(c[40]) == 7              # 3 / 2^-1 = 6
    for amax, e in ((1.0, -2), (1.99, -2), (2.0, -1), (4.0, 0), (0.02, -8), (448.0, 6)):
        assert codes_of(block([amax]))[1] == [127 + e], amax


def test_exponent_clamps_at_both_ends():
    big = torch.finfo(torch.float32).max
    codes, sc = codes_of(block([big, -big, 2.0 ** 127]))
    assert sc == [252] and codes[:3] == [7, 15, 6]         # e = 125: never byte 253..255
    bigb = torch.tensor([[float(torch.finfo(BF16).max)] + [0.0] * 31]).to(BF16)
    assert mxfp4.quantize_rows(bigb)[1].tolist() == [[252]]
    # small end: e stops at -126, smaller values round on that grid (0.5 * 2^-126 is the smallest non-zero magnitude)
    tiny = [2.0 ** -124, 2.0 ** -125, 2.0 ** -126, 2.0 ** -127, 2.0 ** -128, 2.0 ** -129, 2.0 ** -133]
    for lead in range(len(tiny)):
        codes, sc = codes_of(block(tiny[lead:]))
        assert sc == [1]
        want = [6, 4, 2, 1, 0, 0, 0][lead:]               # 4, 2, 1, 0.5, 0.25 (tie -> 0), ... in units of 2^-126
        assert codes[:len(want)] == want
    d = mxfp4.dequantize(*mxfp4.quantize_rows(block(tiny)))
    assert d[0, :4].tolist() == tiny[:4] and d[0, 4:7].tolist() == [0.0, 0.0, 0.0]
    p, s = mxfp4.quantize_rows(torch.randn(4, 96) * 1e-3)
    assert int(s.max()) < 255


def test_pack_unpack_round_trip():
    g = torch.Generator().manual_seed(0)
    codes = torch.randint(0, 16, (5, 64), generator=g, dtype=torch.uint8)
    p = mxfp4.pack_codes(codes)
    assert p.shape == (5, 32) and p.dtype == torch.uint8
    assert torch.equal(mxfp4.unpack_codes(p), codes)
    assert int(p[0, 0]) == int(codes[0, 0]) | (int(codes[0, 1]) << 4)      # element 2j low nibble, 2j + 1 high nibble
    allb = torch.arange(256, dtype=torch.uint8).reshape(1, 256)
    assert torch.equal(mxfp4.pack_codes(mxfp4.unpack_codes(allb)), allb)


@pytest.mark.parametrize("sigma", [0.02, 1.0, 3e-30, 1e30])
def test_dequantised_values_are_bf16_and_requantise_to_the_same_bytes(sigma):
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(64, 512, generator=g) * sigma).to(BF16)
    w[3, 32:64] = 0
    p, s = mxfp4.quantize_rows(w)
    assert p.shape == (64, 256) and s.shape == (64, 16) and p.dtype == s.dtype == torch.uint8
    d = mxfp4.dequantize(p, s)
    assert d.dtype == torch.float32
    assert torch.equal(d.to(BF16).float().view(torch.int32), d.view(torch.int32))        # bit for bit through bf16
    p2, s2 = mxfp4.quantize_rows(d.to(BF16))
    assert torch.equal(p2, p) and torch.equal(s2, s)
    p3, s3 = mxfp4.quantize_rows(d)                                                       # fp32 input: same bytes
    assert torch.equal(p3, p) and torch.equal(s3, s)


def test_gaussian_round_trip_error_is_the_documented_one():
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(256, 6656, generator=g) * 0.02).to(BF16)
    d = mxfp4.dequantize(*mxfp4.quantize_rows(w))
    rel = float((d - w.float()).norm() / w.float().norm())
    assert 0.10 < rel < 0.13, rel                          # 0.114 in the issue and the docs


def test_rejects_non_finite_and_bad_shapes():
    w = torch.zeros(2, 64)
    w[1, 5] = float("inf")
    with pytest.raises(ValueError):
        mxfp4.quantize_rows(w)
    w[1, 5] = float("nan")
    with pytest.raises(ValueError):
        mxfp4.quantize_rows(w)
    with pytest.raises(ValueError):
        mxfp4.quantize_rows(torch.zeros(2, 48))
    with pytest.raises(ValueError):
        mxfp4.dequantize(torch.zeros(2, 16, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.uint8))


def test_module_does_not_import_the_oracle():
    src = open(mxfp4.__file__).read()
    assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M)


def test_weight_bytes_per_token_counts_elements_and_scales():
    from emu_amd.llama import LlamaEngine
    eng = LlamaEngine.__new__(LlamaEngine)
    H, HD, F, V = 256, 256, 512, 1000
    eng._keep = {"0.wqkv": torch.empty(3 * HD, H, dtype=BF16), "0.wo": torch.empty(H, HD, dtype=BF16),
                 "0.wgu": torch.empty(2 * F, H, dtype=BF16), "0.wdown": torch.empty(H, F, dtype=BF16),
                 "0.ln1": torch.empty(H, dtype=BF16), "0.ln2": torch.empty(H, dtype=BF16)}
    eng.lm_head = torch.empty(V, H, dtype=BF16)
    weights = 3 * HD * H + H * HD + 2 * F * H + H * F + V * H
    assert eng.weight_bytes_per_token() == 2 * weights
    eng.fp8_decode = True
    assert eng.weight_bytes_per_token() == weights
    eng.fp8_decode, eng.fp4_decode = False, True
    rows_k = [(3 * HD, H), (H, HD), (2 * F, H), (H, F), (V, H)]
    want = sum(n * (k // 2 + k // 32) for n, k in rows_k)
    assert eng.weight_bytes_per_token() == want
    assert want * 32 == weights * 17                       # 0.53125 byte per weight
    eng.fp4_decode = False
    assert eng.weight_bytes_per_token() == 2 * weights


@pytest.mark.parametrize("tp", [1, 2, 4, 8])
def test_real_config_shard_widths_are_whole_blocks(tp):
    """Blocks never straddle a shard: every reduction width of every rank's packed matrices is a multiple of 32."""
    from emu_amd.conf.emu_conf import LlamaCfg
    from emu_amd.tp import ShardPlan
    c = LlamaCfg()
    assert (c.hidden_size, c.intermediate_size) == (6656, 17920)
    for rank in range(tp):
        p = ShardPlan(c.hidden_size, c.num_attention_heads, c.head_dim, c.intermediate_size, tp, rank)
        for k in (c.hidden_size, p.heads_local * c.head_dim, p.ffn_local):
            assert k % 32 == 0, (tp, rank, k)


def test_fp4_calls_are_declared_and_bound():
    from emu_amd import _lib
    names = ["emu_quantize_mxfp4_rows", "emu_linear_fp4w_bf16", "emu_llama_set_layer_fp4", "emu_llama_set_head_fp4", "emu_llama_use_fp4"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "emu_hip.h")).read()
    protos = next(v for v in vars(_lib).values() if isinstance(v, dict) and "emu_linear_fp8w_bf16" in v)
    for n in names:
        assert n in protos, n
        assert re.search(r"\b%s\s*\(" % n, header), n
