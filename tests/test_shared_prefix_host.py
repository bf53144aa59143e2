"""CPU: the host side of candidate ranking on a shared prefix -- ``scoring.two_segment_attention`` (the specification of the
two-segment flash kernel) against plain masked softmax attention, ``scoring.shared_prefix_plan`` against the cache shapes the
engine allocates, and the refusals of ``LlamaEngine.score_continuations(share_prefix=True)`` before any device work."""
import itertools
import types

import pytest
import torch

from emu_amd import scoring
from emu_amd.llama import LlamaEngine


def plain_attention(q, kp, vp, ko, vo, kstart, scale):
    """softmax(q [prefix ; own]^T * scale + mask) [prefix ; own] with ONE mask over the concatenated keys: left padding ``kstart``
    and causal on the own part."""
    B, Sq, H, D = q.shape
    P, Sk = kp.shape[0], ko.shape[1]
    k = torch.cat([kp[None].expand(B, -1, -1, -1), ko], dim=1)
    v = torch.cat([vp[None].expand(B, -1, -1, -1), vo], dim=1)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    key = torch.arange(P + Sk)[None, :]
    i = torch.arange(Sq)[:, None]
    ok = (key >= kstart) & (key <= i + (P + Sk - Sq))
    s = s.masked_fill(~ok[None, None], float("-inf"))
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), v)


@pytest.mark.parametrize("P", (1, 63, 64, 65))
def test_specification_equals_plain_attention_on_the_concatenated_keys(P):
    g = torch.Generator().manual_seed(100 + P)
    B, H, D = 3, 2, 16
    for Sq, extra, kstart in itertools.product((1, 5), (0, 3), sorted({0, P - 1})):
        Sk = Sq + extra
        q, ko, vo = (torch.randn(B, n, H, D, generator=g, dtype=torch.float64) for n in (Sq, Sk, Sk))
        kp, vp = (torch.randn(P, H, D, generator=g, dtype=torch.float64) for _ in range(2))
        got = scoring.two_segment_attention(q, kp, vp, ko, vo, kstart, 0.25)
        want = plain_attention(q, kp, vp, ko, vo, kstart, 0.25)
        assert got.dtype == torch.float64 and got.shape == (B, Sq, H, D)
        assert float((got - want).abs().max()) <= 1e-12, (P, Sq, Sk, kstart)


def test_specification_refuses_what_the_kernel_refuses():
    z = torch.zeros
    for kstart, Sq, Sk in ((-1, 2, 2), (4, 2, 2), (0, 3, 2)):
        with pytest.raises(ValueError):
            scoring.two_segment_attention(z(1, Sq, 1, 8), z(4, 1, 8), z(4, 1, 8), z(1, Sk, 1, 8), z(1, Sk, 1, 8), kstart, 1.0)


def _engine_capacity():
    """The product's bucket rule on a stand-in with LLaMA-33B's position limit."""
    eng = types.SimpleNamespace(cfg=types.SimpleNamespace(max_position_embeddings=2048), KV_BUCKETS=LlamaEngine.KV_BUCKETS)
    return lambda need: LlamaEngine.kv_capacity(eng, need)


def test_plan_reproduces_the_33b_numbers():
    """64 candidates of 8 tokens behind an 800-token prompt, 60 layers x 52 heads x 128: one slot of one row is 1.6 MB, the copying
    route's cache 105 GB with 82 GB copied into it, the shared route's two caches 1.6 GB each."""
    cap = _engine_capacity()
    p = scoring.shared_prefix_plan(64, 800, [8], 60, 52, 128, cap)
    assert p["slot_bytes"] == 2 * 60 * 52 * 128 * 2 == 1597440
    assert p["prefix_capacity"] == cap(808) == 1024 and p["prefix_shape"] == (60, 1, 52, 1024, 128)
    assert p["prefix_bytes"] == 1024 * 1597440                                    # 1.6 GB
    (seg,) = p["segments"]
    assert seg["rows"] == 64 and seg["width"] == 8 and seg["suffix_capacity"] == 16
    assert seg["suffix_shape"] == (60, 64, 52, 16, 128) and seg["shared_bytes"] == 64 * 16 * 1597440       # 1.6 GB
    # what fan_out_kv allocates (rows x kv_capacity slots, K and V) and copies (rows x S slots)
    assert seg["unshared_shape"] == (60, 64, 52, cap(808), 128)
    assert seg["unshared_bytes"] == 2 * 2 * torch.Size(seg["unshared_shape"]).numel() == 64 * 1024 * 1597440
    assert round(seg["unshared_bytes"] / 1e9) == 105 and round(seg["copy_bytes"] / 1e9) == 82
    assert round(seg["shared_bytes"] / 1e9, 1) == round(p["prefix_bytes"] / 1e9, 1) == 1.6
    assert p["shared_peak_bytes"] == p["prefix_bytes"] + seg["shared_bytes"]
    assert p["unshared_peak_bytes"] == p["prefix_bytes"] + seg["unshared_bytes"]


def test_plan_capacities_and_segments():
    cap = _engine_capacity()
    for w in range(1, 70):
        c = scoring.suffix_capacity(w)
        assert c >= max(16, w) and c & (c - 1) == 0 and (c == 16 or c // 2 < w)
    p = scoring.shared_prefix_plan(7, 70, [3, 33], 2, 2, 128, cap)               # segments of 3 and 4 rows (split_segments)
    assert [g["rows"] for g in p["segments"]] == [3, 4] == [b - a for a, b in scoring.split_segments(7, 2)]
    assert [g["suffix_capacity"] for g in p["segments"]] == [16, 64]
    assert p["prefix_capacity"] == cap(70 + 33) == 256
    assert p["shared_peak_bytes"] == p["prefix_bytes"] + 4 * 64 * p["slot_bytes"]
    with pytest.raises(ValueError):
        scoring.shared_prefix_plan(4, 10, [], 2, 2, 128, cap)
    with pytest.raises(ValueError):
        scoring.shared_prefix_plan(4, 10, [0], 2, 2, 128, cap)


class _NoDevice:
    """A stand-in engine on which every attribute but the ones the refusals read raises: nothing on the device is called."""

    def __init__(self, head_dim=128, tp_size=1):
        object.__setattr__(self, "cfg", types.SimpleNamespace(hidden_size=32, head_dim=head_dim, max_position_embeddings=2048))
        object.__setattr__(self, "ctx", types.SimpleNamespace(tp_size=tp_size))
        object.__setattr__(self, "vocab", 100)
        object.__setattr__(self, "SCORE_MAX_ROWS", LlamaEngine.SCORE_MAX_ROWS)

    _score_args = LlamaEngine._score_args

    def __getattr__(self, name):
        raise AssertionError(f"score_continuations touched engine.{name} before refusing")


@pytest.mark.parametrize("kw, eng, what", [
    (dict(via="decode"), dict(), "via='prefill' only"),
    (dict(), dict(tp_size=2), "tensor-parallel"),
    (dict(), dict(head_dim=64), "head_dim 128"),
])
def test_share_prefix_refusals_come_before_any_device_work(kw, eng, what):
    x, mask = torch.zeros(1, 5, 32), torch.ones(1, 5, dtype=torch.long)
    cand = torch.ones(4, 3, dtype=torch.long)
    with pytest.raises(ValueError, match=what):
        LlamaEngine.score_continuations(_NoDevice(**eng), x, mask, cand, None, share_prefix=True, **kw)
    # the same calls without the option get past the refusals (and then reach for the device)
    with pytest.raises(AssertionError, match="touched engine"):
        LlamaEngine.score_continuations(_NoDevice(**eng), x, mask, cand, None, **kw)


def test_emu1_predict_forwards_the_option_and_leaves_the_default_call_as_it_was():
    from emu_amd.emu1 import Emu
    from tests.test_scoring_host import _Tok

    class Lm:
        def __init__(self):
            self.kw = []

        def embed_tokens(self, ids):
            return torch.zeros(*ids.shape, 8)

        def score_continuations(self, x, mask, cand_ids, cand_mask, **kw):
            self.kw.append(kw)
            return -(cand_ids.float() + 1.0) / 10.0 * cand_mask, cand_mask.clone()

    m = Emu.__new__(Emu)
    m.lm, m.ctx, m.tokenizer = Lm(), types.SimpleNamespace(device=torch.device("cpu")), _Tok()
    ids, mask = torch.ones(1, 5, dtype=torch.int64), torch.ones(1, 5, dtype=torch.int64)
    cand, cmask = torch.tensor([[4, 0], [1, 1]]), torch.tensor([[1, 0], [1, 1]], dtype=torch.bool)
    m.predict_ids(ids, mask, None, cand, cmask)
    assert "share_prefix" not in m.lm.kw[-1]
    m.predict_ids(ids, mask, None, cand, cmask, share_prefix=True)
    assert m.lm.kw[-1]["share_prefix"] is True and m.lm.kw[-1]["hf_generate_positions"] is False
    ranks = m.predict({"prompt": ["3 4"], "image": None}, ["7 8", "2"], share_prefix=True)
    assert m.lm.kw[-1]["share_prefix"] is True and ranks.shape == (1, 2)
    m.predict({"prompt": ["3 4"], "image": None}, ["7 8", "2"])
    assert "share_prefix" not in m.lm.kw[-1]
