"""GPU tests of the few-row fp8 weight stream on the matrix cores (csrc/gemv_fp8_thin.hip, ``ops.linear_fp8w_thin``,
``LlamaEngine.use_fp8(True, wide=True)``): steps of 3..16 rows -- the default 5-beam search, batches, contrastive search.

Every e4m3 value is exact in bf16, so the MFMA sees exact weights: (a) the decode of every finite code at every byte position of a
stage through the conversion and the MFMA, exactly, for 16 and for 32 weight rows per workgroup; (b) the linear with its epilogues
against the fp64 product with the dequantised weights at the bounds tests/test_gpu_fp8.py uses for the same arithmetic; (c) the
refusals; (d) an engine step of 5 and of 16 rows against the CPU oracle, with a witness that the fp8 bytes were what streamed, and
mode 1 unchanged; (e) 5-beam search against itself, its captured graph and a twin engine holding the dequantised weights as bf16.
"""
import pytest
import torch

from tests import tiny
from tests.fp4_common import BF16, _f32, _gemv_profile, rel_err
from tests.test_gpu_fp8 import tiny_fp8  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu
E4M3 = torch.float8_e4m3fn


# ------------------------------------------------------------------------------------------------ (a) decode, exact
@pytest.fixture
def pinned_rows():
    """emu_gemm_tune bits 28-29: 1 / 2 = 16 / 32 weight rows per workgroup; back to the heuristic afterwards."""
    from emu_amd._lib import lib

    def pin(v):
        lib().emu_gemm_tune(v << 28)
    yield pin
    lib().emu_gemm_tune(0)


@pytest.mark.parametrize("pin,rows", [(1, 16), (2, 32)])
def test_decode_every_code_at_every_byte_position(pinned_rows, pin, rows):
    """N = 64, K = 512 (two stages), M = 16.  Row n holds code (n + 64 (k // 16) + 37 (k % 16)) mod 254 of the 254 finite e4m3 codes
    at column k, so every code meets every byte of a 16-byte chunk and every column of a stage holds 64 codes.  Activation rows are
    one-hot (+-1, +-2^-3), 16 columns per call: each output is ONE product, bf16(fp32(code) * x * scale), whatever the summation
    order.  Pins the byte select of the conversion, the A / B k pairing, both swizzles and the scale's place."""
    import ctypes as C
    from emu_amd import _lib, ops
    N, K = 64, 512
    finite = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8)      # 0x7F / 0xFF are NaN
    assert finite.numel() == 254
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    idx = (n + 64 * (k // 16) + 37 * (k % 16)) % 254
    w8 = finite[idx]
    for j in range(16):                                                       # every code at every byte of a chunk, every column in use
        assert torch.unique(w8[:, j::16]).numel() == 254
    wf = w8.view(E4M3).float()
    assert bool(torch.isfinite(wf).all()) and torch.equal(wf.to(BF16).float(), wf)
    scale = torch.tensor([1.0, 0.5, 0.37, 2.0, 1.7, 0.013, 4.0, 0.0625, 0.9, 3.3, 0.25, 1.1, 8.0, 0.61, 0.125, 0.77]).repeat(N // 16)
    vals = torch.tensor([1.0, -1.0, 0.125, -0.125])
    xval = vals[(torch.arange(K) % 16 + torch.arange(K) // 16) % 4]
    want = ((wf.t() * xval[:, None]) * scale[None, :]).to(BF16)              # [K, N], fp32 in the kernel's order
    p = _lib.GemvFp8ThinPlanC()
    assert _lib.lib().emu_gemv_fp8_thin_plan(16, N, K, K, K, 0, pin << 28, C.byref(p)) == 0 and p.rows == rows
    pinned_rows(pin)
    w_d, s_d = w8.cuda(), scale.cuda()
    x = torch.zeros(K, K)
    x[torch.arange(K), torch.arange(K)] = xval
    x = x.to(BF16).cuda()
    got = torch.cat([ops.linear_fp8w_thin(x[k0:k0 + 16], w_d, s_d) for k0 in range(0, K, 16)]).cpu()
    assert torch.equal(got, want)


def test_identity_weight_returns_the_scaled_rows():
    """W8 = the identity (code 0x38 = 1.0), mixed row scales, random x: out == bf16(x * scale) exactly."""
    from emu_amd import ops
    N = K = 256
    w8 = torch.zeros(N, K, dtype=torch.uint8)
    w8[torch.arange(N), torch.arange(N)] = 0x38
    g = torch.Generator().manual_seed(3)
    scale = torch.where(torch.arange(N) % 3 == 0, torch.tensor(0.5), torch.rand(N, generator=g) + 0.2)
    x = torch.randn(16, K, generator=g).to(BF16)
    got = ops.linear_fp8w_thin(x.cuda(), w8.cuda(), scale.cuda()).cpu()
    assert torch.equal(got, (x.float() * scale[None, :]).to(BF16))


# ------------------------------------------------------------------------------------------------ (b) linear parity
_CASE8 = {}


def _case8(N, K, seed_extra=0):
    """Weights, their fp8 bytes and row scales on the device and the exact dequantisation in fp64, once per shape."""
    from emu_amd import ops
    key = (N, K, seed_extra)
    if key not in _CASE8:
        g = torch.Generator().manual_seed(N * 3 + K + seed_extra)
        w = (torch.randn(N, K, generator=g) * 0.03).to(BF16)
        q, sc = ops.quantize_fp8_rows(w.cuda())
        _CASE8[key] = (q, sc, (q.cpu().view(E4M3).float() * sc.cpu()[:, None]).double())
    return _CASE8[key]


@pytest.mark.parametrize("M", [3, 5, 8, 9, 16])
@pytest.mark.parametrize("N,K", [(16, 256), (37, 512), (1000, 6656), (64, 17920)])
def test_linear_fp8w_thin_plain_and_resid(M, N, K):
    from emu_amd import ops
    q, sc, wd = _case8(N, K)
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(BF16)
    res = torch.randn(M, N, generator=g).to(BF16)
    want = x.double() @ wd.T
    e1 = rel_err(ops.linear_fp8w_thin(x.cuda(), q, sc), want)
    e2 = rel_err(ops.linear_fp8w_thin(x.cuda(), q, sc, res=res.cuda(), epi=ops.EPI_RESID), want + res.double())
    print(f"fp8 thin M={M} N={N} K={K}: rel L2 plain {e1:.2e} resid {e2:.2e}")
    assert e1 < 4e-3
    assert e2 < 4e-3


def test_linear_fp8w_thin_bias():
    from emu_amd import ops
    N, K, M = 300, 512, 5
    q, sc, wd = _case8(N, K)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, K, generator=g).to(BF16)
    bias = torch.randn(N, generator=g).to(BF16)
    e = rel_err(ops.linear_fp8w_thin(x.cuda(), q, sc, bias=bias.cuda()), x.double() @ wd.T + bias.double())
    print(f"fp8 thin bias: rel L2 {e:.2e}")
    assert e < 4e-3


@pytest.mark.parametrize("M", [5, 16])
@pytest.mark.parametrize("N,K", [(38, 512), (2240, 6656)])
def test_linear_fp8w_thin_swiglu(M, N, K):
    from emu_amd import ops
    q, sc, wd = _case8(N, K, 1)
    g = torch.Generator().manual_seed(11 + M + N)
    x = torch.randn(M, K, generator=g).to(BF16)
    y = x.double() @ wd.T
    want = torch.nn.functional.silu(y[:, 0::2]) * y[:, 1::2]                  # packed rows interleave gate / up
    got = ops.linear_fp8w_thin(x.cuda(), q, sc, epi=ops.EPI_SWIGLU)
    assert got.shape == (M, N // 2)
    e = rel_err(got, want)
    print(f"fp8 thin SwiGLU M={M} N={N} K={K}: rel L2 {e:.2e}")
    assert e < 8e-3


@pytest.mark.parametrize("M,N,K", [(5, 32274, 256), (1, 1000, 6656), (2, 1000, 6656)])
def test_linear_fp8w_thin_head_rows_and_one_or_two_rows(M, N, K):
    """The head's N = 32 274 (no multiple of 16 or 32: the last workgroup's rows are clamped and dropped), and M = 1 / 2, which the
    kernel takes although the engine sends them to the VALU stream."""
    from emu_amd import ops
    q, sc, wd = _case8(N, K)
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(BF16)
    e = rel_err(ops.linear_fp8w_thin(x.cuda(), q, sc), x.double() @ wd.T)
    print(f"fp8 thin M={M} N={N} K={K}: rel L2 {e:.2e}")
    assert e < 4e-3


# ------------------------------------------------------------------------------------------------ (c) refusals
def test_fp8_thin_refusals_leave_the_output_untouched():
    from emu_amd import ops
    from emu_amd._lib import lib

    def args(M, N, K, ldw=None):
        w = torch.zeros(N, ldw or K, dtype=torch.uint8, device="cuda")[:, :K]
        return torch.ones(M, K, dtype=BF16, device="cuda"), w, torch.ones(N, dtype=torch.float32, device="cuda")
    ops.linear_fp8w_thin(*args(16, 64, 256))
    ops.linear_fp8w_thin(*args(1, 64, 256))
    for M, N, K, ldw, msg in ((5, 64, 384, None, "multiple of 256"), (5, 64, 128, None, "multiple of 256"), (17, 64, 256, None, "1..16 rows"),
                              (5, 64, 256, 264, "16-byte")):
        x, w, sc = args(M, N, K, ldw)
        out = torch.full((M, N), 1.5, dtype=BF16, device="cuda")
        with pytest.raises(ValueError, match=msg):
            ops.linear_fp8w_thin(x, w, sc, out=out)
        # the library itself, past the wrapper's checks: -22, nothing launched
        st = lib().emu_linear_fp8w_thin_bf16(x.data_ptr(), w.data_ptr(), sc.data_ptr(), 0, 0, out.data_ptr(), M, N, K, x.stride(0),
                                             w.stride(0), 0, out.stride(0), ops.EPI_NONE, ops.stream(x))
        assert st == -22
        torch.cuda.synchronize()
        assert bool((out == 1.5).all())
    x, w, sc = args(3, 64, 256)
    from emu_amd._lib import EmuHipError
    with pytest.raises(EmuHipError):
        ops.linear_fp8w(x, w, sc)                                               # the VALU stream still ends at two rows


def test_use_fp8_wide_rejects_widths_not_multiple_of_256():
    from emu_amd import synth
    from emu_amd._lib import EmuHipError
    from emu_amd.conf.emu_conf import LlamaCfg
    from emu_amd.llama import EmuHipContext, LlamaEngine
    l = LlamaCfg(hidden_size=256, intermediate_size=384, num_attention_heads=2, num_hidden_layers=1)
    eng = LlamaEngine(l, 64, EmuHipContext(torch.device("cuda", 0)))
    eng.load_weights(synth.iter_synth(synth.llama_param_shapes(l, 64), device="cuda", dtype=BF16))
    assert eng.ready
    with pytest.raises(EmuHipError, match="multiples of 256"):
        eng.use_fp8(True, wide=True)
    assert not getattr(eng, "fp8_wide", False) and not getattr(eng, "fp8_decode", False)
    eng.use_fp8(True)                                                            # mode 1 takes multiples of 16
    assert eng.fp8_decode and not eng.fp8_wide
    with pytest.raises(EmuHipError, match="multiples of 256"):
        eng.use_fp8(True, prefill=True, wide=True)
    assert eng.fp8_decode and not eng.fp8_wide
    eng.use_fp8(False)


# ------------------------------------------------------------------------------------------------ engine
def _fp8_mats(lm, layers):
    return [lm._keep[f"{i}.{k}"] for i in range(layers) for k in ("wqkv", "wo", "wgu", "wdown")] + [lm.lm_head]


@pytest.mark.parametrize("B", [5, 16])
def test_fp8_wide_step_matches_oracle_and_streams_the_fp8_set(tiny_fp8, B):                  # (d)
    """bf16 prefill of B rows, then ONE cached single-token step of B rows through the wide fp8 stream == the oracle's step on the
    dequantised weights (the bounds of tests/test_gpu_fp8.py); the GEMV profiler counts exactly the fp8 bytes of the layers' matrices
    and the head -- without the stream these rows read the bf16 bytes."""
    from oracle import emu2_ref as R
    m, W, W8, cfg = tiny_fp8
    lm = m.decoder.lm
    g = torch.Generator().manual_seed(5 + B)
    S = 24
    x = (torch.randn(B, S + 1, cfg.llama.hidden, generator=g) * 0.5).to(BF16)
    mask = torch.ones(B, S, dtype=torch.long)
    cache = R.KVCache(cfg.llama.layers)
    xf = x.float()
    R.llama_model(xf[:, :S].to(BF16), mask, R.cast_weights(W, BF16), cfg.llama, cache=cache, final_norm=False)
    mask1 = torch.ones(B, S + 1, dtype=torch.long)
    want = R.llama_model(xf[:, S:], mask1, R.cast_weights(W8, torch.float32), cfg.llama, cache=_f32(cache), final_norm=False)[:, 0]
    out = {}

    def step():
        out["h"] = lm.decode_embeds(x[:, S].contiguous().cuda(), pos, S, kstart)
        out["l"] = lm.logits(out["h"])
    try:
        lm.use_fp8(True, wide=True)
        assert lm.fp8_wide and lm.fp8_decode
        _, kstart, pos = lm.prefill(x[:, :S].contiguous().cuda(), mask)
        wb, nl = _gemv_profile(step)
    finally:
        lm.use_fp8(False)
    assert not lm.fp8_wide and not lm.fp8_decode
    e_h = rel_err(out["h"], want)
    h = R.rms_norm(want, W["decoder.lm.model.norm.weight"].float(), cfg.llama.rms_eps)
    e_l = rel_err(out["l"], h @ W8["decoder.lm.lm_head.weight"].T)
    print(f"fp8 wide step B={B} vs oracle: hidden {e_h:.2e}, logits {e_l:.2e}; profiler {wb:.0f} bytes in {nl} launches")
    assert e_h < 2e-2
    assert e_l < 2.5e-2
    mats = _fp8_mats(lm, cfg.llama.layers)
    assert wb == sum(t.numel() for t in mats) and nl == len(mats)               # the fp8 bytes, one launch per matrix
    assert wb != sum(t.numel() * 2 for t in mats)


def test_fp8_narrow_mode_leaves_five_row_steps_on_bf16(tiny_fp8):                             # (d) mode 1 unchanged
    """With wide=False a 5-row step is bit-identical to the same step with fp8 off, and streams the bf16 bytes."""
    m, W, W8, cfg = tiny_fp8
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
        lm.use_fp8(True)
        assert lm.fp8_decode and not lm.fp8_wide
        h1, l1, wb1 = run()
    finally:
        lm.use_fp8(False)
    assert torch.equal(h0, h1) and torch.equal(l0, l1)
    assert wb0 == wb1 == sum(t.numel() * 2 for t in _fp8_mats(lm, cfg.llama.layers))


def test_fp8_wide_beam_search_equals_itself_its_graph_and_a_twin_engine(tiny_fp8, golden_dir):   # (e)
    """5-beam search through the wide fp8 stream: twice the same ids; the run replayed from the captured graph the same ids; and
    against a twin engine that holds the dequantised weights as bf16 and runs the bf16 stream (prefill sees the same weights in both)
    a row may diverge only at a step where the twin's own gap between the accumulated scores of the two continuations is below 0.08
    (the rule of tests/test_gpu_fp4_wide.py::test_fp4_wide_beam_search_equals_twin_engine).  Switching the stream off restores the
    bf16 beam ids and the golden ids of the margin fixture."""
    from emu_amd import EmuModel, TextDecoderCfg
    m, W, W8, cfg = tiny_fp8
    z = tiny.load(golden_dir, "generate_tiny.npz")
    v, l, vocab, _ = tiny.weights_from(z)
    ids, mask = torch.from_numpy(z["ids2"]), torch.from_numpy(z["mask2"])
    n_new = 6
    kw = dict(max_new_tokens=n_new, num_beams=5, hf_semantics="5.x")
    m8 = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda")
    m8.load_state_dict(W8, strict=True)
    twin = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda")
    twin.load_state_dict(W8, strict=True)
    lm8 = m8.decoder.lm
    try:
        lm8.use_fp8(True, wide=True)
        got = m8.generate_ids(ids, mask, None, **kw).cpu()
        again = m8.generate_ids(ids, mask, None, **kw).cpu()
        m8.use_graph = True
        graph = m8.generate_ids(ids, mask, None, **kw).cpu()
    finally:
        m8.use_graph = False
        lm8.use_fp8(False)
    assert got.tolist() == again.tolist()
    assert got.tolist() == graph.tolist()
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
        lm.use_fp8(True, wide=True)
        m.generate_ids(ids, mask, None, **kw)
    finally:
        lm.use_fp8(False)
    assert m.generate_ids(ids, mask, None, **kw).cpu().tolist() == before.tolist()
    zm = tiny.load(golden_dir, "generate_margin_tiny.npz")
    b5 = m.generate_ids(torch.from_numpy(zm["b5_ids"]), torch.from_numpy(zm["b5_mask"]), torch.from_numpy(zm["image"]).cuda(),
                        max_new_tokens=int(zm["b5_n_new"]), num_beams=5, hf_semantics="5.x")
    assert b5.cpu().tolist() == zm["b5_new"].tolist()
