"""GPU tests of running LLaMA from the fp8 weights alone: the 64 x 128 form of the W8A16 GEMM for 65 rows and more
(csrc/gemm_fp8.hip, ``ops.linear_fp8w_tile``), ``LlamaEngine.use_fp8(True, wide=True, mid=True, all_rows=True)``, ``release_bf16``
under it and ``load_fp8``.

Every e4m3 value is exact in bf16 and the new form walks k as the 64-row form does, so: (a) the decode of every finite code at every
byte position, exactly, on one row tile per call, on two, and on ragged rows; (b) the identity weight; (c) the same bits as
``ops.linear_fp8w_gemm`` on every whole 64-row block; (d) the linear with its epilogues against the fp64 product with the dequantised
weights at the bounds tests/test_gpu_fp8_mid.py holds the same arithmetic to; (e) the refusals; (f) prefill and logits under mode 5 +
all_rows against the CPU oracle with a witness that the fp8 bytes were what streamed; (g) the switch off changes nothing; (h) mode 6 +
all_rows; (i) ``release_bf16``; (j) ``load_fp8``; (k) the vocabulary-sharded head.
"""
import pytest
import torch

from tests.fp4_common import BF16, _gemv_profile, _tiny_model, rel_err
from tests.test_gpu_fp8 import tiny_fp8  # noqa: F401 (the fixture)
from tests.test_gpu_fp8_mid import _decode_case, _run_step, _step_inputs
from tests.test_gpu_fp8_wide import _case8, _fp8_mats

pytestmark = pytest.mark.gpu

ALL = dict(wide=True, mid=True, all_rows=True)


# ------------------------------------------------------------------------------------------------ (a) decode, exact
def _plan(M, N, K):
    import ctypes as C
    from emu_amd import _lib
    p = _lib.GemmFp8tPlanC()
    assert _lib.lib().emu_gemm_fp8t_plan(M, N, K, K, K, 0, 0, C.byref(p)) == 0 and p.form == 3
    return p


@pytest.mark.parametrize("M,row_tiles", [(128, 1), (256, 2)])
def test_decode_every_code_at_every_byte_position(M, row_tiles):
    """Four calls of one row tile each, two calls of two row tiles each (m0 = 128 in the second workgroup)."""
    from emu_amd import ops
    d = _decode_case()
    assert _plan(M, 64, d["K"]).grid_x == row_tiles
    got = torch.cat([ops.linear_fp8w_tile(d["x"][k0:k0 + M], d["w"], d["s"]) for k0 in range(0, d["K"], M)]).cpu()
    assert torch.equal(got, d["want"])


def test_decode_every_code_ragged_rows():
    """M = 65 per call (the last call ends at row 512 by overlapping the one before): rows clamped on load, masked on store."""
    from emu_amd import ops
    d = _decode_case()
    K, M = d["K"], 65
    got = torch.full((K, 64), 7.0, dtype=BF16, device="cuda")
    for k0 in list(range(0, K - M, M)) + [K - M]:
        ops.linear_fp8w_tile(d["x"][k0:k0 + M], d["w"], d["s"], out=got[k0:k0 + M])
    assert torch.equal(got.cpu(), d["want"])


def test_identity_weight_returns_the_scaled_rows():                            # (b)
    """W8 = the identity (code 0x38 = 1.0), mixed row scales, random x, M = 200: out == bf16(x * scale) exactly."""
    from emu_amd import ops
    N = K = 256
    w8 = torch.zeros(N, K, dtype=torch.uint8)
    w8[torch.arange(N), torch.arange(N)] = 0x38
    g = torch.Generator().manual_seed(3)
    scale = torch.where(torch.arange(N) % 3 == 0, torch.tensor(0.5), torch.rand(N, generator=g) + 0.2)
    x = torch.randn(200, K, generator=g).to(BF16)
    got = ops.linear_fp8w_tile(x.cuda(), w8.cuda(), scale.cuda()).cpu()
    assert torch.equal(got, (x.float() * scale[None, :]).to(BF16))


# ------------------------------------------------------------------------------------------------ (c) the 64-row form's bits
@pytest.mark.parametrize("M,N,K,epi", [(128, 37, 512, "none"), (128, 37, 512, "resid"), (300, 1000, 6656, "none"),
                                       (300, 1000, 6656, "resid"), (130, 38, 512, "swiglu")])
def test_same_bits_as_the_64_row_form(M, N, K, epi):
    """Rows [r0, r0 + 64) of the tile call == ``linear_fp8w_gemm`` on those rows, for every whole 64-row block: a row's result does
    not depend on how many rows share the call."""
    from emu_amd import ops
    q, sc, _ = _case8(N, K, 1 if epi == "swiglu" else 0)
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(BF16).cuda()
    res = torch.randn(M, N, generator=g).to(BF16).cuda()
    kw = {"none": {}, "resid": dict(epi=ops.EPI_RESID), "swiglu": dict(epi=ops.EPI_SWIGLU)}[epi]
    got = ops.linear_fp8w_tile(x, q, sc, res=res if epi == "resid" else None, **kw)
    assert got.shape == (M, N // 2 if epi == "swiglu" else N)
    blocks = list(range(0, M - 63, 64))
    assert len(blocks) == M // 64 >= 2
    for r0 in blocks:
        want = ops.linear_fp8w_gemm(x[r0:r0 + 64], q, sc, res=res[r0:r0 + 64] if epi == "resid" else None, **kw)
        assert torch.equal(got[r0:r0 + 64], want), (r0, float((got[r0:r0 + 64].float() - want.float()).abs().max()))


# ------------------------------------------------------------------------------------------------ (d) linear parity
@pytest.mark.parametrize("M", [65, 128, 129, 300])
@pytest.mark.parametrize("N,K", [(16, 256), (37, 512), (1000, 6656), (64, 17920)])
def test_linear_fp8w_tile_plain_and_resid(M, N, K):
    from emu_amd import ops
    q, sc, wd = _case8(N, K)
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(BF16)
    res = torch.randn(M, N, generator=g).to(BF16)
    want = x.double() @ wd.T
    e1 = rel_err(ops.linear_fp8w_tile(x.cuda(), q, sc), want)
    e2 = rel_err(ops.linear_fp8w_tile(x.cuda(), q, sc, res=res.cuda(), epi=ops.EPI_RESID), want + res.double())
    print(f"fp8 tile M={M} N={N} K={K}: rel L2 plain {e1:.2e} resid {e2:.2e}")
    assert e1 < 4e-3
    assert e2 < 4e-3


def test_linear_fp8w_tile_bias():
    from emu_amd import ops
    N, K, M = 300, 512, 70
    q, sc, wd = _case8(N, K)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, K, generator=g).to(BF16)
    bias = torch.randn(N, generator=g).to(BF16)
    e = rel_err(ops.linear_fp8w_tile(x.cuda(), q, sc, bias=bias.cuda()), x.double() @ wd.T + bias.double())
    print(f"fp8 tile bias: rel L2 {e:.2e}")
    assert e < 4e-3


@pytest.mark.parametrize("M", [65, 300])
@pytest.mark.parametrize("N,K", [(38, 512), (2240, 6656)])
def test_linear_fp8w_tile_swiglu(M, N, K):
    from emu_amd import ops
    q, sc, wd = _case8(N, K, 1)
    g = torch.Generator().manual_seed(11 + M + N)
    x = torch.randn(M, K, generator=g).to(BF16)
    y = x.double() @ wd.T
    want = torch.nn.functional.silu(y[:, 0::2]) * y[:, 1::2]                  # packed rows interleave gate / up
    got = ops.linear_fp8w_tile(x.cuda(), q, sc, epi=ops.EPI_SWIGLU)
    assert got.shape == (M, N // 2)
    e = rel_err(got, want)
    print(f"fp8 tile SwiGLU M={M} N={N} K={K}: rel L2 {e:.2e}")
    assert e < 8e-3


def test_linear_fp8w_tile_head_rows():
    """The head's N = 32 274 (no multiple of 64: the last column tile's rows are clamped and dropped) at 70 rows."""
    from emu_amd import ops
    M, N, K = 70, 32274, 256
    q, sc, wd = _case8(N, K)
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(BF16)
    e = rel_err(ops.linear_fp8w_tile(x.cuda(), q, sc), x.double() @ wd.T)
    print(f"fp8 tile M={M} N={N} K={K}: rel L2 {e:.2e}")
    assert e < 4e-3


# ------------------------------------------------------------------------------------------------ (e) refusals
def test_fp8_tile_refusals_leave_the_output_untouched():
    from emu_amd import ops
    from emu_amd._lib import lib

    def args(M, N, K, ldw=None):
        w = torch.zeros(N, ldw or K, dtype=torch.uint8, device="cuda")[:, :K]
        return torch.ones(M, K, dtype=BF16, device="cuda"), w, torch.ones(N, dtype=torch.float32, device="cuda")
    ops.linear_fp8w_tile(*args(65, 64, 256))
    for M, N, K, ldw, msg in ((64, 64, 256, None, "65 rows"), (70, 64, 384, None, "multiple of 256"), (70, 64, 256, 264, "16-byte")):
        x, w, sc = args(M, N, K, ldw)
        out = torch.full((M, N), 1.5, dtype=BF16, device="cuda")
        with pytest.raises(ValueError, match=msg):
            ops.linear_fp8w_tile(x, w, sc, out=out)
        # the library itself, past the wrapper's checks: -22, nothing launched
        st = lib().emu_linear_fp8w_tile_bf16(x.data_ptr(), w.data_ptr(), sc.data_ptr(), 0, 0, out.data_ptr(), M, N, K, x.stride(0),
                                             w.stride(0), 0, out.stride(0), ops.EPI_NONE, ops.stream(x))
        assert st == -22
        torch.cuda.synchronize()
        assert bool((out == 1.5).all())


def test_use_fp8_all_rows_needs_mid_and_widths_that_are_multiples_of_256(tiny_fp8):
    from emu_amd import synth
    from emu_amd._lib import EmuHipError
    from emu_amd.conf.emu_conf import LlamaCfg
    from emu_amd.llama import EmuHipContext, LlamaEngine
    lm = tiny_fp8[0].decoder.lm
    with pytest.raises(ValueError, match="mid=True"):
        lm.use_fp8(True, wide=True, all_rows=True)
    assert not lm.fp8_all and not lm.fp8_mid and not lm.fp8_decode
    l = LlamaCfg(hidden_size=256, intermediate_size=384, num_attention_heads=2, num_hidden_layers=1)
    eng = LlamaEngine(l, 64, EmuHipContext(torch.device("cuda", 0)))
    eng.load_weights(synth.iter_synth(synth.llama_param_shapes(l, 64), device="cuda", dtype=BF16))
    assert eng.ready
    eng.use_fp8(True)                                                            # mode 1 takes multiples of 16
    with pytest.raises(EmuHipError, match="multiples of 256"):
        eng.use_fp8(True, **ALL)
    assert eng.fp8_decode and not eng.fp8_wide and not eng.fp8_mid and not eng.fp8_all      # the previous mode stays
    with pytest.raises(RuntimeError, match="all_rows"):
        eng.release_bf16()
    eng.use_fp8(False)


# ------------------------------------------------------------------------------------------------ engine
def _prefill_inputs(B, S, hidden, pad, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, S, hidden, generator=g) * 0.5).to(BF16)
    mask = torch.ones(B, S, dtype=torch.long)
    if pad:
        mask[1, :pad] = 0                                                        # left padding on row 1
    return x, mask


def _prefill_and_logits(lm, x, mask):
    B, S = mask.shape
    h, _, _ = lm.prefill(x.cuda(), mask)
    lg = lm.logits(h.reshape(B * S, -1).contiguous())
    return h.cpu(), lg.view(B, S, -1).cpu()


@pytest.mark.parametrize("B,S,pad", [(1, 72, 0), (2, 40, 7)])
def test_fp8_all_rows_prefill_matches_oracle_and_streams_the_fp8_set(tiny_fp8, B, S, pad):   # (f)
    """A prefill of 72 / 80 rows under mode 5 + all_rows == the oracle's prefill on the dequantised weights (padded rows are
    don't-care), logits of ALL rows through the fp8 head included.  The weight-stream profiler, which prices the fp8 streams and no
    bf16 GEMM, saw one launch per matrix and exactly the fp8 bytes: no projection ran on bf16."""
    from oracle import emu2_ref as R
    m, W, W8, cfg = tiny_fp8
    lm = m.decoder.lm
    x, mask = _prefill_inputs(B, S, cfg.llama.hidden, pad, 31 + B)
    want = R.llama_model(x.float(), mask, R.cast_weights(W8, torch.float32), cfg.llama, final_norm=False)
    out = {}
    try:
        lm.use_fp8(True, **ALL)
        assert lm.fp8_all and lm.fp8_mid and lm.fp8_wide and lm.fp8_decode
        wb, nl = _gemv_profile(lambda: out.update(zip("hl", _prefill_and_logits(lm, x, mask))))
    finally:
        lm.use_fp8(False)
    assert not lm.fp8_all and not lm.fp8_decode
    ok = mask.bool()
    e_h = rel_err(out["h"][ok], want[ok])
    hn = R.rms_norm(want, W["decoder.lm.model.norm.weight"].float(), cfg.llama.rms_eps)
    e_l = rel_err(out["l"][ok], (hn @ W8["decoder.lm.lm_head.weight"].T)[ok])
    print(f"fp8 all_rows prefill {B} x {S} vs oracle: hidden {e_h:.2e}, logits {e_l:.2e}; profiler {wb:.0f} bytes in {nl} launches")
    assert e_h < 2e-2
    assert e_l < 2.5e-2
    mats = _fp8_mats(lm, cfg.llama.layers)
    assert wb == sum(t.numel() for t in mats) and nl == len(mats)               # the fp8 bytes, one launch per matrix
    assert wb != sum(t.numel() * 2 for t in mats)


def test_fp8_switch_off_changes_nothing(tiny_fp8):                                           # (g)
    """Mode 5 without all_rows: the 72-row prefill and its logits are bit-identical to the same engine with fp8 off.  Mode 5 +
    all_rows: a 20-row step (behind a 60-row prefill, which both modes run on the 17..64-row form) is bit-identical to mode 5's and
    streams the same fp8 bytes."""
    m, W, W8, cfg = tiny_fp8
    lm = m.decoder.lm
    x, mask = _prefill_inputs(1, 72, cfg.llama.hidden, 0, 41)
    x20, mask20, S = _step_inputs(20, cfg.llama.hidden, 9, S=3)
    off = _prefill_and_logits(lm, x, mask)
    try:
        lm.use_fp8(True, wide=True, mid=True)
        assert lm.fp8_mid and not lm.fp8_all
        mid = _prefill_and_logits(lm, x, mask)
        s5 = _run_step(lm, x20, mask20, S)
        lm.use_fp8(True, **ALL)
        assert lm.fp8_all
        s5a = _run_step(lm, x20, mask20, S)
        lm.use_fp8(True, wide=True, mid=True)
        assert not lm.fp8_all                                                    # ... and the switch goes off again
        again = _prefill_and_logits(lm, x, mask)
    finally:
        lm.use_fp8(False)
    assert torch.equal(off[0], mid[0]) and torch.equal(off[1], mid[1])
    assert torch.equal(off[0], again[0]) and torch.equal(off[1], again[1])
    mats = _fp8_mats(lm, cfg.llama.layers)
    assert torch.equal(s5[0], s5a[0]) and torch.equal(s5[1], s5a[1]) and s5[2:] == s5a[2:] == (sum(t.numel() for t in mats), len(mats))


def test_fp8_mode_6_all_rows_keeps_the_w8a8_layers_and_runs_the_fp8_head(tiny_fp8):          # (h)
    """Mode 6 + all_rows: the 72-row prefill's hidden states are bit-identical to mode 6 alone (the layers keep the W8A8 GEMMs, which
    the profiler does not price); the head, which has no W8A8 GEMM, streams exactly its N * K fp8 bytes in one launch, and its
    logits follow rms_norm(hidden) @ W8 head^T computed in fp32 from the GPU's own hidden rows."""
    from oracle import emu2_ref as R
    m, W, W8, cfg = tiny_fp8
    lm = m.decoder.lm
    x, mask = _prefill_inputs(1, 72, cfg.llama.hidden, 0, 43)
    out = {}
    try:
        lm.use_fp8(True, prefill=True, wide=True, mid=True)
        h6, _ = _prefill_and_logits(lm, x, mask)
        lm.use_fp8(True, prefill=True, **ALL)
        assert lm.fp8_all
        wb, nl = _gemv_profile(lambda: out.update(zip("hl", _prefill_and_logits(lm, x, mask))))
    finally:
        lm.use_fp8(False)
    assert torch.equal(out["h"], h6)
    assert (wb, nl) == (lm.lm_head.numel(), 1)
    hn = R.rms_norm(out["h"].float(), W["decoder.lm.model.norm.weight"].float(), cfg.llama.rms_eps)
    e_l = rel_err(out["l"], hn @ W8["decoder.lm.lm_head.weight"].T)
    print(f"fp8 mode 6 + all_rows, 72-row logits vs fp32 on the GPU's hidden rows: {e_l:.2e}")
    assert e_l < 2.5e-2


@pytest.mark.parametrize("prefill", [False, True])
def test_release_bf16_under_fp8(golden_dir, prefill):                                        # (i)
    """``release_bf16`` under mode 5 / 6 + all_rows frees the bf16 matrices and changes nothing that runs: the same kernels read
    the same fp8 pointers."""
    from tests import tiny
    from emu_amd._lib import EmuHipError
    m, v, l, vocab, W = _tiny_model(golden_dir)
    lm = m.decoder.lm
    z = tiny.load(golden_dir, "generate_tiny.npz")
    ids, mask = torch.from_numpy(z["ids2"]), torch.from_numpy(z["mask2"])
    H = lm.cfg.hidden_size
    x, xmask = _prefill_inputs(1, 72, H, 0, 24)
    x5, mask5, S = _step_inputs(5, H, 25, S=3)
    x20, mask20, _ = _step_inputs(20, H, 26, S=3)
    lm.use_fp8(True, prefill=prefill, wide=True, mid=True)
    with pytest.raises(RuntimeError, match="all_rows"):
        lm.release_bf16()                                                        # needs the switch
    lm.use_fp8(True, prefill=prefill, **ALL)

    def record():
        h, lg = _prefill_and_logits(lm, x, xmask)
        m.use_graph = False
        eager = m.generate_ids(ids, mask, None, max_new_tokens=6, stop_on_eos=False).cpu()
        m.use_graph = True
        graph = m.generate_ids(ids, mask, None, max_new_tokens=6, stop_on_eos=False).cpu()
        m.use_graph = False
        h5, l5 = _run_step(lm, x5, mask5, S)[:2]                                 # the five rows of a 5-beam step
        h20, l20 = _run_step(lm, x20, mask20, S)[:2]                             # four prompts x five beams
        beams = m.generate_ids(ids, mask, None, max_new_tokens=4, num_beams=5, hf_semantics="5.x").cpu()
        return h, lg, eager, graph, h5, l5, h20, l20, beams
    before = record()
    assert before[2].tolist() == before[3].tolist()
    bytes_fp8 = sum(q.numel() for q, _ in lm._fp8.values())
    released = sum(t.numel() * 2 for k, t in lm._keep.items() if k.split(".")[1] in lm._FP4_KINDS) + lm.lm_head.numel() * 2
    assert released == 2 * bytes_fp8
    head_shape = tuple(lm.lm_head.shape)
    torch.cuda.synchronize()
    mem0 = torch.cuda.memory_allocated()
    lm.release_bf16()
    torch.cuda.synchronize()
    mem1 = torch.cuda.memory_allocated()
    print(f"release_bf16 under fp8: {released} bytes of bf16 matrices, memory_allocated fell by {mem0 - mem1}")
    assert mem0 - mem1 >= released
    assert lm.lm_head is None and not any(k.split(".")[1] in lm._FP4_KINDS for k in lm._keep) and lm.ready and lm.bf16_released
    assert lm.weight_bytes_per_token() == bytes_fp8
    assert tuple(lm.fp8_dequantized("lm_head").shape) == head_shape and tuple(lm._fp4_source("lm_head").shape) == head_shape
    for refused in (lambda: lm.use_fp8(False), lambda: lm.use_fp8(True), lambda: lm.use_fp8(True, prefill=True),
                    lambda: lm.use_fp8(True, wide=True), lambda: lm.use_fp8(True, wide=True, mid=True),
                    lambda: lm.use_fp8(True, prefill=True, wide=True, mid=True), lambda: lm.use_fp4(), lambda: lm.use_fp4(False),
                    lambda: lm.use_fp4(True, wide=True, all_rows=True), lambda: lm.set_decode_fused(1),
                    lambda: lm.use_bf16_pack(True), lambda: lm.use_bf16_pack_wide(True)):
        with pytest.raises(EmuHipError, match="release"):
            refused()
    with pytest.raises(RuntimeError, match="release"):                           # a direct call says what happened, no KeyError
        lm.quantize_fp8()
    with pytest.raises(RuntimeError, match="release"):
        lm.pack_bf16()
    assert lm.fp8_all and lm.fp8_mid and lm.fp8_decode and not lm.fp4_decode and lm.decode_fused == 0
    after = record()                                                             # still runs: prefill, logits, eager and graph greedy, steps, beams
    assert after[2].tolist() == after[3].tolist()
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    # the other all_rows mode is still there, and the way back
    lm.use_fp8(True, prefill=not prefill, **ALL)
    assert lm.fp8_all
    h, lg = _prefill_and_logits(lm, x, xmask)
    assert bool(torch.isfinite(h.float()).all()) and bool(torch.isfinite(lg.float()).all())
    lm.use_fp8(True, prefill=prefill, **ALL)
    h, lg = _prefill_and_logits(lm, x, xmask)
    assert torch.equal(h, before[0]) and torch.equal(lg, before[1])


def test_load_fp8_registers_external_tensors(tiny_fp8, golden_dir):                          # (j)
    """A second engine is handed the first engine's fp8 tensors key by key: nothing is quantised anew, and the 72-row prefill, its
    logits and a 5-row step under mode 5 + all_rows are the first engine's bit for bit."""
    m, W, W8, cfg = tiny_fp8
    lm = m.decoder.lm
    lm.quantize_fp8()
    m2, *_ = _tiny_model(golden_dir)
    lm2 = m2.decoder.lm
    H = cfg.llama.hidden
    x, mask = _prefill_inputs(1, 72, H, 0, 51)
    x5, mask5, S = _step_inputs(5, H, 52, S=3)
    with pytest.raises(ValueError, match="must be"):
        lm2.load_fp8("lm_head", lm._fp8["lm_head"][0].view(torch.int8), lm._fp8["lm_head"][1])
    with pytest.raises(ValueError, match="must be"):
        lm2.load_fp8("lm_head", lm._fp8["lm_head"][0], lm._fp8["lm_head"][1].double())
    with pytest.raises(ValueError, match="must be"):
        lm2.load_fp8("0.wo", lm._fp8["0.wo"][0][:-1], lm._fp8["0.wo"][1][:-1])
    with pytest.raises(ValueError, match="must be"):
        lm2.load_fp8("0.wo", *lm._fp8["0.wqkv"])
    with pytest.raises(KeyError):
        lm2.load_fp8("0.nothing", *lm._fp8["0.wo"])
    assert not getattr(lm2, "_fp8", None)
    for key, (q, sc) in lm._fp8.items():
        lm2.load_fp8(key, q, sc)
    assert set(lm2._fp8) == set(lm._fp8)

    def run(e):
        try:
            e.use_fp8(True, **ALL)
            return _prefill_and_logits(e, x, mask) + _run_step(e, x5, mask5, S)
        finally:
            e.use_fp8(False)
    a, b = run(lm), run(lm2)
    assert all(lm2._fp8[k][0].data_ptr() == lm._fp8[k][0].data_ptr() for k in lm._fp8)       # quantize_fp8 kept what was loaded
    for s, t in zip(a[:4], b[:4]):
        assert torch.equal(s, t)
    assert a[4:] == b[4:]
    try:
        lm2.use_fp8(True)
        with pytest.raises(RuntimeError, match="use_fp8"):
            lm2.load_fp8("lm_head", *lm._fp8["lm_head"])
    finally:
        lm2.use_fp8(False)


def test_fp8_all_rows_head_shard_equals_whole_head(golden_dir):                              # (k)
    """emu_llama_set_head_shard on a single-rank context, as tests/test_gpu_fp4_gemm.py does for the 4-bit set: the engine is handed
    rows [r0, r1) of lm_head and of its fp8 copy; the 70-row logits of those columns (the tile form writing at a column offset that is
    not 8-byte aligned) equal the unsharded logits bit for bit, every other column is zero, and the profiler saw the shard's bytes."""
    from emu_amd._lib import check, lib
    m, *_ = _tiny_model(golden_dir)
    lm = m.decoder.lm
    g = torch.Generator().manual_seed(4)
    hid = (torch.randn(70, lm.cfg.hidden_size, generator=g) * 0.5).to(BF16).cuda()
    r0, r1 = 4101, 4101 + 8075                                                   # a ragged slice of the vocabulary at an odd column
    lm.use_fp8(True, **ALL)
    try:
        whole = lm.logits(hid).cpu()
        head = lm.lm_head[r0:r1].contiguous()
        q, sc = (t[r0:r1].contiguous() for t in lm._fp8["lm_head"])
        h = lm.handle
        check(lib().emu_llama_set_head(h, lm.final_norm.data_ptr(), head.data_ptr(), lm.embed.data_ptr(), lm.cos.data_ptr(),
                                       lm.sin.data_ptr()), "emu_llama_set_head")
        check(lib().emu_llama_set_head_fp8(h, q.data_ptr(), sc.data_ptr()), "emu_llama_set_head_fp8", lm.ctx.handle)
        check(lib().emu_llama_set_head_shard(h, r0, r1 - r0), "emu_llama_set_head_shard", lm.ctx.handle)
        out = {}
        seen = _gemv_profile(lambda: out.update(l=lm.logits(hid)))
        shard = out["l"].cpu()
    finally:
        check(lib().emu_llama_set_head_shard(lm.handle, 0, -1), "emu_llama_set_head_shard", lm.ctx.handle)
        check(lib().emu_llama_set_head(lm.handle, lm.final_norm.data_ptr(), lm.lm_head.data_ptr(), lm.embed.data_ptr(),
                                       lm.cos.data_ptr(), lm.sin.data_ptr()), "emu_llama_set_head")
        lm._fp8_register("lm_head")
        lm.use_fp8(False)
    assert seen == ((r1 - r0) * lm.cfg.hidden_size, 1)
    assert torch.equal(shard[:, r0:r1], whole[:, r0:r1])
    assert not bool(shard[:, :r0].any()) and not bool(shard[:, r1:].any())
