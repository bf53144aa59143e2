"""GPU: the 13-bit lossless bf16 decode stream.  The device packer against emu_amd/bf16pack.py byte for byte; the packed kernels
(emu_linear_bf16pack) against emu_linear_bf16 on the raw bf16 bits, one case per form; a small engine and one true-shape layer with the
stream on and off.  Every comparison is bit-exact."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
EPI_NONE, EPI_RESID, EPI_SWIGLU = 0, 1, 2
HEAD, PRELOAD, RT = 1, 2, 3
BLOCK_ONLY = 1 << 17          # emu_gemm_tune: small matrices reach the block kernel's forms (no wave / single-round-trip form)


def bits(t):
    return t.contiguous().view(torch.int16)


def _lib():
    from emu_amd._lib import lib
    return lib()


class _Tune:
    def __init__(self, mask):
        self.mask = mask

    def __enter__(self):
        _lib().emu_gemm_tune(self.mask)

    def __exit__(self, *a):
        _lib().emu_gemm_tune(0)


def _matrix(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, K, generator=g) * 0.02).to(BF16)
    W[W == 0] = 0.01
    return W


def _planted():
    from tests.test_bf16_pack_format import planted_matrix
    return planted_matrix()[0]


# ------------------------------------------------------------------------------------------------ 1. the packer
PACK_SIZES = [(8, 32), (6, 64), (10, 2048), (8, 6656), (4, 17920)]


@pytest.mark.parametrize("rows", [2, 4])
@pytest.mark.parametrize("shape", PACK_SIZES + ["planted"])
def test_device_packer_matches_python(shape, rows):
    from emu_amd import bf16pack, ops
    W = _planted() if shape == "planted" else _matrix(*shape, seed=shape[0] + shape[1])
    want = bf16pack.pack(W, rows)
    got = ops.pack_bf16_rows(W.cuda(), rows)
    assert got["hb"] == want["hb"] and got["rows"] == rows and tuple(got["shape"]) == tuple(W.shape)
    for k in ("lo", "nib", "sign", "flags"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert torch.equal(got[k].cpu(), want[k]), k
    if shape == "planted":
        assert bf16pack.flagged_groups(want).any() and not bf16pack.flagged_groups(want).all()


# ------------------------------------------------------------------------------------------------ 2. the stream kernels
def _case(W, form, rows, epi, norm, seed, finite=True):
    """emu_linear_bf16pack over the packed set of W == emu_linear_bf16 on W, on the raw bits."""
    from emu_amd import ops
    N, K = W.shape
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(1, K, generator=g) * 0.5).to(BF16).cuda()
    gain = (1 + 0.1 * torch.randn(K, generator=g)).to(BF16).cuda() if norm else None
    res = torch.randn(1, N, generator=g).to(BF16).cuda() if epi == EPI_RESID else None
    Wd = W.cuda()
    want = ops.linear(x, Wd, res=res, norm_w=gain, eps=1e-5, epi=epi)
    p = ops.pack_bf16_rows(Wd, rows)
    n_out = N // 2 if epi == EPI_SWIGLU else N
    out = torch.full((1, n_out + 8), float("nan"), dtype=BF16, device="cuda")        # a guard band behind the row
    ops.linear_bf16pack(x, Wd, p, form, res=res, norm_w=gain, eps=1e-5, epi=epi, out=out)
    torch.cuda.synchronize()
    assert not finite or bool(torch.isfinite(want.float()).all())
    assert torch.equal(bits(out[:, :n_out]), bits(want))
    assert bool(torch.isnan(out[:, n_out:].float()).all())                           # nothing written past the row


@pytest.mark.parametrize("K", [32, 64, 2048, 2080, 6656])
@pytest.mark.parametrize("N", [4, 6, 8])
@pytest.mark.parametrize("epi", [EPI_NONE, EPI_SWIGLU])
def test_head_form(N, K, epi):
    _case(_matrix(N, K, seed=N * 7 + K), HEAD, 4, epi, True, seed=K + N + epi)


@pytest.mark.parametrize("K", [32, 64, 2048, 2080, 6656])
@pytest.mark.parametrize("N", [2, 3])
def test_preload_form(N, K):
    _case(_matrix(N, K, seed=N * 5 + K), PRELOAD, 2, EPI_RESID, False, seed=K + N)


@pytest.mark.parametrize("K", [32, 64, 2048, 2080, 6656, 17920])
@pytest.mark.parametrize("N", [2, 3])
def test_single_round_trip_form(N, K):
    _case(_matrix(N, K, seed=N * 3 + K), RT, 2, EPI_RESID, False, seed=K + N + 1)


@pytest.mark.parametrize("form,rows,epi,norm", [(HEAD, 4, EPI_NONE, True), (HEAD, 4, EPI_SWIGLU, True), (PRELOAD, 2, EPI_RESID, False),
                                                (RT, 2, EPI_RESID, False)])
def test_planted_matrix_flagged_and_unflagged_workgroups(form, rows, epi, norm):
    """Flagged and unflagged workgroups in one launch.  The rows that hold the planted Inf / NaN give Inf / NaN in both kernels: the
    comparison is on the bits all the same."""
    from emu_amd import bf16pack
    W = _planted()
    fl = bf16pack.flagged_groups(bf16pack.pack(W, rows))
    assert fl.any() and not fl.all()
    _case(W, form, rows, epi, norm, seed=form * 10 + epi, finite=False)


# ------------------------------------------------------------------------------------------------ 3. a small engine
def _engine():
    from emu_amd import synth
    from emu_amd.conf.emu_conf import LlamaCfg
    from emu_amd.llama import EmuHipContext, LlamaEngine
    cfg = LlamaCfg(hidden_size=256, intermediate_size=512, num_attention_heads=2, num_hidden_layers=2)
    dev = torch.device("cuda", 0)
    eng = LlamaEngine(cfg, 512, EmuHipContext(dev, 0, 1))
    eng.load_weights(synth.iter_synth(synth.llama_param_shapes(cfg, 512), seed=3, device=dev, dtype=BF16))
    return eng


def _greedy(eng, S, steps, graph):
    from emu_amd import ops
    from emu_amd.llama import GreedyState
    dev = eng.device
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(1, S, eng.cfg.hidden_size, generator=g) * 0.1).to(BF16).to(dev)
    hidden, kstart, next_pos = eng.prefill(x, torch.ones(1, S, dtype=torch.long), eng.kv_capacity(S + steps + 8))
    cur = ops.argmax(eng.logits(hidden[:, -1, :].contiguous()), suppress_id=2)
    out = torch.zeros(steps + 2, 1, device=dev, dtype=torch.int32)
    st = GreedyState(eng, 1, cur, next_pos, S, kstart, out)
    lg = []
    for _ in range(steps):
        (st.step_graph if graph else st.step)()
        lg.append(st.logits.clone())
    torch.cuda.synchronize()
    return out.clone(), torch.stack(lg)


def _gemv_bytes(eng, steps):
    """Weight bytes the GEMV profiler prices over `steps` eager greedy steps."""
    from emu_amd._lib import check
    L = _lib()
    check(L.emu_profile_gemv(1), "emu_profile_gemv")
    try:
        _greedy(eng, 40, steps, False)
        ms, wb, nl = C.c_double(), C.c_double(), C.c_long()
        check(L.emu_profile_gemv_read(C.byref(ms), C.byref(wb), C.byref(nl)), "emu_profile_gemv_read")
    finally:
        L.emu_profile_gemv(0)
    return wb.value, nl.value


def test_small_engine_stream_on_and_off():
    """Hidden 256, 2 heads x 128, ffn 512, vocab 512: under the default plan every matrix of such an engine is a small
    single-round-trip shape without a packed twin, so the engine packs nothing by itself; with the block-kernel-only tune bit the
    o_proj and down matrices take the preload form, whose twin then runs in both layers."""
    eng = _engine()
    assert not getattr(eng, "bf16_pack_on", False) and not getattr(eng, "_pack", {})
    with _Tune(BLOCK_ONLY):
        ref = {graph: _greedy(eng, 40, 8, graph) for graph in (False, True)}
        bytes_off, launches = _gemv_bytes(eng, 2)
        n, nbytes = eng.pack_bf16(tune=BLOCK_ONLY)
        assert n == 4 and sorted(eng._pack) == ["0.wdown", "0.wo", "1.wdown", "1.wo"]
        full = eng.weight_bytes_per_token()
        eng.use_bf16_pack(True)
        saved = 2 * (256 * 256 + 256 * 512) * 3 // 8 - 4 * 16          # 3 of 16 bits per weight, less 4 flag words (128 row groups) per matrix
        assert eng.weight_bytes_per_token() == full - saved
        epoch = eng.mode_epoch
        got = {graph: _greedy(eng, 40, 8, graph) for graph in (False, True)}
        bytes_on, launches_on = _gemv_bytes(eng, 2)
        assert launches_on == launches and bytes_off - bytes_on == pytest.approx(2 * saved)     # the packed twins are what ran
        eng.use_bf16_pack(False)
        assert eng.mode_epoch == epoch + 1 and not eng.__dict__.get("_loop_states")    # the captured graph went with the mode
        assert eng.weight_bytes_per_token() == full
        again = _greedy(eng, 40, 8, True)
    for graph in (False, True):
        assert torch.equal(got[graph][0], ref[graph][0]) and torch.equal(bits(got[graph][1]), bits(ref[graph][1]))
    assert torch.equal(ref[False][0], ref[True][0]) and torch.equal(bits(ref[False][1]), bits(ref[True][1]))
    assert torch.equal(again[0], ref[True][0]) and torch.equal(bits(again[1]), bits(ref[True][1]))


def test_other_modes_keep_the_bf16_kernels():
    """fp8, fp4, decode-fused, decode-tail and l2-warm: the rule answers the kernel it was given (no GPU work)."""
    L = _lib()
    N, K = 19968, 6656
    assert L.emu_llama_pack_kernel(0, 1, 4, 1, 0, 0, 0, N, K, 1, EPI_NONE, 0) == 6
    for f8, f4 in ((1, 0), (2, 0), (0, 1), (0, 2), (0, 3)):
        k = L.emu_llama_weight_kernel(f8, f4, 1, 6656, 6656, 17920)
        assert k != 0 and L.emu_llama_pack_kernel(k, 1, 4, 1, 0, 0, 0, N, K, 1, EPI_NONE, 0) == k
    for fused, tail, warm in ((1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0), (0, 1, 0), (0, 0, 31), (0, 0, 1)):
        assert L.emu_llama_pack_kernel(0, 1, 4, 1, fused, tail, warm, N, K, 1, EPI_NONE, 0) == 0


# ------------------------------------------------------------------------------------------------ 4. one true-shape layer
def test_true_shape_layer_identical_on_and_off():
    """One layer at 6656 / 52 heads / 17920, one cached decode row at 64 context slots: qkv, o_proj, gate/up and down all have a
    packed twin at these shapes (0.9 GB of sets).  The default packs the two plain streams (o_proj, down), whose twins are the faster
    ones; the head-form sets (qkv, gate/up) are added here, so all four packed kernels run in the layer."""
    from emu_amd import synth
    from emu_amd.conf.emu_conf import LlamaCfg
    from emu_amd.llama import EmuHipContext, LlamaEngine
    cfg = LlamaCfg(hidden_size=6656, intermediate_size=17920, num_attention_heads=52, num_hidden_layers=1)
    dev = torch.device("cuda", 0)
    eng = LlamaEngine(cfg, 64, EmuHipContext(dev, 0, 1))
    eng.load_weights(synth.iter_synth(synth.llama_param_shapes(cfg, 64), seed=1, device=dev, dtype=BF16))
    assert eng.bf16_pack_on and sorted(eng._pack) == ["0.wdown", "0.wo"]                          # the default
    assert eng.pack_bf16(head_form=True)[0] == 2 and sorted(eng._pack) == ["0.wdown", "0.wgu", "0.wo", "0.wqkv"]
    assert [eng._pack[k]["rows"] for k in ("0.wqkv", "0.wo", "0.wgu", "0.wdown")] == [4, 2, 4, 2]
    g = torch.Generator().manual_seed(2)
    eng.alloc_kv(1, 64)
    kv0 = (torch.randn(2, 1, 1, 52, 64, 128, generator=g) * 0.5).to(BF16).to(dev)
    x = (torch.randn(1, 6656, generator=g) * 0.5).to(BF16).to(dev)
    pos = torch.tensor([63], device=dev, dtype=torch.int32)
    kstart = torch.zeros(1, device=dev, dtype=torch.int32)
    outs = {}
    for on in (True, False, True):
        eng.use_bf16_pack(on)
        eng.kcache.copy_(kv0[0]); eng.vcache.copy_(kv0[1])
        h = eng.decode_embeds(x, pos, 63, kstart)
        torch.cuda.synchronize()
        got = (h.clone(), eng.kcache[0, 0, :, 63].clone(), eng.vcache[0, 0, :, 63].clone())
        if on in outs:
            for a, b in zip(got, outs[on]):
                assert torch.equal(bits(a), bits(b))
        outs[on] = got
    assert bool(torch.isfinite(outs[True][0].float()).all())
    assert not torch.equal(bits(outs[True][1]), bits(kv0[0][0, 0, :, 63]))          # the step appended its K row
    for a, b in zip(outs[True], outs[False]):
        assert torch.equal(bits(a), bits(b))
