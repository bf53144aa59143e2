"""GPU: L2 warming (csrc/l2_warm.h) changes no bit.

The touches are loads whose results are discarded, so every kernel that carries the loop must give the same bits with a plan as
with none -- the three one-row bf16 stream forms and the combine launch on their own (through emu_l2_warm_test_plan, against a
successor tensor of exactly the planned size), and the decoder's default step under every mask.  Where a line lands cannot be seen
from here (that is what the counters in profiles/l2_warm.md are for); that the plan the kernels run stays inside the successor is
tests/test_l2_warm_plan.py's.  Modes without warming (beams, fp8 weights, tensor parallelism) must carry no plan even when the mask
is set: asserted through the engine's counter of warmed launches.
Replaces nothing of the reference: its nn.Linear / attention modules (Emu2/emu/emu.py:213-229) are the launches being joined."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
EPI_NONE, EPI_RESID, EPI_SWIGLU = 0, 1, 2
ROLLING, HEAD, PRELOAD, RT, WAVE = range(5)
MIB = 1 << 20
BLOCK_ONLY = 1 << 17                          # emu_gemm_tune: no wave / single-round-trip form (small matrices reach head / preload)


def _lib():
    from emu_amd._lib import lib
    return lib()


def _geometry(N, K, norm, epi):
    out = (C.c_int * 4)()
    assert _lib().emu_gemv_geometry_query(N, K, int(norm), epi, out) == 0
    return out[0], out[1]


def _plan_over(succ, rows, pred_wgs, extra, lanes):
    """A plan that covers the whole [Ns, Ks] successor tensor, read `rows` rows per workgroup."""
    from emu_amd._lib import WarmPlanC
    Ns, Ks = succ.shape
    p = WarmPlanC()
    assert _lib().emu_l2_warm_plan_make(succ.data_ptr(), 0, rows, Ks * 2, Ks * 2, Ns, 0, 1, pred_wgs, int(extra), lanes, 64 * MIB, 0,
                                        C.byref(p)) == 0
    assert p.ntouch > 0 and p.nsucc * rows >= Ns - Ns % (8 * rows), (p.ntouch, p.nsucc)
    return p


class _Plan:
    def __init__(self, p):
        self.p = p

    def __enter__(self):
        _lib().emu_l2_warm_test_plan(C.byref(self.p) if self.p is not None else None)

    def __exit__(self, *a):
        _lib().emu_l2_warm_test_plan(None)


class _Tune:
    def __init__(self, mask):
        self.mask = mask

    def __enter__(self):
        _lib().emu_gemm_tune(self.mask)

    def __exit__(self, *a):
        _lib().emu_gemm_tune(0)


@pytest.mark.parametrize("form,N,K,norm,epi,tune", [
    (HEAD, 40, 6656, True, EPI_NONE, BLOCK_ONLY),        # K / 8 = 832 is no multiple of 256: the clamped chunks of the last trip
    (HEAD, 40, 6656, True, EPI_SWIGLU, BLOCK_ONLY),
    (PRELOAD, 38, 520, False, EPI_RESID, BLOCK_ONLY),
    (PRELOAD, 38, 520, False, EPI_NONE, BLOCK_ONLY),
    (RT, 38, 17920, False, EPI_RESID, 0),
    (RT, 38, 17920, False, EPI_NONE, 0),
])
def test_stream_forms_bit_identical_with_and_without_a_plan(form, N, K, norm, epi, tune):
    from emu_amd import ops
    g = torch.Generator().manual_seed(N * 31 + K)
    x = torch.randn(1, K, generator=g).to(BF16).cuda()
    w = (torch.randn(N, K, generator=g) * 0.05).to(BF16).cuda()
    gain = (1 + 0.1 * torch.randn(K, generator=g)).to(BF16).cuda() if norm else None
    res = torch.randn(1, N, generator=g).to(BF16).cuda() if epi == EPI_RESID else None
    succ = torch.randn(96, 1032, generator=g).to(BF16).cuda()             # 96 rows of 2064 bytes: lines straddle rows
    with _Tune(tune):
        got_form, rows = _geometry(N, K, norm, epi)
        assert got_form == form
        plan = _plan_over(succ, 2, -(-N // rows), False, 256)
        run = lambda: ops.linear(x, w, res=res, norm_w=gain, eps=1e-6, epi=epi).clone()
        base = run()
        with _Plan(plan):
            warmed = run()
        again = run()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(base.float()).all())
    assert torch.equal(base.view(torch.int16), warmed.view(torch.int16))
    assert torch.equal(base.view(torch.int16), again.view(torch.int16))
    # the form under test computes what the plain product does (loose: bf16 rounding; the exact checks are the stream tests')
    xe = x.float()
    if norm:
        xe = (gain.float() * (xe * torch.rsqrt(xe.pow(2).mean(-1, keepdim=True) + 1e-6)).to(BF16).float()).to(BF16).float()
    y = xe @ w.float().t()
    if epi == EPI_SWIGLU:
        y = torch.nn.functional.silu(y[:, 0::2]) * y[:, 1::2]
    if res is not None:
        y = y.to(BF16).float() + res.float()
    assert torch.allclose(base.float(), y, rtol=3e-2, atol=3e-2 * float(y.abs().max()))


def test_combine_launch_bit_identical_with_warming_workgroups():
    """H = 4 heads, context 300 in a launch sized for eight 128-key splits: three live, five dead (their workspace words poisoned)."""
    from emu_amd import ops
    H, D, S_max, ctx_max, slot = 4, 128, 1024, 1024, 299
    g = torch.Generator().manual_seed(77)
    qkv = torch.randn(1, 3 * H * D, generator=g).to(BF16).cuda()
    kc = torch.randn(1, H, S_max, D, generator=g).to(BF16).cuda()
    vc = torch.randn(1, H, S_max, D, generator=g).to(BF16).cuda()
    ang = torch.rand(2048, D, generator=g) * 6.28
    cos, sin = torch.cos(ang).to(BF16).cuda(), torch.sin(ang).to(BF16).cuda()
    pos = torch.tensor([slot], dtype=torch.int32).cuda()
    sl = torch.tensor([slot], dtype=torch.int32).cuda()
    succ = torch.randn(96, 1032, generator=g).to(BF16).cuda()
    plan = _plan_over(succ, 2, H, True, D)
    assert plan.first == H and plan.lanes == D
    outs = []
    for p in (None, plan, None):
        k, v = kc.clone(), vc.clone()
        ws = torch.full((_lib().emu_decode_fused_ws_bytes(1, H, D, ctx_max) // 4,), float("nan"), device="cuda")
        with _Plan(p):
            o = ops.decode_fused(qkv, cos, sin, pos, sl, k, v, H, ctx_max, D ** -0.5, ws=ws)
        outs.append((o.clone(), k, v))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0][0].float()).all())
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    for a, b in zip(outs[0], outs[2]):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---- the decoder: two layers at H = 512, 4 heads x 128, F = 1024
def _engine(tp=1):
    from emu_amd import synth
    from emu_amd.conf.emu_conf import LlamaCfg
    from emu_amd.llama import EmuHipContext, LlamaEngine
    cfg = LlamaCfg(hidden_size=512, intermediate_size=1024, num_attention_heads=4, num_hidden_layers=2)
    dev = torch.device("cuda", 0)
    real = EmuHipContext(dev, 0, 1)
    ctx = real
    if tp > 1:
        # a one-rank peer-to-peer comm block: the engine runs its all-reduces, the peers are this rank
        real.init_tp(lambda b: b, force=True, allgather_bytes=lambda b: [b], rccl=False)

        class ShardView:                                  # rank 0's 1/tp shard
            def __init__(self, c, size):
                self.__dict__.update(ctx=c, tp_rank=0, tp_size=size)

            def __getattr__(self, k):
                return getattr(self.ctx, k)
        ctx = ShardView(real, tp)
    eng = LlamaEngine(cfg, 256, ctx)
    eng.load_weights(synth.iter_synth(synth.llama_param_shapes(cfg, 256), seed=3, device=dev, dtype=BF16))
    return eng


def _greedy(eng, S, steps, graph):
    """prefill S random rows, then `steps` greedy steps: ids, hidden states and logits of every step, K / V caches."""
    from emu_amd import ops
    from emu_amd.llama import GreedyState
    dev = eng.device
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(1, S, eng.cfg.hidden_size, generator=g) * 0.1).to(BF16).to(dev)
    hidden, kstart, next_pos = eng.prefill(x, torch.ones(1, S, dtype=torch.long), eng.kv_capacity(S + steps + 8))
    cur = ops.argmax(eng.logits(hidden[:, -1, :].contiguous()), suppress_id=2)
    out = torch.zeros(steps + 2, 1, device=dev, dtype=torch.int32)
    st = GreedyState(eng, 1, cur, next_pos, S, kstart, out)
    hs, lg = [], []
    for _ in range(steps):
        (st.step_graph if graph else st.step)()
        hs.append(st.hidden.clone())
        lg.append(st.logits.clone())
    torch.cuda.synchronize()
    return out.clone(), torch.stack(hs), torch.stack(lg), eng.kcache.clone(), eng.vcache.clone()


@pytest.fixture(scope="module")
def decoder():
    eng = _engine()
    ref = {}
    eng.set_l2_warm(0)
    for graph in (False, True):
        n0 = eng.l2_warm_count()
        ref[graph] = _greedy(eng, 120, 12, graph)          # slots 120..131: across the 128-key split boundary
        assert eng.l2_warm_count() == n0                   # mask 0: no launch carries a plan
    for a, b in zip(ref[False], ref[True]):
        assert torch.equal(a, b)
    return eng, ref


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("mask", [31, 1, 2, 4, 8, 16, 31 | 32, 31 | (8 << 8)])
def test_decoder_bit_identical_under_every_mask(decoder, mask, graph):
    eng, ref = decoder
    eng.set_l2_warm(mask)
    try:
        n0 = eng.l2_warm_count()
        got = _greedy(eng, 120, 12, graph)
        assert eng.l2_warm_count() > n0                     # the path under test is the one that ran
    finally:
        eng.set_l2_warm(0)
    assert bool(torch.isfinite(got[1].float()).all())
    for a, b in zip(got, ref[graph]):
        assert torch.equal(a, b)


def test_tune_bit_30_switches_all_warming_off(decoder):
    eng, ref = decoder
    eng.set_l2_warm(31)
    try:
        with _Tune(1 << 30):
            n0 = eng.l2_warm_count()
            got = _greedy(eng, 120, 12, False)
            assert eng.l2_warm_count() == n0
    finally:
        eng.set_l2_warm(0)
    for a, b in zip(got, ref[False]):
        assert torch.equal(a, b)


def _one_step(eng, B, S):
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(B, S + 1, eng.cfg.hidden_size, generator=g) * 0.1).to(BF16).cuda()
    _, kstart, pos = eng.prefill(x[:, :S].contiguous(), torch.ones(B, S, dtype=torch.long), eng.kv_capacity(S + 16))
    h = eng.decode_embeds(x[:, S].contiguous(), pos, S, kstart).clone()
    torch.cuda.synchronize()
    return h


@pytest.mark.parametrize("mode", ["beams", "fp8", "tp"])
def test_modes_without_warming_carry_no_plan(mode):
    eng = _engine(tp=2 if mode == "tp" else 1)
    if mode == "fp8":
        eng.use_fp8(True)
    B = 5 if mode == "beams" else 1
    outs = []
    for mask in (0, 31):
        eng.set_l2_warm(mask)
        n0 = eng.l2_warm_count()
        outs.append(_one_step(eng, B, 40))
        assert eng.l2_warm_count() == n0, mode              # the plans are null there
    eng.set_l2_warm(0)
    assert bool(torch.isfinite(outs[0].float()).all())
    assert torch.equal(outs[0], outs[1])
