"""GPU: the few-row (4..16) stream over the 13-bit packed bf16 sets (csrc/gemv_pack_thin.hip, emu_linear_bf16pack_thin,
LlamaEngine.use_bf16_pack_wide).  Every comparison is on the raw bits: the primitive against emu_linear_bf16 on the bf16 matrix (the
bf16 few-row stream), the decode against the matrix itself through one-hot activations, flagged and unflagged workgroups with a
witness of which branch ran, a small engine and one true-shape layer with the switch off / on."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
EPI_NONE, EPI_RESID, EPI_SWIGLU = 0, 1, 2
BLOCK_ONLY = 1 << 17          # emu_gemm_tune: small matrices reach the block kernel's one-row forms (tests/test_gpu_bf16_pack.py)
PIN16, PIN32 = 1 << 28, 2 << 28       # emu_gemm_tune bits 28-29: 16 / 32 weight rows per workgroup, so small shapes run both tiles
ROWS = (4, 5, 8, 9, 16)


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


def _plan(M, N, K, epi, R, tune):
    """(weight rows per workgroup, ring depth) of the launch, from the planner hook."""
    from tests.test_gemv_plan import PlanC, ShapeC, shape
    out = PlanC()
    assert _lib().emu_gemv_pack_thin_plan(C.byref(ShapeC(*shape(M, N, K, epi))), R, tune, C.byref(out)) == 0
    return out.rows, out.stages


def _guarded(M, n_out):
    """([M, n_out] output view, the NaN guard band behind its last row)"""
    buf = torch.full((M * n_out + 64,), float("nan"), dtype=BF16, device="cuda")
    return buf[:M * n_out].view(M, n_out), buf[M * n_out:]


# ------------------------------------------------------------------------------------------------ 1. bit identity with the bf16 stream
# (37, 256): one stage, ragged N, the last workgroup's groups clamped (odd N: no SwiGLU, the planner refuses it); (50, 1024): R = 2;
# (264, 768); (64, 2560): ten stages, more than the ring is deep; (2240, 6656): a true width
SHAPES = [(37, 256, (2, 4)), (50, 1024, (2,)), (264, 768, (2, 4)), (64, 2560, (2, 4)), (2240, 6656, (2, 4))]
CASES = [(N, K, R, tune) for N, K, Rs in SHAPES for R in Rs for tune in (PIN16, PIN32)]


@pytest.mark.parametrize("N,K,R,tune", CASES)
def test_bits_of_the_bf16_stream(N, K, R, tune):
    from emu_amd import ops
    W = _matrix(N, K, seed=N + K).cuda()
    p = ops.pack_bf16_rows(W, R)
    g = torch.Generator().manual_seed(N * 3 + K + R)
    for M in ROWS:
        x = (torch.randn(M, K, generator=g) * 0.5).to(BF16).cuda()
        res = torch.randn(M, N, generator=g).to(BF16).cuda()
        for epi in (EPI_NONE, EPI_RESID) + ((EPI_SWIGLU,) if N % 2 == 0 else ()):
            r = res if epi == EPI_RESID else None
            want = ops.linear(x, W, res=r, epi=epi)                         # emu_gemm_tune 0: the bf16 few-row stream
            assert _plan(M, N, K, epi, R, tune) == ((32, 4 if M <= 8 else 3) if tune == PIN32 else (16, 6 if M <= 8 else 5))
            out, guard = _guarded(M, N // 2 if epi == EPI_SWIGLU else N)
            with _Tune(tune):
                ops.linear_bf16pack_thin(x, W, p, res=r, epi=epi, out=out)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(want.float()).all())
            assert torch.equal(bits(out), bits(want)), (M, epi)
            assert bool(torch.isnan(guard.float()).all()), (M, epi)          # nothing written past the rows


# ------------------------------------------------------------------------------------------------ 2. decode exactness
def _all_codes_matrix():
    """[8192, 256]: column k holds every 13-bit code (sign, nibble, low byte) once, so every code meets every position of a stage;
    hb = 48 puts the exponent fields at 96 .. 127: all finite, none zero."""
    n = torch.arange(8192, dtype=torch.int32)[:, None]
    k = torch.arange(256, dtype=torch.int32)[None, :]
    code = (n + 37 * k) % 8192
    b = ((code >> 12) << 15) | ((((code >> 8) & 15) + 48) << 8) | (code & 255)
    return torch.where(b >= 2 ** 15, b - 2 ** 16, b).to(torch.int16).view(BF16)


@pytest.fixture(scope="module")
def all_codes():
    from emu_amd import bf16pack
    W = _all_codes_matrix()
    codes = (W.view(torch.int16).to(torch.int32) & 0xFFFF)
    codes = ((codes >> 15) << 12) | ((((codes >> 8) & 0x7F) - 48) << 8) | (codes & 255)
    assert all(sorted(codes[:, k].tolist()) == list(range(8192)) for k in (0, 1, 127, 255))
    assert bf16pack.matrix_hb(W) == 48 and not bool(bf16pack.flag_rule(W, 48).any())
    assert bool(torch.isfinite(W.float()).all())
    return W.cuda()


@pytest.mark.parametrize("tune", [PIN16, PIN32])
@pytest.mark.parametrize("R", [2, 4])
def test_every_code_decodes_exactly(all_codes, R, tune):
    """One-hot activation rows: out[m, n] must be W[n, k_m], independent of the bf16 kernel.  Sixteen k per launch, sixteen launches."""
    from emu_amd import ops
    W = all_codes
    p = ops.pack_bf16_rows(W, R)
    assert p["hb"] == 48 and not bool(p["flags"].any())
    poison = torch.full_like(W, float("nan"))                               # the bf16 matrix is not what is read
    with _Tune(tune):
        for k0 in range(0, 256, 16):
            x = torch.zeros(16, 256, dtype=BF16, device="cuda")
            x[torch.arange(16), torch.arange(k0, k0 + 16)] = 1.0
            out = ops.linear_bf16pack_thin(x, poison, p)
            assert torch.equal(bits(out), bits(W[:, k0:k0 + 16].t())), k0


# ------------------------------------------------------------------------------------------------ 3. flags
def _planted(N, K):
    """Zeros (outside the 32-binade window of weights around 0.02) in the first and in the last 16 rows, none between."""
    W = _matrix(N, K, seed=11)
    W[3, K - 212] = 0.0
    W[N - 1, 7] = 0.0
    return W


# (N, K, M, tune) -> the tile: every built (weight rows, activation bucket, ring depth), hence both depths of the flagged branch's own
# ring (three stages where they fit the packed ring, else two); 16500 rows: 516 / 1032 workgroups, which fill three per CU best
FLAG_CASES = {(200, 512, 5, PIN16): (16, 6), (200, 512, 5, PIN32): (32, 4), (200, 512, 9, PIN16): (16, 5), (200, 512, 9, PIN32): (32, 3),
              (16500, 256, 5, PIN32): (32, 3), (16500, 256, 5, PIN16): (16, 4), (16500, 256, 9, PIN16): (16, 3)}


@pytest.mark.parametrize("case", sorted(FLAG_CASES))
@pytest.mark.parametrize("R", [2, 4])
def test_flagged_workgroups_stream_bf16_and_the_others_the_planes(R, case):
    from emu_amd import bf16pack, ops
    N, K, M, tune = case
    W = _planted(N, K)
    fl = bf16pack.flagged_groups(bf16pack.pack(W, R))
    assert fl.any() and not fl.all() and int(fl.sum()) == 2
    rn, stages = _plan(M, N, K, EPI_NONE, R, tune)                           # the workgroup extent
    assert (rn, stages) == FLAG_CASES[case]
    nwg = (N + rn - 1) // rn
    wg_flagged = torch.zeros(nwg, dtype=torch.bool)
    wg_flagged[(torch.nonzero(fl).flatten() * R) // rn] = True
    assert wg_flagged.tolist() == [True] + [False] * (nwg - 2) + [True]      # one in the first workgroup, one in the last
    Wd = W.cuda()
    p = ops.pack_bf16_rows(Wd, R)
    assert torch.equal(bf16pack.flagged_groups({**p, "flags": p["flags"].cpu()}), fl)
    g = torch.Generator().manual_seed(R)
    x = (torch.randn(M, K, generator=g) * 0.5).to(BF16).cuda()
    want = ops.linear(x, Wd)
    row_flagged = wg_flagged.repeat_interleave(rn)[:N].cuda()
    # witness: the unflagged workgroups never read the bf16 rows, the flagged ones never use the planes
    W_nan = Wd.clone()
    W_nan[~row_flagged] = float("nan")
    q = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in p.items()}
    grp_flagged = wg_flagged.repeat_interleave(rn // R)[:q["lo"].shape[0]].cuda()
    for name in ("lo", "nib", "sign"):
        noise = torch.randint(0, 256, q[name].shape, dtype=torch.uint8, generator=g).cuda()
        q[name][grp_flagged] = noise[grp_flagged]
    with _Tune(tune):
        for w_arg, set_arg in ((Wd, p), (W_nan, p), (Wd, q), (W_nan, q)):
            out, guard = _guarded(M, N)
            ops.linear_bf16pack_thin(x, w_arg, set_arg, out=out)
            torch.cuda.synchronize()
            assert torch.equal(bits(out), bits(want))
            assert bool(torch.isnan(guard.float()).all())


# ------------------------------------------------------------------------------------------------ 4. a small engine
def _engine():
    from emu_amd import synth
    from emu_amd.conf.emu_conf import LlamaCfg
    from emu_amd.llama import EmuHipContext, LlamaEngine
    cfg = LlamaCfg(hidden_size=256, intermediate_size=512, num_attention_heads=2, num_hidden_layers=2)
    dev = torch.device("cuda", 0)
    eng = LlamaEngine(cfg, 512, EmuHipContext(dev, 0, 1))
    eng.load_weights(synth.iter_synth(synth.llama_param_shapes(cfg, 512), seed=3, device=dev, dtype=BF16))
    return eng


def _prompt(eng, S=24):
    ids = (torch.arange(S) % 6 + 7).view(1, S)                               # a repeating prompt: the lookup finds drafts
    x = eng.embed[ids.to(eng.device)].view(1, S, -1).contiguous()
    return x, torch.ones(1, S, dtype=torch.long), ids


def _beam(eng, graph):
    x, mask, _ = _prompt(eng)
    eng.beam_graph = graph
    ids = eng.beam_search_generate(x, mask, 5, 8, hf_semantics="5.x").cpu()
    lg = eng._loop_states["beam"][1]["lg"].clone()                           # the last step's logits of the 5 beams
    torch.cuda.synchronize()
    return ids, lg


def _lookup(eng, graph):
    x, mask, ids = _prompt(eng)
    trace = None if graph else []
    out = eng.lookup_generate(x, mask, ids, 10, 4, use_graph=graph, stop_on_eos=False, trace=trace).cpu()
    lg = eng._loop_states["lookup"][1]["lg"].clone()                         # the last chunk step's logits of its 5 rows
    torch.cuda.synchronize()
    return out, lg if graph else torch.stack([t["logits"] for t in trace])


def _five_row_steps(eng, steps):
    """(bytes, launches) the GEMV profiler prices over `steps` eager cached steps of 5 rows, and the last step's hidden rows."""
    from emu_amd._lib import check
    L = _lib()
    g = torch.Generator().manual_seed(5)
    S = 24
    x = (torch.randn(5, S + steps, eng.cfg.hidden_size, generator=g) * 0.1).to(BF16).to(eng.device)
    _, kstart, pos = eng.prefill(x[:, :S].contiguous(), torch.ones(5, S, dtype=torch.long), eng.kv_capacity(S + steps + 8))
    check(L.emu_profile_gemv(1), "emu_profile_gemv")
    try:
        for j in range(steps):
            h = eng.decode_embeds(x[:, S + j].contiguous(), pos + j, S + j, kstart)
            lg = eng.logits(h)
        ms, wb, nl = C.c_double(), C.c_double(), C.c_long()
        check(L.emu_profile_gemv_read(C.byref(ms), C.byref(wb), C.byref(nl)), "emu_profile_gemv_read")
    finally:
        L.emu_profile_gemv(0)
    torch.cuda.synchronize()
    return wb.value, nl.value, (h.clone(), lg.clone())


def test_small_engine_switch_off_on_off():
    """tests/test_gpu_bf16_pack.py's engine and sets (o_proj and down of both layers, R = 2, made under the block-kernel-only tune
    bit).  A 5-beam search and a prompt-lookup generation with k = 4 (5-row chunk steps), eager and replayed from a graph: the ids
    and the logits are the same bits with the switch off, on and off again; on, the 5-row steps stream the planes of the four packed
    matrices -- 3 of 16 bits per weight less, flag words more -- in as many launches; the switch drops the captured graph."""
    from emu_amd._lib import EmuHipError
    eng = _engine()
    with _Tune(BLOCK_ONLY):
        assert eng.pack_bf16(tune=BLOCK_ONLY)[0] == 4 and sorted(eng._pack) == ["0.wdown", "0.wo", "1.wdown", "1.wo"]
        with pytest.raises(RuntimeError, match="use_bf16_pack"):
            eng.use_bf16_pack_wide(True)                                     # needs the packed stream on
        eng.use_bf16_pack(True)
        assert not getattr(eng, "bf16_pack_wide", False)                     # off by default
        runs = {}
        for state in ("off", "on", "off again"):
            epoch = eng.mode_epoch
            eng.use_bf16_pack_wide(state == "on")
            assert eng.bf16_pack_wide == (state == "on")
            assert eng.mode_epoch == epoch + 1 and not eng.__dict__.get("_loop_states")       # the captured graphs went with the mode
            runs[state] = dict(beam={gr: _beam(eng, gr) for gr in (False, True)}, lookup={gr: _lookup(eng, gr) for gr in (False, True)},
                               prof=_five_row_steps(eng, 2))
        eng.beam_graph = True
    off = runs["off"]
    for state in ("on", "off again"):
        for loop in ("beam", "lookup"):
            for gr in (False, True):
                assert torch.equal(runs[state][loop][gr][0], off[loop][gr][0]), (state, loop, gr)
                assert torch.equal(bits(runs[state][loop][gr][1]), bits(off[loop][gr][1])), (state, loop, gr)
        for a, b in zip(runs[state]["prof"][2], off["prof"][2]):
            assert torch.equal(bits(a), bits(b))
    for loop in ("beam", "lookup"):
        assert torch.equal(off[loop][False][0], off[loop][True][0])          # eager and graph agree with each other
    # per step: 3 of 16 bits per weight of o_proj and down in both layers, less 4 flag words (128 row groups) per matrix
    saved = 2 * (256 * 256 + 256 * 512) * 3 // 8 - 4 * 16
    (b_off, n_off, _), (b_on, n_on, _), (b_again, n_again, _) = (runs[s]["prof"] for s in ("off", "on", "off again"))
    assert n_on == n_off == n_again and b_again == b_off
    assert b_off - b_on == pytest.approx(2 * saved)


# ------------------------------------------------------------------------------------------------ 5. one true-shape layer
def test_true_shape_layer_five_rows_on_and_off():
    """One layer at 6656 / 52 heads / 17920 with all four sets (R = 4, 2, 4, 2), a chunk of five rows on 59 cached slots: hidden state
    and the appended K / V rows are the same bits with the switch on and off."""
    from emu_amd import synth
    from emu_amd.conf.emu_conf import LlamaCfg
    from emu_amd.llama import EmuHipContext, LlamaEngine
    cfg = LlamaCfg(hidden_size=6656, intermediate_size=17920, num_attention_heads=52, num_hidden_layers=1)
    dev = torch.device("cuda", 0)
    eng = LlamaEngine(cfg, 64, EmuHipContext(dev, 0, 1))
    eng.load_weights(synth.iter_synth(synth.llama_param_shapes(cfg, 64), seed=1, device=dev, dtype=BF16))
    eng.pack_bf16(head_form=True)
    assert [eng._pack[k]["rows"] for k in ("0.wqkv", "0.wo", "0.wgu", "0.wdown")] == [4, 2, 4, 2]
    eng.use_bf16_pack(True)
    L = _lib()
    for N, K, epi, R in ((19968, 6656, EPI_NONE, 4), (6656, 6656, EPI_RESID, 2), (35840, 6656, EPI_SWIGLU, 4), (6656, 17920, EPI_RESID, 2)):
        assert L.emu_llama_pack_thin_kernel(0, 5, R, N, K, 1, 1, N, K, 0, epi, 0) == 8
    g = torch.Generator().manual_seed(2)
    eng.alloc_kv(1, 64)
    kv0 = (torch.randn(2, 1, 1, 52, 64, 128, generator=g) * 0.5).to(BF16).to(dev)
    x = (torch.randn(5, 6656, generator=g) * 0.5).to(BF16).to(dev)
    at = torch.tensor([59], device=dev, dtype=torch.int32)
    kstart = torch.zeros(1, device=dev, dtype=torch.int32)
    outs = {}
    for on in (True, False, True):
        eng.use_bf16_pack_wide(on)
        eng.kcache.copy_(kv0[0]); eng.vcache.copy_(kv0[1])
        h = eng.forward_chunk(x.clone(), 1, 5, at, at, kstart, 64)
        torch.cuda.synchronize()
        got = (h.clone(), eng.kcache[0, 0, :, 59:64].clone(), eng.vcache[0, 0, :, 59:64].clone())
        if on in outs:
            for a, b in zip(got, outs[on]):
                assert torch.equal(bits(a), bits(b))
        outs[on] = got
    assert bool(torch.isfinite(outs[True][0].float()).all())
    assert not torch.equal(bits(outs[True][1]), bits(kv0[0][0, 0, :, 59:64]))       # the step appended its K rows
    for a, b in zip(outs[True], outs[False]):
        assert torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_output_untouched():
    from emu_amd import ops
    from emu_amd._lib import Bf16PackSetC
    L = _lib()
    W = _matrix(64, 1792, seed=1).cuda()
    for M, K, rows in ((3, 256, None), (17, 256, None), (5, 896, None), (5, 256, 0)):
        Wk = W[:, :K].contiguous()
        p = ops.pack_bf16_rows(Wk, 2)
        s = ops.pack_set_c(p)
        if rows is not None:
            s = Bf16PackSetC(s.lo, s.nib, s.sign, s.flags, s.hb, rows)
        x = torch.ones(M, K, dtype=BF16, device="cuda")
        out = torch.full((M, 64), 1.5, dtype=BF16, device="cuda")
        st = L.emu_linear_bf16pack_thin(x.data_ptr(), Wk.data_ptr(), C.byref(s), None, out.data_ptr(), M, 64, K, EPI_NONE, ops.stream(x))
        torch.cuda.synchronize()
        assert st == -22 and bool((out == 1.5).all()), (M, K, rows)
    x = torch.ones(5, 256, dtype=BF16, device="cuda")
    Wk = W[:, :256].contiguous()
    assert bool(torch.isfinite(ops.linear_bf16pack_thin(x, Wk, ops.pack_bf16_rows(Wk, 2)).float()).all())      # the same call, accepted


def test_use_bf16_pack_wide_after_release_raises():
    from emu_amd._lib import EmuHipError
    eng = _engine()
    eng.use_fp4(True, wide=True, all_rows=True)
    eng.release_bf16()
    with pytest.raises(EmuHipError, match="released"):
        eng.use_bf16_pack_wide(True)
    assert not eng.bf16_pack_wide
