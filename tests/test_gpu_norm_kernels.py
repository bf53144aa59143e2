"""GPU: the row-wise kernels on their own -- rmsnorm_kernel, layernorm_kernel, softmax_rows_kernel (csrc/elementwise.hip),
gn_stats_kernel / gn_apply_kernel and cfg_euler_kernel (csrc/unet.hip) -- against float64 references written from the definition,
every element under a bound derived from the kernels' code.  The references, the bounds with their derivation, the case tables
and the input kinds are in tests/norm_cases.py; tests/test_norm_bound_host.py shows without a GPU that plain fp32 restatements of
the kernels stay within these bounds (RESTATED_WORST below) and that restatements with one deliberate error each leave them.

Exact, on integer views so that NaN patterns compare: a second launch of every case; an all-zero RMSNorm row; equal logits over a
power-of-two column count (1 / cols); the CFG + Euler step against both of its references; whatever lies around a strided
output, in the gaps of a strided softmax input and behind GroupNorm's workspace; refused arguments write nothing.

The kernels' worst ratio to the bound per kernel and input kind on MI355X is MEASURED below (each test prints its own as
"MEASURED [kernel kind] ratio")."""
import pytest
import torch

from tests import norm_cases as N

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

# worst |restatement - ref| / bound per kernel over every case and input kind (CPU, tests/test_norm_bound_host.py; GroupNorm without
# its 13200-pixel case)
RESTATED_WORST = {"rmsnorm": 0.953, "layernorm": 0.965, "groupnorm": 0.976, "softmax": 0.975}
# worst |kernel - ref| / bound on MI355X per kernel and input kind.  No ratio is above 1.0: none of the paths these cases reach for
# the first time (strided RMSNorm, the wide-row and few-group GroupNorm branches, the 2-way slice split, the second trip of the
# chunk fold, biased and strided softmax, the Euler step alone) turned out wrong.  The worst elements are decided by the bf16
# roundings, which kernel and restatement perform alike, so most figures equal the restatement's to the digits printed.
MEASURED = {
    "rmsnorm": {"rand": 0.843, "outlier": 0.900, "tiny": 0.953, "zero_row": 0.821},
    "layernorm": {"rand": 0.965, "rand+res": 0.949, "offset": 0.674, "offset+res": 0.726, "flat": 0.000, "flat+res": 0.116},
    "groupnorm": {"rand": 0.976, "rand+silu": 0.867, "coded": 0.975, "coded+silu": 0.864, "flat": 0.024, "flat+silu": 0.260},
    "softmax": {"rand": 0.975, "spike": 0.957, "uniform": 0.004, "bias": 0.972, "padded": 0.903},
}
# GroupNorm's 13200-pixel case alone (no CPU restatement): rand 0.969, coded 0.969, flat 0.002; with SiLU 0.862, 0.864, 0.114


def _ops():
    from emu_amd import ops
    return ops


def _lib():
    from emu_amd._lib import lib
    return lib()


def _measured(kernel, kind, r):
    print(f"MEASURED [{kernel} {kind}] {r:.3f}")
    assert r <= 1.0, (kernel, kind, r)


def _nan_buffer(*shape):
    """A bf16 GPU buffer of NaN bit patterns, and the same patterns as int16 on the CPU."""
    n = 1
    for s in shape:
        n *= s
    pat = N.nan_pattern(n).view(*shape)
    return pat.cuda().view(BF16), pat


def _sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ RMSNorm
@pytest.mark.parametrize("cols", N.RMS_COLS)
def test_rmsnorm_against_the_reference(cols):
    ops = _ops()
    for rows in N.RMS_ROWS:
        for kind in N.RMS_KINDS:
            x, w = N.rms_inputs(rows, cols, kind)
            ref, bound = N.rms_reference(x, w)
            xd, wd = x.cuda(), w.cuda()
            got = ops.rmsnorm(xd, wd, N.RMS_EPS).cpu()
            _measured("rmsnorm", kind, N.ratio_to_bound(got, ref, bound))
            if kind == "zero_row":
                assert bool((N.bits(got[rows // 2]) == 0).all()), "an all-zero row is not exactly zero"
            assert N.same_bits(got, ops.rmsnorm(xd, wd, N.RMS_EPS).cpu()), (rows, kind)


@pytest.mark.parametrize("cols", N.RMS_COLS)
def test_rmsnorm_strided(cols):
    """x is a 16-byte-aligned column slice of a wider buffer (ldx = cols + 8), out a slice of a wider NaN-pattern buffer
    (ldy = cols + 16): the bits of the contiguous launch, and the gaps keep theirs."""
    ops = _ops()
    rows = 3
    for kind in N.RMS_KINDS:
        x, w = N.rms_inputs(rows, cols, kind)
        ref, bound = N.rms_reference(x, w)
        xbuf, _ = _nan_buffer(rows, cols + 8)
        xs = xbuf[:, 8:]
        xs.copy_(x)
        obuf, pat = _nan_buffer(rows, cols + 16)
        out = obuf[:, 8:8 + cols]
        assert xs.stride(0) == cols + 8 and out.stride(0) == cols + 16 and xs.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
        ops.rmsnorm(xs, w.cuda(), N.RMS_EPS, out=out)
        _sync()
        got = out.cpu()
        _measured("rmsnorm", kind, N.ratio_to_bound(got, ref, bound))
        assert N.same_bits(got, ops.rmsnorm(x.cuda(), w.cuda(), N.RMS_EPS).cpu()), kind
        after = N.bits(obuf).cpu()
        assert torch.equal(after[:, :8], pat[:, :8]) and torch.equal(after[:, 8 + cols:], pat[:, 8 + cols:]), kind


# ------------------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("cols", N.LN_COLS)
def test_layernorm_against_the_reference(cols):
    """Plain, with a residual, and with the output aliasing the residual (the ViT engine's in-place form)."""
    ops = _ops()
    for kind in N.LN_KINDS:
        x, w, b, res = N.ln_inputs(cols, kind)
        xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
        ref, bound = N.ln_reference(x, w, b)
        got = ops.layernorm(xd, wd, bd, N.LN_EPS).cpu()
        _measured("layernorm", kind, N.ratio_to_bound(got, ref, bound))
        assert N.same_bits(got, ops.layernorm(xd, wd, bd, N.LN_EPS).cpu()), kind
        ref, bound = N.ln_reference(x, w, b, res)
        rd = res.cuda()
        got = ops.layernorm(xd, wd, bd, N.LN_EPS, res=rd).cpu()
        _measured("layernorm", kind + "+res", N.ratio_to_bound(got, ref, bound))
        assert N.same_bits(rd.cpu(), res), "the residual was written"
        assert N.same_bits(got, ops.layernorm(xd, wd, bd, N.LN_EPS, res=rd).cpu()), kind
        ops.layernorm(xd, wd, bd, N.LN_EPS, res=rd, out=rd)
        assert N.same_bits(rd.cpu(), got), (kind, "out aliases res")


# ------------------------------------------------------------------------------------------------------------ GroupNorm
def _gid(c):
    return f"C{c.C}-G{c.G}-HW{c.HW}-B{c.B}"


@pytest.mark.parametrize("c", N.GN_CASES, ids=_gid)
def test_groupnorm_against_the_reference(c):
    """With and without SiLU.  The 13200-pixel case keeps its inputs and builds its float64 reference on the GPU with torch."""
    ops = _ops()
    dev = "cuda" if c == N.GN_BIG else "cpu"
    for kind in N.GN_KINDS:
        x, gamma, beta = N.gn_inputs(c, kind, dev)
        ref, bound, s, bound_s = N.gn_reference(x, gamma, beta, c.G)
        xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
        for silu in (False, True):
            got = ops.groupnorm_nhwc(xd, gd, bd, c.G, N.GN_EPS, silu)
            again = ops.groupnorm_nhwc(xd, gd, bd, c.G, N.GN_EPS, silu)
            assert N.same_bits(got, again), (kind, silu)
            del again
            r = N.ratio_to_bound(got.to(dev), s if silu else ref, bound_s if silu else bound)
            _measured("groupnorm", kind + ("+silu" if silu else ""), r)
        del ref, bound, s, bound_s


def test_groupnorm_keeps_to_its_buffers():
    """emu_groupnorm_nhwc_bf16 itself: y sits inside a larger NaN-pattern buffer, the workspace is exactly emu_groupnorm_ws_bytes
    long with a canary behind it; both surroundings keep their bits and y has the bits of the plain call."""
    ops, L = _ops(), _lib()
    c = N.GN_CASES[1]                                                        # three chunks, four slices, idle row groups
    x, gamma, beta = N.gn_inputs(c, "coded")
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    want = ops.groupnorm_nhwc(xd, gd, bd, c.G, N.GN_EPS, True).cpu()
    n, front = c.B * c.HW * c.C, 64
    ybuf, pat = _nan_buffer(front + n + 64)
    need = L.emu_groupnorm_ws_bytes(c.B, c.HW, c.C)
    assert need > 0 and need % 4 == 0
    canary = (torch.arange(need + 256, dtype=torch.int64) * 37 % 251).to(torch.uint8)
    ws = canary.cuda()
    y = ybuf[front:front + n]
    assert y.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0
    st = L.emu_groupnorm_nhwc_bf16(ops._p(xd), ops._p(gd), ops._p(bd), ops._p(y), ops._p(ws), c.B, c.HW, c.C, c.G, N.GN_EPS, 1,
                                   ops.stream(xd))
    _sync()
    assert st == 0
    assert N.same_bits(y.cpu().view(c.B, c.HW, c.C), want)
    after = N.bits(ybuf).cpu()
    assert torch.equal(after[:front], pat[:front]) and torch.equal(after[front + n:], pat[front + n:])
    assert torch.equal(ws.cpu()[need:], canary[need:]), "written behind the workspace"
    assert not torch.equal(ws.cpu()[:need], canary[:need])


# ------------------------------------------------------------------------------------------------------------ softmax
@pytest.mark.parametrize("cols", N.SM_COLS)
def test_softmax_against_the_reference(cols):
    ops = _ops()
    for rows in N.SM_ROWS:
        for kind in N.SM_KINDS:
            x, bias, scale = N.sm_inputs(rows, cols, kind)
            ref, bound = N.sm_reference(x, bias, scale)
            bd = None if bias is None else bias.cuda()
            got = ops.softmax_rows_(x.cuda(), scale, bias=bd).cpu()
            _measured("softmax", kind, N.ratio_to_bound(got, ref, bound))
            if kind == "uniform" and cols & (cols - 1) == 0:
                assert bool((got.float() == 1.0 / cols).all()), "equal logits do not give 1 / cols exactly"
            assert N.same_bits(got, ops.softmax_rows_(x.cuda(), scale, bias=bd).cpu()), (rows, kind)
            if bias is not None:
                assert N.same_bits(bd.cpu(), bias)


@pytest.mark.parametrize("cols", N.SM_COLS)
def test_softmax_strided(cols):
    """x and the bias are column slices of wider buffers with different leading dimensions (cols + 8, cols + 16); the gaps of x
    hold NaN patterns and keep them; the result has the bits of the contiguous launch."""
    ops = _ops()
    rows = 7
    for kind in N.SM_KINDS:
        x, bias, scale = N.sm_inputs(rows, cols, kind)
        xbuf, pat = _nan_buffer(rows, cols + 8)
        xs = xbuf[:, :cols]
        xs.copy_(x)
        bs = None
        if bias is not None:
            bbuf, _ = _nan_buffer(rows, cols + 16)
            bs = bbuf[:, 8:8 + cols]
            bs.copy_(bias)
            assert bs.stride(0) != xs.stride(0)
        want = ops.softmax_rows_(x.cuda(), scale, bias=None if bias is None else bias.cuda()).cpu()
        ops.softmax_rows_(xs, scale, bias=bs)
        _sync()
        assert N.same_bits(xs.cpu(), want), kind
        assert torch.equal(N.bits(xbuf).cpu()[:, cols:], pat[:, cols:]), kind


# ------------------------------------------------------------------------------------------------------------ CFG + Euler
@pytest.fixture(scope="module")
def bare_unet():
    """A UNetEngine of the tiny configuration of test_gpu_unet.py, without weights: the step needs its channel count only."""
    from emu_amd.llama import EmuHipContext
    from emu_amd.unet import UNetCfg, UNetEngine
    cfg = UNetCfg(block_out_channels=(64, 128, 256), transformer_layers_per_block=(1, 1, 2), num_heads=(1, 2, 4),
                  cross_attention_dim=128, projection_class_embeddings_input_dim=128 + 6 * 256)
    eng = UNetEngine(cfg, EmuHipContext(torch.device("cuda", 0)))
    assert cfg.in_channels == N.EULER_C
    eng.set_timesteps(N.EULER_STEPS_N)
    return eng


@pytest.mark.parametrize("H,W", N.EULER_MAPS)
def test_cfg_euler_step_is_exact(bare_unet, H, W):
    """emu_unet_cfg_euler_step against the chain restated op by op and against the scheduler's own update in bf16 torch ops, bit
    for bit; the step counter rises by exactly one and the noise pair keeps its bits."""
    ops, L, eng = _ops(), _lib(), bare_unet
    sig = N.euler_sigmas()
    assert N.same_bits(eng.sigmas.cpu(), sig)
    for step in N.EULER_STEPS:
        eps, lat = N.euler_inputs(H, W, step)
        for g in N.EULER_GUIDANCE:
            want = N.euler_chain(eps, lat, sig, step, g)
            assert N.same_bits(want, N.euler_torch(eps, lat, sig, step, g)), (step, g)
            outs = []
            for _ in range(2):
                pair, x = eps.cuda(), lat.cuda()
                eng.step_dev.fill_(step)
                st = L.emu_unet_cfg_euler_step(eng.handle, pair.data_ptr(), x.data_ptr(), H, W, eng.sigmas.data_ptr(),
                                               eng.step_dev.data_ptr(), g, ops.stream(x))
                _sync()
                assert st == 0
                assert int(eng.step_dev.item()) == step + 1
                assert N.same_bits(pair.cpu(), eps)
                outs.append(x.cpu())
            assert N.same_bits(outs[0], want), (step, g)
            assert N.same_bits(outs[0], outs[1]), (step, g)
    eng.step_dev.zero_()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refused_arguments_write_nothing():
    """Columns or channels that are no multiple of 8, channels that are no multiple of the group count, more than 32 groups, more
    than 2560 channels: the entry returns -22 and the output keeps its bits."""
    ops, L = _ops(), _lib()
    rows, cols = 2, 16
    x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(5)).to(BF16).cuda()
    w = torch.ones(cols, dtype=BF16).cuda()
    out, pat = _nan_buffer(rows, cols)
    s = ops.stream(x)
    calls = {
        "rmsnorm cols 12": lambda: L.emu_rmsnorm_bf16(ops._p(x), ops._p(w), ops._p(out), rows, 12, cols, cols, 1e-6, s),
        "rmsnorm ldx 12": lambda: L.emu_rmsnorm_bf16(ops._p(x), ops._p(w), ops._p(out), rows, 8, 12, cols, 1e-6, s),
        "rmsnorm ldy 12": lambda: L.emu_rmsnorm_bf16(ops._p(x), ops._p(w), ops._p(out), rows, 8, cols, 12, 1e-6, s),
        "layernorm cols 12": lambda: L.emu_layernorm_bf16(ops._p(x), ops._p(w), ops._p(w), None, ops._p(out), rows, 12, 1e-6, s),
        "softmax cols 12": lambda: L.emu_softmax_rows_bf16(ops._p(out), None, rows, 12, cols, 0, 1.0, s),
        "softmax ld 12": lambda: L.emu_softmax_rows_bf16(ops._p(out), None, rows, 8, 12, 0, 1.0, s),
        "softmax ld_bias 12": lambda: L.emu_softmax_rows_bf16(ops._p(out), ops._p(x), rows, 8, cols, 12, 1.0, s),
    }
    for what, call in calls.items():
        assert call() == -22, what
        _sync()
        assert torch.equal(N.bits(out).cpu(), pat), what
    # GroupNorm: (C, groups); buffers sized for the widest of them
    B, HW = 1, 2
    xg = torch.zeros(B, HW, 2568, dtype=BF16).cuda()
    gb = torch.ones(2568, dtype=BF16).cuda()
    y, ypat = _nan_buffer(B * HW * 2568)
    ws = torch.zeros(L.emu_groupnorm_ws_bytes(B, HW, 2568), dtype=torch.uint8).cuda()
    for C, groups in ((36, 4), (64, 3), (64, 64), (2568, 1)):
        st = L.emu_groupnorm_nhwc_bf16(ops._p(xg), ops._p(gb), ops._p(gb), ops._p(y), ops._p(ws), B, HW, C, groups, 1e-5, 0, s)
        assert st == -22, (C, groups)
        _sync()
        assert torch.equal(N.bits(y).cpu(), ypat) and not bool(ws.any()), (C, groups)
