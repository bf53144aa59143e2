"""GPU: the tiled bf16 GEMM on its own -- the lock-step tiles of csrc/gemm.hip, the eight- and four-wave 256 x 256 tiles of
csrc/gemm256.hip / csrc/gemm_w4.hip, their K-sliced forms with both reduce kernels, the hybrid split, and the epilogues and the
3 x 3 gather of csrc/gemm_tile.h -- through emu_amd.ops, against float64 references written from the definition, every element
under a bound derived from the kernels' rounding points.  The references, the bounds with their derivation, the case tables (each
case with the plan emu_gemm_plan gives it) and the input kinds are in tests/gemm_cases.py; tests/test_gemm_bound_host.py shows
without a GPU that a plain fp32 restatement of the tiles stays within these bounds (RESTATED_WORST below), that restatements with
one deliberate error each leave them, and that every case reaches the form its table records.

The cases are tile edges rather than workload shapes: a tile's rows minus one, exactly one tile and one more (the 256 x 256 tile also
at 272 / 273 / 288 / 289 rows, around the remainder rows it folds into its last tile row); N % 4 == 3 (scalar stores), N % 4 == 2
under a GLU, one tile column and a part, an ldc that is no multiple of 4; K = 8, 64, 72, 200 on the lock-step tiles, three k tiles,
the longest unsliced and the shortest sliced K, 17 k tiles in two slices; every epilogue on every tile.

Exact, on integer views so that NaN patterns compare: the ``coded`` kind under NONE / RESID and every ``coded`` conv; the one-hot tap
test of the gather (no tolerance); a second launch of every case; tiles that accumulate in the same k order (B, C, Q, and P / W where
unsliced); staged against direct stores; strided A / W / res with NaN patterns in their gaps against the contiguous launch; whatever
lies around C (always a slice of a NaN-pattern buffer with spare rows) and behind the slices a plan needs in the split-K scratch;
refused arguments write nothing.

A conv whose Hout does not match its mode cannot be expressed through emu_conv3x3_nhwc_bf16 (it derives Hout from the mode); the
planner's refusal of it is asserted on the CPU in tests/test_gemm_bound_host.py.  ops.conv3x3_nhwc allocates its own output, so the
refused conv is sent through the same C symbol with a NaN-pattern output.

The kernels' worst ratio to the bound per tile, epilogue and input kind on MI355X is MEASURED below (each test prints its own as
"MEASURED [tile epilogue kind] ratio")."""
import pytest
import torch

from tests import gemm_cases as G

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
GUARD = 1 << 16                                  # fp32 elements behind the registered scratch
SCRATCH_PATTERN = 0x7FC5A5A5                     # an fp32 NaN

# worst |restatement - ref| / bound per epilogue over every case and kind (CPU, tests/test_gemm_bound_host.py)
RESTATED_WORST = {"none": 0.975, "resid": 0.965, "swiglu": 0.783, "silu": 0.851, "gelu": 0.909, "geglu": 0.788, "conv": 0.905}
# worst |kernel - ref| / bound on MI355X per tile (BCQ: the same-k-order test, H: the hybrid split, conv-<config>, conv-slow-<config>:
# the slow gather), epilogue (conv: mode) and input kind.  No ratio is above 1.0, every ``coded`` case and every tap is exact, and no
# bit outside C or behind a plan's slices changed: none of the edges these cases reach for the first time (scalar stores, odd-width
# GLU outputs, remainder rows, ragged K under strides, two-slice reduces of both kinds, the hybrid's second launch, the slow gather)
# turned out wrong.  The worst elements are decided by the bf16 roundings, which kernel and restatement perform alike; the slow
# gather's bound is dominated by e_acc at K = 37440 (its exact checks are the sharp ones).
MEASURED = {
    "B": {"none": {"rand": 0.973, "offset": 0.973, "coded": 0.975}, "resid": {"rand": 0.960, "offset": 0.962, "coded": 0.958}, "swiglu": {"rand": 0.703, "offset": 0.744, "coded": 0.449},
          "silu": {"rand": 0.846, "offset": 0.819, "coded": 0.426}, "gelu": {"rand": 0.890, "offset": 0.870, "coded": 0.420}, "geglu": {"rand": 0.682, "offset": 0.668, "coded": 0.423}},
    "C": {"none": {"rand": 0.974, "offset": 0.974, "coded": 0.975}, "resid": {"rand": 0.965, "offset": 0.948, "coded": 0.959}, "swiglu": {"rand": 0.663, "offset": 0.707, "coded": 0.449},
          "silu": {"rand": 0.820, "offset": 0.825, "coded": 0.426}, "gelu": {"rand": 0.909, "offset": 0.864, "coded": 0.420}, "geglu": {"rand": 0.701, "offset": 0.757, "coded": 0.545}},
    "K": {"none": {"rand": 0.963, "offset": 0.968, "coded": 0.975}, "resid": {"rand": 0.961, "offset": 0.959, "coded": 0.958}, "swiglu": {"rand": 0.770, "offset": 0.706, "coded": 0.449},
          "silu": {"rand": 0.812, "offset": 0.815, "coded": 0.426}, "gelu": {"rand": 0.863, "offset": 0.838, "coded": 0.420}, "geglu": {"rand": 0.724, "offset": 0.627, "coded": 0.423}},
    "S": {"none": {"rand": 0.972, "offset": 0.970, "coded": 0.958}, "resid": {"rand": 0.962, "offset": 0.950, "coded": 0.959}, "swiglu": {"rand": 0.663, "offset": 0.707, "coded": 0.449},
          "silu": {"rand": 0.820, "offset": 0.825, "coded": 0.426}, "gelu": {"rand": 0.909, "offset": 0.864, "coded": 0.420}, "geglu": {"rand": 0.701, "offset": 0.768, "coded": 0.545}},
    "P": {"none": {"rand": 0.973, "offset": 0.970, "coded": 0.958}, "resid": {"rand": 0.965, "offset": 0.959, "coded": 0.959}, "swiglu": {"rand": 0.731, "offset": 0.783, "coded": 0.449},
          "silu": {"rand": 0.851, "offset": 0.827, "coded": 0.426}, "gelu": {"rand": 0.908, "offset": 0.871, "coded": 0.420}, "geglu": {"rand": 0.690, "offset": 0.702, "coded": 0.545}},
    "Q": {"none": {"rand": 0.973, "offset": 0.970, "coded": 0.958}, "resid": {"rand": 0.965, "offset": 0.959, "coded": 0.959}, "swiglu": {"rand": 0.686, "offset": 0.689, "coded": 0.449},
          "silu": {"rand": 0.851, "offset": 0.827, "coded": 0.426}, "gelu": {"rand": 0.908, "offset": 0.871, "coded": 0.420}, "geglu": {"rand": 0.777, "offset": 0.788, "coded": 0.545}},
    "W": {"none": {"rand": 0.973, "offset": 0.970, "coded": 0.958}, "resid": {"rand": 0.965, "offset": 0.959, "coded": 0.959}, "swiglu": {"rand": 0.686, "offset": 0.689, "coded": 0.449},
          "silu": {"rand": 0.851, "offset": 0.827, "coded": 0.426}, "gelu": {"rand": 0.908, "offset": 0.871, "coded": 0.420}, "geglu": {"rand": 0.777, "offset": 0.788, "coded": 0.545}},
    "BCQ": {"none": {"rand": 0.968}, "resid": {"rand": 0.940}, "swiglu": {"rand": 0.635},
          "gelu": {"rand": 0.717}, "geglu": {"rand": 0.549}},
    "H": {"none": {"rand": 0.916, "coded": 0.623}, "resid": {"rand": 0.925, "coded": 0.759}, "swiglu": {"rand": 0.750, "coded": 0.453}},
    "conv-0": {"mode1": {"rand": 0.898, "coded": 0.852}, "mode2": {"rand": 0.896, "coded": 0.787}, "mode3": {"rand": 0.907, "coded": 0.828}},
    "conv-B": {"mode1": {"rand": 0.898, "coded": 0.852}, "mode2": {"rand": 0.896, "coded": 0.787}, "mode3": {"rand": 0.907, "coded": 0.828}},
    "conv-C": {"mode1": {"rand": 0.898, "coded": 0.852}, "mode2": {"rand": 0.896, "coded": 0.787}, "mode3": {"rand": 0.907, "coded": 0.828}},
    "conv-K": {"mode1": {"rand": 0.898, "coded": 0.852}, "mode2": {"rand": 0.896, "coded": 0.787}, "mode3": {"rand": 0.907, "coded": 0.828}},
    "conv-P": {"mode1": {"rand": 0.898, "coded": 0.852}, "mode2": {"rand": 0.896, "coded": 0.787}, "mode3": {"rand": 0.907, "coded": 0.828}},
    "conv-Q": {"mode1": {"rand": 0.898, "coded": 0.852}, "mode2": {"rand": 0.896, "coded": 0.787}, "mode3": {"rand": 0.907, "coded": 0.828}},
    "conv-W": {"mode1": {"rand": 0.898, "coded": 0.852}, "mode2": {"rand": 0.896, "coded": 0.787}, "mode3": {"rand": 0.907, "coded": 0.828}},
    "conv-slow-0": {"mode1": {"rand": 0.019, "coded": 0.001}},
    "conv-slow-K": {"mode1": {"rand": 0.019, "coded": 0.001}},
    "conv-slow-B": {"mode1": {"rand": 0.019, "coded": 0.001}},
    "conv-slow-C": {"mode1": {"rand": 0.019, "coded": 0.001}},
    "conv-slow-Q": {"mode1": {"rand": 0.019, "coded": 0.001}},
}


def _ops():
    from emu_amd import ops
    return ops


def _lib():
    from emu_amd._lib import lib
    return lib()


def _measured(tile, epilogue, kind, r, what=""):
    print(f"MEASURED [{tile} {epilogue} {kind}] {r:.3f}")
    assert r <= 1.0, (tile, epilogue, kind, r, what)


def _nan_buffer(*shape):
    """A bf16 GPU buffer of NaN bit patterns, and the same patterns as int16 on the CPU."""
    n = 1
    for s in shape:
        n *= s
    pat = G.nan_pattern(n).view(*shape)
    return pat.cuda().view(BF16), pat


class _Gemm:
    """Pins a config, launches into guarded buffers, watches the split-K scratch."""

    def __init__(self, L):
        self.L = L
        self.scratch = torch.full((G.SCRATCH_FLOATS + GUARD,), SCRATCH_PATTERN, dtype=torch.int32, device="cuda")
        L.emu_set_splitk_scratch(self.scratch.data_ptr(), G.SCRATCH_FLOATS * 4)

    def use(self, cfg, extra_tune=0):
        force, tune = ("0", 0) if cfg == "0" else G.CONFIGS[cfg][:2] if cfg in G.CONFIGS else (cfg, 0)
        self.force, self.tune = force, tune | extra_tune
        self.L.emu_gemm_tune(self.tune)
        self.L.emu_gemm_force_config(0 if force == "0" else ord(force))

    def scratch_untouched_behind(self, need, what):
        """Everything behind the first ``need`` floats still holds the pattern; then the used part is patterned again."""
        assert need <= G.SCRATCH_FLOATS, what
        assert bool((self.scratch[need:] == SCRATCH_PATTERN).all()), f"{what}: the scratch was written behind its {need} floats"
        if need:
            self.scratch[:need] = SCRATCH_PATTERN

    def need(self, M, N, K, epi, conv=(0, 0, 0, 0, 0, 0)):
        st, entries = G.plan_query(M, N, K, G.plan_epi(N, epi), self.force, self.tune, conv)
        assert st == 0
        return max(G.scratch_need(p, full, M, n, conv[0] != 0) for p, full, _, n in entries)

    def linear(self, x, w, bias, res, epi, pad, what):
        """ops.linear into the top-left corner of a NaN-pattern buffer pad columns wider and two rows taller -> the result on the
        CPU; everything outside [M, columns] keeps its bits."""
        M, N = x.shape[0], w.shape[0]
        nout = N // 2 if epi in G.GLU else N
        buf, pat = _nan_buffer(M + 2, nout + pad)
        out = buf[:M, :nout]
        assert out.stride(0) == nout + pad
        _ops().linear(x, w, bias=bias, res=res if epi == G.EPI_RESID else None, epi=epi, out=out)
        torch.cuda.synchronize()
        after = G.bits(buf).cpu()
        assert torch.equal(after[M:], pat[M:]), f"{what}: rows behind M were written"
        assert torch.equal(after[:M, nout:], pat[:M, nout:]), f"{what}: columns behind N were written"
        return after[:M, :nout].contiguous().view(BF16)


@pytest.fixture()
def gemm():
    L = _lib()
    g = _Gemm(L)
    try:
        yield g
    finally:
        L.emu_gemm_force_config(0)
        L.emu_gemm_tune(0)
        L.emu_set_splitk_scratch(0, 0)


def _cid(c):
    return f"{c.cfg} {c.M}x{c.N}x{c.K} pad {c.pad}"


def _cases(cfg):
    return [c for c in G.CASES if c.cfg == cfg]


def _dev(M, N, K, kind):
    return tuple(t.cuda() for t in G.gemm_inputs(M, N, K, kind))


# ------------------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("cfg", list(G.CONFIGS))
def test_gemm_tile_edges_against_the_reference(gemm, cfg):
    """Every case of the table, every kind and epilogue: ratio to the bound at most 1.0 on every element, ``coded`` exact under NONE /
    RESID, a second (contiguous, where C may be) launch with the same bits, nothing written around C or behind the plan's slices."""
    ops = _ops()
    worst, bad = {}, []
    gemm.use(cfg)
    for c in _cases(cfg):
        for kind in G.KINDS:
            x, w, bias, res = _dev(c.M, c.N, c.K, kind)
            for epi in c.epis:
                what = f"{_cid(c)} {G.EPI_NAMES[epi]} {kind}"
                ref, bound = G.gemm_reference(c.M, c.N, c.K, kind, epi)
                got = gemm.linear(x, w, bias, res, epi, c.pad, what)
                r = G.ratio_to_bound(got, ref, bound)
                key = (G.EPI_NAMES[epi], kind)
                worst[key] = max(worst.get(key, 0.0), r)
                if r > 1.0:
                    bad.append((what, r))
                if kind == "coded" and epi in (G.EPI_NONE, G.EPI_RESID) and not G.same_bits(got, G.gemm_exact(c.M, c.N, c.K, epi)):
                    bad.append((what, "coded: not the exact bits"))
                if epi in G.GLU and (c.N // 2) % 2:                          # a contiguous C of odd width is refused under a GLU
                    rep = gemm.linear(x, w, bias, res, epi, c.pad, what)
                else:
                    rep = ops.linear(x, w, bias=bias, res=res if epi == G.EPI_RESID else None, epi=epi).cpu()
                gemm.scratch_untouched_behind(gemm.need(c.M, c.N, c.K, epi), what)
                if not G.same_bits(got, rep):
                    bad.append((what, "a second launch differs"))
    for (e, kind), r in worst.items():
        print(f"MEASURED [{cfg} {e} {kind}] {r:.3f}")
    assert not bad, bad[:20]


@pytest.mark.parametrize("cfg", list(G.CONFIGS))
def test_staged_and_direct_epilogues_store_the_same_bits(gemm, cfg):
    """emu_gemm_tune bit 3 switches the staged epilogue off: the same bits, and the same untouched surroundings, on every case whose
    plan stages (a whole tile column inside N next to a ragged one, ragged rows, remainder rows, K-sliced forms)."""
    n = 0
    for c in _cases(cfg):
        if not c.plan.stage & 1:
            continue
        x, w, bias, res = _dev(c.M, c.N, c.K, "rand")
        for epi in c.epis:
            outs = []
            for extra in (0, G.TUNE_DIRECT):
                gemm.use(cfg, extra)
                outs.append(gemm.linear(x, w, bias, res, epi, c.pad, f"{_cid(c)} epi {epi} tune {extra}"))
                gemm.scratch_untouched_behind(gemm.need(c.M, c.N, c.K, epi), _cid(c))
            assert G.same_bits(*outs), f"{_cid(c)} epi {epi}: staged != direct"
            n += 1
    assert n >= 6


SAME_ORDER = [(257, 259, 64, G.EPI_NONE), (273, 320, 192, G.EPI_RESID), (129, 136, 128, G.EPI_SWIGLU), (127, 264, 960, G.EPI_GELU),
              (289, 264, 1088, G.EPI_NONE), (272, 272, 1024, G.EPI_GEGLU)]


@pytest.mark.parametrize("M,N,K,epi", SAME_ORDER)
def test_tiles_with_the_same_k_order_store_the_same_bits(gemm, M, N, K, epi):
    """B, C and Q accumulate every output over the k tiles in order, one k-group, no slices: equal bits -- and so do P and W below
    K = 1024, where they are not sliced (the four-wave tile keeps the ping-pong tile's order)."""
    x, w, bias, res = _dev(M, N, K, "rand")
    outs = {}
    for cfg in ("B", "C", "Q") + (("P", "W", "S") if K < 1024 else ()):
        gemm.use(cfg)
        assert gemm.need(M, N, K, epi) == 0
        outs[cfg] = gemm.linear(x, w, bias, res, epi, 8, f"{cfg} {M}x{N}x{K}")
    for cfg, o in outs.items():
        assert G.same_bits(o, outs["B"]), f"{cfg} != B at {M}x{N}x{K} epi {epi}: {int((G.bits(o) != G.bits(outs['B'])).sum())} elements"
    ref, bound = G.gemm_reference(M, N, K, "rand", epi)
    _measured("BCQ", G.EPI_NAMES[epi], "rand", G.ratio_to_bound(outs["B"], ref, bound))


@pytest.mark.parametrize("cfg", list(G.CONFIGS))
def test_strided_operands_with_nan_gaps_give_the_contiguous_bits(gemm, cfg):
    """A and W are column slices of buffers 56 columns wider (lda = ldw = K + 56, the ragged K = 72 and 200 among them), res of one 8
    wider; the gaps hold NaN patterns.  A kernel that reads a gap into a product, or takes one stride for another, cannot give the
    bits of the contiguous launch."""
    ops = _ops()
    n = 0
    gemm.use(cfg)
    for c in _cases(cfg):
        if c.K not in (72, 200, 64, 192, 1088) or c.M not in (65, 129, 257) or c.pad != 8:
            continue
        x, w, bias, res = _dev(c.M, c.N, c.K, "rand")
        xb, _ = _nan_buffer(c.M, c.K + 56)
        wb, _ = _nan_buffer(c.N, c.K + 56)
        rbuf, _ = _nan_buffer(c.M, c.N + 8)
        xs, ws, rs = xb[:, :c.K], wb[:, :c.K], rbuf[:, :c.N]
        xs.copy_(x), ws.copy_(w), rs.copy_(res)
        assert xs.stride(0) == ws.stride(0) == c.K + 56
        for epi in c.epis:
            if epi in G.GLU and (c.N // 2) % 2:
                continue
            want = ops.linear(x, w, bias=bias, res=res if epi == G.EPI_RESID else None, epi=epi).cpu()
            got = gemm.linear(xs, ws, bias, rs, epi, c.pad, _cid(c))
            assert G.same_bits(got, want), f"{_cid(c)} epi {epi}: strided operands change the result"
            n += 1
    assert n >= 4


def test_hybrid_split_against_the_reference(gemm):
    """The smallest problem found that takes the hybrid split (whole rounds on the 256 x 256 tile, the last 8 columns a second GEMM
    on the 128 x 64 tile): reference and comparison on the GPU.  GLU: the second launch's output starts at column col0 / 2."""
    M, N, K = G.HYBRID
    for kind in ("rand", "coded"):
        x, w, bias, res = _dev(M, N, K, kind)
        acc, mag = G.acc64(x, w)
        for epi in (G.EPI_NONE, G.EPI_RESID, G.EPI_SWIGLU):
            ref, bound = G.epilogue64(acc, mag, K, epi, bias=bias, res=res)
            for cfg in ("H", "0"):
                gemm.use(cfg)
                st, entries = G.plan_query(M, N, K, epi, gemm.force, gemm.tune)
                assert st == 0 and [e[2:] for e in entries] == [e[2:] for e in G.HYBRID_PLAN], entries
                got = gemm.linear(x, w, bias, res, epi, 8, f"hybrid {cfg} {kind} epi {epi}").cuda()
                gemm.scratch_untouched_behind(0, "hybrid")
                _measured("H", G.EPI_NAMES[epi], kind, G.ratio_to_bound(got, ref, bound))
                if kind == "coded" and epi != G.EPI_SWIGLU:
                    assert float(mag.max()) < 2 ** 24 - 64
                    assert G.same_bits(got, G.epilogue_chain(acc.float(), epi, bias=bias, res=res)), (cfg, epi)
            del ref, bound
        del acc, mag


def test_refused_arguments_write_nothing(gemm):
    """K % 8 != 0, an odd N under a GLU, a conv with Cin % 64 != 0: status -22 from the library, which ops raises, and the
    NaN-pattern output keeps its bits."""
    from emu_amd._lib import EmuHipError, check
    from emu_amd import ops
    gemm.use("0")
    xb = torch.randn(129, 104, device="cuda").to(BF16)
    wb = torch.randn(136, 104, device="cuda").to(BF16)
    buf, pat = _nan_buffer(129, 136)
    with pytest.raises(EmuHipError, match="status -22"):
        ops.linear(xb[:, :100], wb[:, :100], out=buf)                        # lda = ldw = 104: only K is wrong
    x, w = torch.randn(129, 128, device="cuda").to(BF16), torch.randn(135, 128, device="cuda").to(BF16)
    gbuf, gpat = _nan_buffer(129, 68)
    with pytest.raises(EmuHipError, match="status -22"):
        ops.linear(x, w, epi=G.EPI_SWIGLU, out=gbuf[:, :67])                 # ldc = 68 is even: only N is wrong
    cx, cw = torch.randn(3, 5, 8, 72, device="cuda").to(BF16), torch.randn(36, 3, 3, 72, device="cuda").to(BF16)
    ybuf, ypat = _nan_buffer(3 * 5 * 8, 36)
    st = _lib().emu_conv3x3_nhwc_bf16(cx.data_ptr(), cw.data_ptr(), 0, 0, 0, 0, ybuf.data_ptr(), 3, 5, 8, 72, 36, 1, ops.stream(cx))
    assert st == -22
    with pytest.raises(EmuHipError, match="status -22"):
        check(st, "emu_conv3x3_nhwc_bf16")
    with pytest.raises(EmuHipError, match="status -22"):
        ops.conv3x3_nhwc(cx, cw)
    torch.cuda.synchronize()
    assert torch.equal(G.bits(buf).cpu(), pat) and torch.equal(G.bits(gbuf).cpu(), gpat) and torch.equal(G.bits(ybuf).cpu(), ypat)
    gemm.scratch_untouched_behind(0, "refused")


# ------------------------------------------------------------------------------------------------------------ conv
def _conv_geo(mode, B, h, w, cin):
    ho, wo = G.conv_out_hw(mode, h, w)
    return B * ho * wo, (mode, h, w, ho, wo, cin)


@pytest.mark.parametrize("hw", G.CONV_IMAGES, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("mode", G.CONV_MODES)
def test_conv_against_the_reference(gemm, mode, hw):
    """Non-square images with an odd side, three batch rows (the batch changes inside a tile), bias, a per-batch bias2 that is a column
    slice of a wider table, and a residual, on every tile; the ``coded`` kind is exact (every fp32 sum is) whatever the k order."""
    ops = _ops()
    h, w = hw
    worst, bad = {}, []
    for cin, cout in G.CONV_CH:
        for kind in G.CONV_KINDS:
            x, wt, bias, b2, res = (t.cuda() for t in G.conv_inputs(mode, h, w, cin, cout, kind))
            cx, cw, cb, cb2, cres = G.conv_inputs(mode, h, w, cin, cout, kind)
            b2s = b2[:, 8:8 + cout]
            assert b2s.stride(0) == cout + 24
            for full in (True, False):
                ref, bound = G.conv_reference(cx, cw, mode, cb, cb2[:, 8:8 + cout] if full else None, cres if full else None)
                exact = G.conv_restate(cx, cw, mode, cb, cb2[:, 8:8 + cout] if full else None, cres if full else None) if kind == "coded" else None
                for cfg in G.CONV_CFGS:
                    what = f"conv mode {mode} {h}x{w} {cin}->{cout} {kind} cfg {cfg} full {full}"
                    gemm.use(cfg)
                    M, geo = _conv_geo(mode, G.CONV_B, h, w, cin)
                    got = ops.conv3x3_nhwc(x, wt, bias=bias, bias2=b2s if full else None, res=res if full else None, mode=mode)
                    rep = ops.conv3x3_nhwc(x, wt, bias=bias, bias2=b2s if full else None, res=res if full else None, mode=mode)
                    gemm.scratch_untouched_behind(gemm.need(M, cout, 9 * cin, int(full), geo), what)
                    got = got.cpu()
                    r = G.ratio_to_bound(got, ref, bound)
                    worst[(cfg, kind)] = max(worst.get((cfg, kind), 0.0), r)
                    if r > 1.0:
                        bad.append((what, r))
                    if not G.same_bits(got, rep.cpu()):
                        bad.append((what, "a second launch differs"))
                    if exact is not None and not G.same_bits(got, exact):
                        bad.append((what, "coded: not the exact bits"))
    for (cfg, kind), r in worst.items():
        print(f"MEASURED [conv-{cfg} mode{mode} {kind}] {r:.3f}")
    assert not bad, bad[:20]


@pytest.mark.parametrize("hw", G.CONV_IMAGES, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("mode", G.CONV_MODES)
def test_conv_taps_are_exact(gemm, mode, hw):
    """One-hot weights, one (tap, channel) per output channel, distinct bf16 pixels: every output is the source pixel conv_tap names,
    or +0 outside the image, bit for bit, on every tile.  No tolerance."""
    ops = _ops()
    h, w = hw
    for cin in (64, 128):
        x, wt = G.tap_inputs(G.CONV_B, h, w, cin)
        want = G.tap_expected(x, mode)
        xd, wd = x.cuda(), wt.cuda()
        for cfg in G.CONV_CFGS:
            gemm.use(cfg)
            got = ops.conv3x3_nhwc(xd, wd, mode=mode).cpu()
            bad = G.bits(got) != G.bits(want)
            assert not bool(bad.any()), f"mode {mode} {h}x{w} Cin {cin} cfg {cfg}: {int(bad.sum())} wrong, first at {bad.nonzero()[0].tolist()}"


def test_conv_slow_gather(gemm):
    """Cin = 4160: Cin / 64 = 65 > 64, so plan_args leaves the gather in its slow form (conv_tap per k tile), which no UNet shape
    takes.  3 x 3 pixels, K = 37440: the dispatcher's own choice (the 256 x 128 tile in 8 K-slices + splitk_reduce_kernel), the forced
    lock-step tiles, and 'Q', which has to fall back.  Reference, exact ``coded`` sums, and the tap test."""
    ops = _ops()
    B, H, W, Cin, Cout = G.SLOW_GATHER
    M, geo = _conv_geo(1, B, H, W, Cin)
    assert not G.conv_fast_gather(B, H, W, Cin, 1)
    for kind in G.CONV_KINDS:
        cx, cw, cb, cb2, cres = G.conv_inputs(1, H, W, Cin, Cout, kind, B)
        x, wt, bias, b2, res = (t.cuda() for t in (cx, cw, cb, cb2, cres))
        ref, bound = G.conv_reference(cx, cw, 1, cb, cb2[:, 8:8 + Cout], cres)
        for cfg in ("0", "K", "B", "C", "Q"):
            gemm.use(cfg)
            st, entries = G.plan_query(M, Cout, 9 * Cin, 1, gemm.force, gemm.tune, geo)
            assert st == 0 and entries[0][0].tile != "256"
            got = ops.conv3x3_nhwc(x, wt, bias=bias, bias2=b2[:, 8:8 + Cout], res=res, mode=1).cpu()
            gemm.scratch_untouched_behind(gemm.need(M, Cout, 9 * Cin, 1, geo), f"slow gather {cfg}")
            _measured("conv-slow-" + cfg, "mode1", kind, G.ratio_to_bound(got, ref, bound))
            if kind == "coded":
                assert G.same_bits(got, G.conv_restate(cx, cw, 1, cb, cb2[:, 8:8 + Cout], cres)), cfg
    x, wt = G.tap_inputs(B, H, W, Cin)
    want = G.tap_expected(x, 1)
    for cfg in ("0", "K"):
        gemm.use(cfg)
        assert G.same_bits(ops.conv3x3_nhwc(x.cuda(), wt.cuda(), mode=1).cpu(), want), cfg
