"""Not a test: what tests/test_norm_bound_host.py (CPU) and tests/test_gpu_norm_kernels.py (GPU) share about the row-wise kernels
rmsnorm_kernel, layernorm_kernel, softmax_rows_kernel (csrc/elementwise.hip), gn_stats_kernel / gn_apply_kernel and cfg_euler_kernel
(csrc/unet.hip): the case tables, the input kinds, the float64 references, the bounds, a plain fp32 CPU restatement of each kernel's
algorithm, and restatements with one deliberate error each.  Imports without a GPU.

Every reference is float64 on the bf16 input values, written from the definition, with an intermediate rounding only where named.
U = 2^-8 is the project's figure for one bf16 rounding.  Each bound is applied to every element, none excluded; where a bound is
zero the result must be exact.  The bounds are derived from the kernels' code, nothing is measured on a GPU:

RMSNorm     ref = w x r, r = (mean(x^2) + eps)^-1/2.                    |got - ref| <= 1.02 * 2U |ref|
            Two roundings, bf16(x r) and the product with w, both relative: no absolute term; an all-zero row gives zeros.
LayerNorm   t = (x - mu) r g, ref = t + b, biased variance.
            bound = 1.02 U |ref| + 2^-14 mean|x| r |g| + 2^-22 (|t| + |b|)
            2^-14: the fp32 row mean (the longest serial chain of adds is below 512); 2^-22: the final fma.
            With a residual: compare with res + ref, and add 1.02 U |res + ref|.
GroupNorm   per (batch row, group): n = HW cg, biased mu, var, r = (var + eps)^-1/2, m1 = mean|x|, m2 = mean x^2.
            t = (x - mu) r gamma, ref = t + beta.  L = ceil(rows / RG) + RG + cg from gn_geometry is the longest chain of fp32 adds
            in gn_stats_kernel (the chunk fold is in double), e = L 2^-24.
            bound = 1.02 U |ref| + e (m1 r |gamma| + 1/2 |t| m2 r^2) + 2^-22 (|x r gamma| + |beta - mu r gamma|)
            m2 r^2 is where the one-pass variance E[x^2] - mean^2 shows: it grows as (mu / sigma)^2.
            With SiLU (the kernel rounds to bf16 first): s = silu(ref), bound_s = 1.1 bound + 1.02 U |s| + 2^-120
            (|silu'| <= 1.1; the floor covers flush to zero).
Softmax     L = x scale (scale as its float32 value) or, with a bias, L = bf16(x scale + bias) for scale in {1, 0.5} (the product is
            then exact, so the sum is rounded once, as the kernel's fma rounds it).  ref = softmax(L).
            bound = 1.02 U ref (1 + 2^-12 |L - max L|) + 2^-120
CFG + Euler no bound, exact bits: ``euler_chain`` is the kernel's chain op by op in fp32 with ``.to(bfloat16)`` at every rounding
            point; ``euler_torch`` is the same update as plain bf16 torch ops in the order of oracle/unet_ref.py.

If a restatement goes over 1.0 on a listed case, the case or the derivation is wrong and is corrected in writing; no constant is
scaled until it fits, and nothing is fitted to a kernel's output.
"""
import functools
import math
from typing import NamedTuple

import torch

BF16 = torch.bfloat16
F32 = torch.float32
U = 2.0 ** -8
C1 = 1.02 * U
FLOOR = 2.0 ** -120


# ------------------------------------------------------------------------------------------------------------ helpers
def bits(t):
    """Integer view of the same bytes, so that NaN patterns compare."""
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


_NAN16 = torch.tensor([0x7FC0, 0x7F81, -1, -0x7F], dtype=torch.int16)                # quiet, signalling, all ones, negative


def nan_pattern(n):
    """n bf16 NaN bit patterns as int16."""
    return _NAN16[torch.arange(n) % len(_NAN16)].clone()


def ratio_to_bound(got, ref, bound):
    """max over every element of |got - ref| / bound; where the bound is zero the result must be exact.  A NaN or an infinity in
    the result is infinitely far over."""
    if not bool(torch.isfinite(got.float()).all()):
        return float("inf")
    err = (got.double() - ref).abs()
    one, zero = torch.ones_like(err), torch.zeros_like(err)
    return float(torch.where(bound > 0, err / torch.where(bound > 0, bound, one), torch.where(err > 0, one / zero, zero)).max())


def close_passes(got, want, rtol=2e-2):
    """The criterion of tests/test_gpu_ops.py (``close``): 1 % of the largest |want| plus 2 % of the value."""
    got, want = got.float(), want.float()
    atol = 1e-2 * float(want.abs().max().clamp_min(1e-6))
    return not bool(((got - want).abs() > atol + rtol * want.abs()).any())


def rel_l2_passes(got, want, tol=5e-3):
    """The criterion of test_groupnorm_nhwc (and of the softmax test): relative L2 below 5e-3."""
    got, want = got.double(), want.double()
    return not bool(torch.isnan(got).any()) and float((got - want).norm() / want.norm().clamp_min(1e-12)) < tol


def f32_value(v):
    return float(torch.tensor(v, dtype=F32))


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (k if isinstance(k, int) else sum(map(ord, k)))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _gain(n, g, scale=0.1):
    return (1 + scale * torch.randn(n, generator=g)).to(BF16)


def _thread_partials(v):
    """The row kernels' per-thread fp32 sums: v [rows, cols] -> [rows, 256]; thread t adds the 8 elements of the vectors t,
    t + 256, ... one after the other (the padding zeros add exactly nothing)."""
    rows, cols = v.shape
    trips = (cols // 8 + 255) // 256
    p = torch.zeros(rows, trips * 2048, dtype=F32)
    p[:, :cols] = v
    p = p.view(rows, trips, 256, 8)
    acc = torch.zeros(rows, 256, dtype=F32)
    for t in range(trips):
        for j in range(8):
            acc = acc + p[:, t, :, j]
    return acc


def _block_sum(p):
    """block_sum<4>: a tree inside each wave of 64, then the four waves one after the other."""
    w = p.view(p.shape[0], 4, 64)
    while w.shape[-1] > 1:
        w = w[..., 0::2] + w[..., 1::2]
    t = torch.zeros(p.shape[0], dtype=F32)
    for i in range(4):
        t = t + w[:, i, 0]
    return t[:, None]


# ------------------------------------------------------------------------------------------------------------ RMSNorm
RMS_COLS = (8, 248, 2048, 2056, 6656)           # one vector; below one trip; one trip of 256 threads x 8; one vector more; 3.25 trips
RMS_ROWS = (1, 3)
RMS_KINDS = ("rand", "outlier", "tiny", "zero_row")
RMS_EPS = 1e-6
RMS_MUTANTS = ("no_eps", "drop_last_vector")


@functools.lru_cache(maxsize=None)
def rms_inputs(rows, cols, kind):
    """x [rows, cols], w [cols], bf16 on the CPU.  rand: sigma 2; outlier: rand with 2^10 in the last column of each row; tiny:
    rand * 2^-12, so that eps = 1e-6 decides the result (mean x^2 = 2.4e-7); zero_row: rand with the middle row all zero."""
    assert kind in RMS_KINDS
    g = _gen("rms", rows, cols)
    x = (torch.randn(rows, cols, generator=g) * 2).to(BF16)
    w = _gain(cols, g)
    if kind == "outlier":
        x[:, -1] = 2.0 ** 10
    if kind == "tiny":
        x = (x.float() * 2.0 ** -12).to(BF16)                                # exact
    if kind == "zero_row":
        x[rows // 2] = 0
    return x, w


def rms_reference(x, w, eps=RMS_EPS):
    xd = x.double()
    r = (xd.pow(2).mean(-1, keepdim=True) + f32_value(eps)) ** -0.5
    ref = w.double() * xd * r
    return ref, 2 * C1 * ref.abs()


def rms_restate(x, w, eps=RMS_EPS, mutant=None):
    assert mutant in (None,) + RMS_MUTANTS
    xf = x.float()
    sq = xf * xf
    if mutant == "drop_last_vector":
        sq[:, -8:] = 0
    ss = _block_sum(_thread_partials(sq))
    e = torch.tensor(0.0 if mutant == "no_eps" else eps, dtype=F32)
    rinv = torch.rsqrt(ss / torch.tensor(float(x.shape[1]), dtype=F32) + e)
    return (w.float() * (xf * rinv).to(BF16).float()).to(BF16)


# ------------------------------------------------------------------------------------------------------------ LayerNorm
LN_COLS = (8, 256, 1792, 2056, 5120)
LN_ROWS = 5
LN_KINDS = ("rand", "offset", "flat")
LN_EPS = 1e-6
LN_MUTANTS = ("unbiased",)


@functools.lru_cache(maxsize=None)
def ln_inputs(cols, kind, rows=LN_ROWS):
    """x, w, b, res.  rand: sigma 2; offset: mean 32, sigma 0.5; flat: the constant 1.5 (the result is b within the absolute terms)."""
    assert kind in LN_KINDS
    g = _gen("ln", rows, cols)
    x = torch.randn(rows, cols, generator=g)
    x = {"rand": x * 2, "offset": 32 + 0.5 * x, "flat": torch.full_like(x, 1.5)}[kind].to(BF16)
    w = _gain(cols, g)
    b = (0.1 * torch.randn(cols, generator=g)).to(BF16)
    res = torch.randn(rows, cols, generator=g).to(BF16)
    return x, w, b, res


def ln_reference(x, w, b, res=None, eps=LN_EPS):
    xd, gd, bd = x.double(), w.double(), b.double()
    mu = xd.mean(-1, keepdim=True)
    r = ((xd - mu).pow(2).mean(-1, keepdim=True) + f32_value(eps)) ** -0.5
    t = (xd - mu) * r * gd
    ref = t + bd
    bound = C1 * ref.abs() + 2.0 ** -14 * xd.abs().mean(-1, keepdim=True) * r * gd.abs() + 2.0 ** -22 * (t.abs() + bd.abs())
    if res is not None:
        ref = res.double() + ref
        bound = bound + C1 * ref.abs()
    return ref, bound


def ln_restate(x, w, b, res=None, eps=LN_EPS, mutant=None):
    assert mutant in (None,) + LN_MUTANTS
    xf = x.float()
    n = torch.tensor(float(x.shape[1]), dtype=F32)
    mean = _block_sum(_thread_partials(xf)) / n
    d = xf - mean
    v = _block_sum(_thread_partials(d * d))
    rstd = torch.rsqrt(v / (n - 1 if mutant == "unbiased" else n) + torch.tensor(eps, dtype=F32))
    y = (d * rstd * w.float() + b.float()).to(BF16)
    if res is not None:
        y = (res.float() + y.float()).to(BF16)
    return y


# ------------------------------------------------------------------------------------------------------------ GroupNorm
class GNCase(NamedTuple):
    C: int
    G: int
    HW: int
    B: int


GN_EPS = 1e-5
GN_KINDS = ("rand", "coded", "flat")
GN_MUTANTS = ("ragged_rows_left_out", "group_of_32")
# (case, (cs, nv, RG, nchunk, rows), what it reaches)
GN_TABLE = [
    (GNCase(64, 32, 1, 2), (1, 8, 32, 1, 1), "one pixel, cg = 2"),
    (GNCase(320, 32, 1000, 2), (4, 10, 25, 3, 334), "idle row groups, ragged last chunk"),
    (GNCase(2560, 32, 16, 2), (4, 80, 3, 1, 16), "widest UNet activation"),
    (GNCase(2560, 5, 40, 2), (1, 320, 1, 3, 14), "wide branch, second 256-lane trip, G < 32"),
    (GNCase(2048, 1, 24, 1), (1, 256, 1, 2, 12), "wide branch at its edge, one group"),
    (GNCase(2040, 1, 24, 1), (1, 255, 1, 2, 12), "256 / nv == 1"),
    (GNCase(512, 8, 100, 3), (4, 16, 16, 1, 100), "2 groups per slice"),
    (GNCase(256, 2, 33, 2), (2, 16, 16, 1, 33), "2-way slice split"),
    (GNCase(2560, 5, 13200, 1), (1, 320, 1, 64, 207), "two trips of the 32-chunk fold"),
]
GN_CASES = [c for c, _, _ in GN_TABLE]
GN_BIG = GN_CASES[-1]                           # a 67 MB tensor: its reference is built on the GPU; the host file skips it alone


def gn_geometry(C, G, HW):
    """launch_groupnorm's planner restated -> (cs, nv, RG, nchunk, rows, cg): channel slices, 16-byte vectors per slice row, row
    groups side by side in a statistics workgroup, pixel chunks, pixel rows per chunk, channels per group."""
    cs = 4
    while cs > 1 and (G % cs or ((C // cs) & 7) or C // cs < 64):
        cs >>= 1
    nv = (C // cs) >> 3
    RG = 1 if nv >= 256 else 256 // nv
    unit = 16 * RG
    nchunk = (HW + unit - 1) // unit
    cap = 32
    while cap < 256 and HW * (C // cs) * 2 // cap > (2 << 20):
        cap <<= 1
    nchunk = min(nchunk, cap)
    rows = (HW + nchunk - 1) // nchunk
    nchunk = (HW + rows - 1) // rows
    return cs, nv, RG, nchunk, rows, C // G


def gn_group_means(c, device="cpu"):
    """The ``coded`` kind's mean per (batch row, group): 4 ((g + b) mod 5 - 2), so a mix-up of either index is an error of order one."""
    b, g = torch.arange(c.B, device=device)[:, None], torch.arange(c.G, device=device)[None, :]
    return (4 * ((g + b) % 5 - 2)).float()


def gn_inputs(c, kind, device="cpu"):
    """x [B, HW, C], gamma [C], beta [C], bf16 on ``device``.  rand: sigma 2, mean 0.5; coded: group g of batch row b has the mean
    of gn_group_means and sigma 0.5 (mu / sigma reaches 16); flat: that mean + 1.5, constant within each group."""
    assert kind in GN_KINDS
    g = torch.Generator(device=device).manual_seed(c.C * 10007 + c.G * 101 + c.HW * 7 + c.B)
    gamma = (1 + 0.1 * torch.randn(c.C, generator=g, device=device)).to(BF16)
    beta = (0.5 * torch.randn(c.C, generator=g, device=device)).to(BF16)
    x = torch.randn(c.B, c.HW, c.C, generator=g, device=device)
    m = gn_group_means(c, device)[:, None, :, None]
    xg = x.view(c.B, c.HW, c.G, c.C // c.G)
    if kind == "rand":
        x = x.mul_(2).add_(0.5)
    elif kind == "coded":
        x = xg.mul_(0.5).add_(m).view(c.B, c.HW, c.C)
    else:
        x = xg.zero_().add_(m + 1.5).view(c.B, c.HW, c.C)
    return x.to(BF16), gamma, beta


def gn_reference(x, gamma, beta, G, eps=GN_EPS):
    """(ref, bound, silu(ref), the bound with SiLU), float64 [B, HW, C] on x's device."""
    B, HW, C = x.shape
    cs, nv, RG, nchunk, rows, cg = gn_geometry(C, G, HW)
    e = ((rows + RG - 1) // RG + RG + cg) * 2.0 ** -24
    xd = x.double().view(B, HW, G, cg)
    gd, bd = gamma.double().view(1, 1, G, cg), beta.double().view(1, 1, G, cg)
    mu = xd.mean((1, 3), keepdim=True)
    r = ((xd - mu).pow(2).mean((1, 3), keepdim=True) + f32_value(eps)) ** -0.5
    m1, m2 = xd.abs().mean((1, 3), keepdim=True), xd.pow(2).mean((1, 3), keepdim=True)
    t = (xd - mu) * r * gd
    ref = t + bd
    bound = C1 * ref.abs() + e * (m1 * r * gd.abs() + 0.5 * t.abs() * m2 * r * r)
    del t
    bound += 2.0 ** -22 * ((xd * r * gd).abs() + (bd - mu * r * gd).abs())
    del xd
    s = ref * torch.sigmoid(ref)
    bound_s = 1.1 * bound + C1 * s.abs() + FLOOR
    return ref.view(B, HW, C), bound.view(B, HW, C), s.view(B, HW, C), bound_s.view(B, HW, C)


def gn_restate(x, gamma, beta, G, eps=GN_EPS, silu=False, mutant=None):
    """gn_stats_kernel + gn_apply_kernel in plain fp32 on the CPU.  Mutants: "ragged_rows_left_out" (the rows of the last chunk
    behind its last whole pass of RG rows never reach the sums); "group_of_32" (the apply pass takes a channel's group from
    cg = ceil(C / 32), the most groups there can be, instead of C / G; a statistics slot no group wrote reads as mean 0, rstd 1)."""
    assert mutant in (None,) + GN_MUTANTS
    B, HW, C = x.shape
    cs, nv, RG, nchunk, rows, cg = gn_geometry(C, G, HW)
    xf = x.float()
    K = (rows + RG - 1) // RG                                                # rows a thread walks one after the other
    xp = torch.zeros(B, nchunk, K * RG, C, dtype=F32)
    for ch in range(nchunk):
        r0, r1 = ch * rows, min(HW, ch * rows + rows)
        n = r1 - r0
        if mutant == "ragged_rows_left_out" and ch == nchunk - 1:
            n = n // RG * RG
        xp[:, ch, :n] = xf[:, r0:r0 + n]
    xp = xp.view(B, nchunk, K, RG, C)                                        # pixel row r0 + k RG + tr belongs to thread row tr
    s = torch.zeros(B, nchunk, RG, C, dtype=F32)
    q = torch.zeros(B, nchunk, RG, C, dtype=F32)
    for k in range(K):
        s = s + xp[:, :, k]
        q = q + xp[:, :, k] * xp[:, :, k]
    cs_, cq_ = torch.zeros(B, nchunk, C, dtype=F32), torch.zeros(B, nchunk, C, dtype=F32)
    for tr in range(RG):                                                     # the row groups meet in LDS, in order
        cs_ = cs_ + s[:, :, tr]
        cq_ = cq_ + q[:, :, tr]
    cs_, cq_ = cs_.view(B, nchunk, G, cg), cq_.view(B, nchunk, G, cg)
    ws_s, ws_q = torch.zeros(B, nchunk, G, dtype=F32), torch.zeros(B, nchunk, G, dtype=F32)
    for i in range(cg):                                                      # channels to groups, in order
        ws_s = ws_s + cs_[..., i]
        ws_q = ws_q + cq_[..., i]
    n = float(HW) * cg
    mean = ws_s.double().sum(1) / n                                          # the chunk fold is in double
    var = (ws_q.double().sum(1) / n - mean * mean).clamp_min(0.0)
    stat_m, stat_r = torch.zeros(B, 32, dtype=F32), torch.ones(B, 32, dtype=F32)
    stat_m[:, :G] = mean.float()
    stat_r[:, :G] = (1.0 / torch.sqrt(var + f32_value(eps))).float()
    gi = torch.arange(C) // ((C + 31) // 32 if mutant == "group_of_32" else cg)
    A = gamma.float()[None] * stat_r[:, gi]                                  # [B, C]
    Bv = beta.float()[None] - stat_m[:, gi] * A
    v = (xf * A[:, None] + Bv[:, None]).to(BF16)
    if silu:
        v = v.float()
        v = (v * torch.sigmoid(v)).to(BF16)
    return v


# ------------------------------------------------------------------------------------------------------------ softmax
SM_COLS = (8, 32, 2048, 2056, 4096)
SM_ROWS = (1, 7)
# scale per kind.  ``padded`` is this file's addition to the four kinds of the issue: see sm_inputs
SM_KINDS = {"rand": 0.37, "spike": 0.5, "uniform": 0.37, "bias": 1.0, "padded": 0.5}
SM_MUTANTS = ("max_of_first_2048", "bias_at_ld")
BF16_MIN = torch.finfo(BF16).min


@functools.lru_cache(maxsize=None)
def sm_inputs(rows, cols, kind):
    """x [rows, cols], bias [rows, cols] or None, scale.  rand: randn * 4, scale 0.37; spike: rand with one logit of exactly 60
    per row (x = 120, scale 0.5; in the last vector for row 0, three columns further left per row); uniform: equal logits; bias:
    randn x plus randn bias plus the causal mask of finfo(bf16).min as emu_amd/emu1.py builds it (``mem <= ctx``), here the last
    ``rows`` rows of the cols x cols mask, scale 1; padded: the same with the mask of left padding instead -- all but the last
    three columns masked -- because softmax does not depend on which maximum is subtracted until exp overflows: of all kinds
    only this one, with every one of the first 2048 columns masked, can tell a maximum taken over a part of the row."""
    assert kind in SM_KINDS
    g = _gen("softmax", rows, cols)
    x = torch.randn(rows, cols, generator=g)
    bias = None
    if kind in ("rand", "spike"):
        x = (x * 4).to(BF16)
        if kind == "spike":
            for r in range(rows):
                x[r, (cols - 1 - 3 * r) % cols] = 120.0
    elif kind == "uniform":
        x = torch.full_like(x, 3.0).to(BF16)
    else:
        x = x.to(BF16)
        rel = torch.randn(rows, cols, generator=g).to(BF16)
        mem, ctx = torch.arange(cols)[None, :], (torch.arange(rows) + (cols - rows))[:, None]
        seen = mem <= ctx if kind == "bias" else (mem >= cols - 3).expand(rows, cols)
        mask = torch.where(seen, 0.0, BF16_MIN).to(BF16)
        bias = rel + mask                                                    # a bf16 tensor add, as in emu1.py
        assert bool((bias[~seen] == BF16_MIN).all()) and bool(seen.any(-1).all())
    return x, bias, SM_KINDS[kind]


def sm_logits(x, bias, scale):
    if bias is None:
        return x.double() * f32_value(scale)
    assert scale in (1.0, 0.5)                                               # x * scale is exact: one rounding, fma or not
    return (x.float() * scale + bias.float()).to(BF16).double()


def sm_reference(x, bias, scale):
    L = sm_logits(x, bias, scale)
    mx = L.max(-1, keepdim=True).values
    ref = torch.softmax(L, -1)
    return ref, C1 * ref * (1 + 2.0 ** -12 * (L - mx).abs()) + FLOOR


def sm_restate(xbuf, rows, cols, ld, scale, biasbuf=None, ld_bias=0, mutant=None):
    """softmax_rows_kernel on flat buffers (row r of x starts at r * ld, of the bias at r * ld_bias) -> bf16 [rows, cols]."""
    assert mutant in (None,) + SM_MUTANTS
    row = lambda buf, l: torch.stack([buf[r * l:r * l + cols] for r in range(rows)]).float()
    f = row(xbuf, ld)
    sc = torch.tensor(scale, dtype=F32)
    if biasbuf is not None:
        f = (f * sc + row(biasbuf, ld if mutant == "bias_at_ld" else ld_bias)).to(BF16).float()
    else:
        f = f * sc
    m = (f[:, :2048] if mutant == "max_of_first_2048" else f).max(-1, keepdim=True).values
    p = torch.exp(f - m)
    l = _block_sum(_thread_partials(p))
    return (p * (1.0 / l)).to(BF16)


# ------------------------------------------------------------------------------------------------------------ CFG + Euler
EULER_MAPS = ((5, 7), (16, 17))                 # 140 elements: one partial workgroup; 1088: four full ones and a quarter
EULER_STEPS_N = 6
EULER_STEPS = (0, EULER_STEPS_N - 2, EULER_STEPS_N - 1)                      # the last one goes to sigma 0
EULER_GUIDANCE = (1.0, 3.0, 7.5)
EULER_C = 4


@functools.lru_cache(maxsize=None)
def euler_inputs(H, W, step):
    """eps_pair [2 HW, C] (NHWC rows, cond first), latents [1, C, H, W]; the latents at the scale of the step's sigma."""
    g = _gen("euler", H, W, step)
    sig = float(euler_sigmas()[step])
    eps = torch.randn(2 * H * W, EULER_C, generator=g).to(BF16)
    lat = (torch.randn(1, EULER_C, H, W, generator=g) * math.sqrt(sig * sig + 1)).to(BF16)
    return eps, lat


@functools.lru_cache(maxsize=None)
def euler_sigmas(n=EULER_STEPS_N):
    from emu_amd.unet import EulerDiscreteSchedule
    return EulerDiscreteSchedule().set_timesteps(n).sigmas.clone()


def euler_chain(eps, lat, sigmas, step, guidance):
    """cfg_euler_kernel op by op: fp32 arithmetic, ``.to(bfloat16)`` wherever the kernel rounds."""
    rb = lambda t: t.to(BF16).float()
    _, C, H, W = lat.shape
    HW = H * W
    sigma, dt = sigmas[step], sigmas[step + 1] - sigmas[step]               # fp32, as the kernel forms them
    ec, eu = eps[:HW].float(), eps[HW:].float()                              # cond first
    e = rb(eu + rb(torch.tensor(guidance, dtype=F32) * rb(ec - eu)))
    e = e.t().reshape(1, C, H, W)                                            # NHWC rows -> the latents' NCHW
    x = lat.float()
    x0 = rb(x - rb(sigma * e))
    der = rb(rb(x - x0) / sigma)
    return (x + rb(der * dt)).to(BF16)


def euler_torch(eps, lat, sigmas, step, guidance):
    """The same update as plain bf16 torch ops in the order of oracle/unet_ref.py: ``e_u + g (e_c - e_u)``, then
    EulerSchedule.step itself with Python-float sigmas."""
    from oracle import unet_ref as R
    _, C, H, W = lat.shape
    e_c, e_u = eps.view(2, H, W, C).permute(0, 3, 1, 2).chunk(2)
    e = e_u + guidance * (e_c - e_u)
    sch = R.EulerSchedule()
    sch.sigmas = [float(s) for s in sigmas]
    out = sch.step(e, step, lat)
    assert out.dtype == BF16
    return out
