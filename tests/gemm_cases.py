"""Not a test: what tests/test_gemm_bound_host.py (CPU) and tests/test_gpu_gemm_kernels.py (GPU) share about the tiled bf16 GEMM
(csrc/gemm.hip: the lock-step 128 x 128 / 256 x 128 / 128 x 64 tiles; csrc/gemm256.hip and csrc/gemm_w4.hip: the eight- and
four-wave 256 x 256 tiles) and the epilogues and 3 x 3 implicit-GEMM gather of csrc/gemm_tile.h: the case tables with the plan
every case was confirmed with, the input kinds, the float64 references, the bounds, a plain fp32 CPU restatement, and restatements
with one deliberate error each.  Imports without a GPU.

References.  Float64 on the bf16 input values, written from the definition: acc = sum_k a_k w_k, y = acc + bias, then + bias2,
then the epilogue -- y + res; silu(y); gelu(y) (erf); silu(y[2j]) y[2j+1] (SwiGLU); y[2j] gelu(y[2j+1]) (GEGLU).  The reference
itself is not rounded anywhere; every rounding gemm_tile.h::quad_value names -- bf16(acc + bias), bf16(y + bias2), bf16(y + res),
bf16(act(y)), bf16(bf16(silu(y[2j])) y[2j+1]), bf16(y[2j] bf16(gelu(y[2j+1]))) -- is a term of the bound.  ``gemm_exact`` applies
those roundings to the exact sums of the ``coded`` kind, where every fp32 sum is exact, and gives the bits the kernel must store.

Bounds (U = 2^-8, C1 = 1.02 U, FLOOR = 2^-120 from tests/norm_cases.py), applied to every element, none excluded; derived from the
code, nothing is measured on a GPU and no constant is fitted to a kernel's output:

plain       bound_y = C1 |y| + e_acc + FLOOR,  e_acc = (K + 2) 2^-23 (sum_k |a_k w_k| + |bias|).
            Every product of two bf16 values is exact in fp32.  A sum of K products (+ the bias) in ANY order, K-slices and the
            two k-groups of the 128 x 64 tile included, is off by at most (K + 1) u (sum |a w| + |bias|) to first order, u the
            unit of one fp32 add.  u = 2^-24 for round to nearest; 2^-23 is taken because the rounding of the bf16 matrix core's
            internal adds is not documented: it covers truncation too.  K + 2 for K + 1 covers the second-order terms
            ((1 + 2^-23)^1100 - 1 < 1.0001 * 1100 * 2^-23).  Derived, not measured.  e_acc is computed per element from the
            float64 sum of |a w|; at K <= 1100 it is at most 1102 * 2^-23 = 0.034 U of that sum, so the bound remains a
            rounding-level one wherever the sum does not cancel (where it does, as in the ``offset`` kind, e_acc is the term
            that says how far a correct kernel may be off).  The slow-gather conv (K = 37440) has e_acc = 1.14 U of the sum.
bias2       v = y + bias2: bound_v = bound_y + C1 |v|   (one more rounding of the value rounded)
RESID       v = y + res:   bound_v = bound_y + C1 |v|
SILU, GELU  s = act(y):    bound_s = L bound_y + C1 |s| + FLOOR,  L = 1.1 (max |silu'| = 1.0998), 1.13 (max |gelu'| = 1.129)
SWIGLU      g = silu(y[2j]) with bound_g as for SILU, u = y[2j+1] with bound_u = bound_y:
            p = g u, bound_p = |g| bound_u + |u| bound_g + bound_g bound_u + C1 |p| + FLOOR   (product rule, cross term included)
GEGLU       the same with h = y[2j] and g = gelu(y[2j+1]).

``resid_rounded_once`` (bf16(acc + bias + res), one rounding instead of two) is not among the mutants: it has less error than the
kernel, and the bound allows two roundings, so no case can catch it.

Restatement (``gemm_restate``).  fp32 on the CPU: k tiles of 64 accumulated one after the other (the 128 x 64 tile: its two
k-groups take elements 0..31 and 32..63 of every k tile and are added at the end, gemm.hip ``KSTEPS``), K-slice s takes the k tiles
[s nk / ks, (s + 1) nk / ks) and the slices are summed in slice order from zero (splitk_reduce_kernel, pp_reduce_kernel), then the
epilogue chain with ``.to(bfloat16)`` at every rounding point.

Input kinds.  rand: x sigma 1, w sigma 0.05, bias and res sigma 1.  offset: x mean 4, so that |acc| is a small difference of large
sums: accumulation error and cancellation show.  coded: exact small integers -- even rows of x are rows of I (a single 1 at column
5 m mod K), odd rows are (m + 3 k) mod 5 - 2; w is (i * 7) % 251 - 125 over the flat index i; bias and res are integers below 64
in magnitude.  |acc| < 1100 * 2 * 125 < 2^24, so every fp32 sum is exact in any order.

Tiles (rows x columns): B 128 x 128, C 128 x 256, K 64 x 128 (two k-groups), S = C with forced K-slices, Q the 256 x 256 tile
unsliced, P the same with the planned K-slices, W = P with emu_gemm_tune bit 22 (the four-wave kernel wherever it exists).

What the planner (emu_gemm_plan, on the CPU) says; tests/test_gemm_bound_host.py asserts each of these:
  GEMM_REDUCE_SPLITK   force 'S': from K = 1024 on (16 k tiles: two slices of 8, pick_ksplit's forced minimum), at any M, N with
                       N % 4 == 0 and a non-GLU epilogue; K = 960 is unsliced.  Found with M = 63, N = 4 (tile C, ksplit 2,
                       reduce 1).  Unforced it needs 24 k tiles per slice (K >= 3072, above the cap); the slow-gather conv
                       (K = 37440) reaches it unforced with 8 slices.
  GEMM_REDUCE_PP       force 'P': from K = 1024 on (plan_pp: 8 k tiles per slice and a cost model that takes two slices for one
                       tile there), any M, N % 4 == 0, GLU epilogues included.  M = 63, N = 4: tile 256, ksplit 2, reduce 2.
  four-wave + slices   the same shapes under tune bit 22: w4 = 1, ksplit 2, reduce 2.
  unequal K-slices     K = 1088: 17 k tiles in slices of 8 and 9.
  hybrid split 'H'     cannot be reached below the cap: plan_hybrid needs at least one whole round of 256 tiles of 256 x 256 and a
                       remainder, i.e. more than 256 tiles (M N > 16.7 M) and K >= 512.  The smallest by M N: one tile row needs
                       N > 65536 (192 x 65544, 12.6 M outputs), two rows M >= 273 (257..272 fold into one row) and N > 32768:
                       273 x 32776 x 512 (8.9 M) -- three rows 529 x 21768 (11.5 M), four 785 x 16392 (12.9 M).  Plan: 256 tile
                       on columns [0, 32768), then tile K on the last 8.  K = 448 does not split.  Unforced dispatch takes it too.
  slow conv gather     Cin = 4160 (Cin / 64 = 65 > 64): plan_args leaves cpt_magic 0; visible in the plan as force 'Q' falling
                       back to a lock-step tile (gemm256_ok refuses the slow form), while Cin = 4096 takes the 256 tile.
The remainder rows the 256 x 256 tile folds into its last tile row are M % 256 in 1..16 (pp_tiles_m), not 32: M = 257 and 272 fold,
273, 288 and 289 open a second tile row; all five are in the table.
"""
import ctypes as C
import functools
from typing import NamedTuple

import torch

from tests.norm_cases import BF16, C1, F32, FLOOR, U, bits, close_passes, nan_pattern, ratio_to_bound, same_bits  # noqa: F401

EPI_NONE, EPI_RESID, EPI_SWIGLU, EPI_SILU, EPI_GELU, EPI_GEGLU = range(6)
EPI_NAMES = ("none", "resid", "swiglu", "silu", "gelu", "geglu")
GLU = (EPI_SWIGLU, EPI_GEGLU)
KINDS = ("rand", "offset", "coded")
MUTANTS = ("truncating_store", "bias_after_rounding", "ragged_k_chunk_dropped", "glu_halves")
CONV_MUTANTS = ("s2_last_tap_inside", "up2_parity_swapped")
SCRATCH_FLOATS = 32 * 288 * 256             # the split-K scratch the GPU file registers and the host file plans with
REDUCE_NONE, REDUCE_SPLITK, REDUCE_PP = 0, 1, 2
TUNE_W4, TUNE_DIRECT = 1 << 22, 8
# config -> (force letter, tune, tile rows, tile columns, k-groups)
CONFIGS = {"B": ("B", 0, 128, 128, 1), "C": ("C", 0, 128, 256, 1), "K": ("K", 0, 64, 128, 2), "S": ("S", 0, 128, 256, 1),
           "P": ("P", 0, 256, 256, 1), "Q": ("Q", 0, 256, 256, 1), "W": ("P", TUNE_W4, 256, 256, 1)}
LOCKSTEP = ("B", "C", "K")


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (k if isinstance(k, int) else sum(map(ord, k)))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def rb(t):
    """fp32 -> bf16 -> fp32: one rounding point."""
    return t.to(BF16).float()


def trunc_bf16(t):
    """fp32 -> bf16 by dropping the low 16 bits (the ``truncating_store`` mutant)."""
    return (t.contiguous().view(torch.int32) & -65536).view(F32).to(BF16)


# ------------------------------------------------------------------------------------------------------------ plans
class Plan(NamedTuple):
    tile: str           # 'B', 'C', 'K' or '256'
    ksplit: int
    reduce: int
    w4: int
    stage: int


def plan_query(M, N, K, epi=0, force="0", tune=0, conv=(0, 0, 0, 0, 0, 0), scratch=SCRATCH_FLOATS):
    """emu_gemm_plan on the CPU -> (status, [(Plan, full_tiles, col0, n), ...]).  conv = (mode, Hin, Win, Hout, Wout, Cin)."""
    from emu_amd import _lib
    from tests.test_gemm_plan import PlanC, ShapeC
    out, n = (PlanC * 2)(), C.c_int(0)
    st = _lib.lib().emu_gemm_plan(C.byref(ShapeC(M, N, K, epi, *conv, 0, 0, 0, 0, scratch)), 0 if force == "0" else ord(force), tune,
                                  out, C.byref(n))
    return st, [(Plan("256" if p.tile == 256 else chr(p.tile), p.ksplit, p.reduce, p.w4, p.stage), p.full_tiles, p.col0, p.n)
                for p in out[:n.value]]


def plan_epi(N, epi):
    """The epilogue to ask emu_gemm_plan about: the hook lays C out contiguously, and a contiguous C of odd width (N % 4 == 2
    under a GLU) is refused, so such a case is asked without its epilogue -- a forced config's tile does not depend on it, and
    N % 4 != 0 is never sliced."""
    return EPI_NONE if epi in GLU and (N // 2) % 2 else epi


def scratch_need(plan, full_tiles, M, N, conv=False):
    """fp32 elements of the split-K scratch a planned launch writes: slices of its tail tiles, back to back from the start.  (A
    conv never folds remainder rows into the last row of 256 x 256 tiles.)"""
    if plan.ksplit < 2:
        return 0
    if plan.tile == "256":
        r = M & 255
        tm = M >> 8 if not conv and (M >> 8) >= 1 and 0 < r <= 16 else (M + 255) >> 8
        return (tm * ((N + 255) // 256) - full_tiles) * plan.ksplit * 288 * 256
    return (((M + 127) // 128) * ((N + 255) // 256) - full_tiles) * plan.ksplit * 256 * 128


# ------------------------------------------------------------------------------------------------------------ case tables
class Case(NamedTuple):
    cfg: str
    M: int
    N: int
    K: int
    epis: tuple
    pad: int            # C is a column slice of a buffer pad columns wider (ldc = columns + pad)
    plan: Plan          # of the contiguous launch with the first epilogue, from emu_gemm_plan (see plan_epi)
    why: str


ALL_EPIS = (EPI_NONE, EPI_RESID, EPI_SWIGLU, EPI_SILU, EPI_GELU, EPI_GEGLU)


def _edge_shapes(cfg):
    """(M, N, K, epilogues, pad, why) of one config: the tile edges listed in the module docstring of tests/test_gpu_gemm_kernels.py."""
    _, _, bm, bn, _ = CONFIGS[cfg]
    lock = cfg in LOCKSTEP
    kr = 72 if lock else 64                                                  # a ragged K where the tile takes one
    glu = EPI_SWIGLU if cfg in ("B", "K", "P") else EPI_GEGLU
    out = []
    ms = [bm - 1, bm, bm + 1] + ([272, 273, 288, 289] if bm == 256 else [])
    for m in ms:
        out.append((m, bn + 3, kr, (EPI_NONE, EPI_RESID), 8, f"M = {m}; N % 4 == 3: scalar path of store_quad, one tile and a part"))
        out.append((m, bn + 6, kr, (glu,), 9, f"M = {m}; N % 4 == 2 under a GLU: N / 2 is odd, so C has to be a slice with an even ldc"))
    m = bm + 1
    out.append((m, bn + 64, 192, ALL_EPIS, 8, "every epilogue; three k tiles; a staged tile column and a direct one"))
    out.append((m, bn + 64, 192, (EPI_NONE, EPI_RESID), 5, "ldc % 4 != 0: scalar stores"))
    out.append((m, bn + 64, 192, (glu,), 6, "GLU, ldc % 4 == 2"))
    ks = (8, 64, 72, 200) if lock else (64, 128)
    for k in ks:
        out.append((m, bn + 8, k, (EPI_NONE, EPI_RESID, glu), 8, f"K = {k}: fewer k tiles than the ring is deep"
                    + ("; ragged" if k % 64 else "")))
    if cfg in ("S", "P", "W"):
        for k, why in ((960, "the longest K that is not sliced"), (1024, "the shortest K that is sliced: two slices of 8 k tiles"),
                       (1088, "17 k tiles: slices of 8 and 9")):
            out.append((m, bn + 8, k, (EPI_NONE, EPI_RESID), 8, why))
            if cfg != "S":
                out.append((m, bn + 16, k, (glu,), 8, why + "; GLU through the slice reduce"))
        out.append((63, 4, 1024, (EPI_NONE,), 8, "the smallest sliced problem found"))
    return out


# recorded from emu_gemm_plan (tile, ksplit, reduce, w4, stage); tests/test_gemm_bound_host.py asserts the planner returns them
_PLANS = {
    "B": Plan("B", 1, 0, 0, 0), "C": Plan("C", 1, 0, 0, 0), "K": Plan("K", 1, 0, 0, 0), "S": Plan("C", 1, 0, 0, 0),
    "P": Plan("256", 1, 0, 0, 2), "Q": Plan("256", 1, 0, 0, 2), "W": Plan("256", 1, 0, 1, 2),
}


def _recorded_plan(cfg, M, N, K, epi):
    """The planner's rules for these tables, restated: stage bit 0 = the staged epilogue (N % 8 == 0, GLU: N % 16 == 0), bit 1 = the
    256 tile's slices through LDS; K-slices from 16 k tiles on for S (non-GLU, N % 4 == 0) and P / W (N % 4 == 0)."""
    p = _PLANS[cfg]
    stage = p.stage | int(N % (16 if epi in GLU else 8) == 0)
    sliced = K >= 1024 and K % 64 == 0 and N % 4 == 0 and (cfg in ("P", "W") or (cfg == "S" and epi not in GLU))
    if sliced:
        return Plan(p.tile, 2, REDUCE_SPLITK if cfg == "S" else REDUCE_PP, p.w4, stage)
    return Plan(p.tile, 1, 0, p.w4, stage)


CASES = [Case(cfg, M, N, K, epis, pad, _recorded_plan(cfg, M, N, K, epis[0]), why)
         for cfg in CONFIGS for (M, N, K, epis, pad, why) in _edge_shapes(cfg)]
# the literal record of what the sliced forms plan (the rest of the table follows _recorded_plan's two rules)
SLICED_PLANS = {
    ("S", 63, 4, 1024): Plan("C", 2, 1, 0, 0), ("P", 63, 4, 1024): Plan("256", 2, 2, 0, 2), ("W", 63, 4, 1024): Plan("256", 2, 2, 1, 2),
    ("S", 129, 264, 1024): Plan("C", 2, 1, 0, 1), ("P", 257, 264, 1088): Plan("256", 2, 2, 0, 3), ("W", 257, 272, 1024): Plan("256", 2, 2, 1, 3),
    ("S", 129, 264, 960): Plan("C", 1, 0, 0, 1), ("P", 257, 264, 960): Plan("256", 1, 0, 0, 3), ("W", 257, 264, 960): Plan("256", 1, 0, 1, 3),
}
HYBRID = (273, 32776, 512)                       # M, N, K: the smallest problem found that takes the hybrid split
HYBRID_PLAN = [(Plan("256", 1, 0, 1, 3), 256, 0, 32768), (Plan("K", 1, 0, 0, 1), 5, 32768, 8)]       # (plan, full tiles, col0, n)
HYBRID_TOO_SMALL = ((273, 32520, 512), (192, 65288, 512), (273, 32776, 448))


# ------------------------------------------------------------------------------------------------------------ GEMM inputs
@functools.lru_cache(maxsize=64)
def gemm_inputs(M, N, K, kind):
    """x [M, K], w [N, K], bias [N], res [M, N]: bf16 on the CPU."""
    assert kind in KINDS
    g = _gen("gemm", M, N, K)
    if kind == "coded":
        m, k = torch.arange(M)[:, None], torch.arange(K)[None, :]
        x = ((m + 3 * k) % 5 - 2).float()
        eye = ((5 * m) % K == k).float()
        x = torch.where(m % 2 == 0, eye, x).to(BF16)
        w = ((torch.arange(N * K) * 7) % 251 - 125).float().view(N, K).to(BF16)
        bias = (torch.arange(N) % 127 - 63).float().to(BF16)
        res = ((torch.arange(M * N) * 11) % 125 - 62).float().view(M, N).to(BF16)
        return x, w, bias, res
    x = torch.randn(M, K, generator=g)
    if kind == "offset":
        x = x + 4
    w = torch.randn(N, K, generator=g) * 0.05
    return x.to(BF16), w.to(BF16), torch.randn(N, generator=g).to(BF16), torch.randn(M, N, generator=g).to(BF16)


def acc64(x, w):
    """(sum_k x w, sum_k |x w|) in float64, on the operands' device."""
    xd, wd = x.double(), w.double()
    return xd @ wd.t(), xd.abs() @ wd.abs().t()


def _silu64(y):
    return y * torch.sigmoid(y)


def _gelu64(y):
    return 0.5 * y * (1 + torch.erf(y * 0.5 ** 0.5))


def epilogue64(acc, mag, K, epi, bias=None, bias2=None, res=None):
    """(reference, bound) of the epilogue chain from the float64 sums.  bias [N], bias2 and res broadcastable to acc."""
    b = 0 if bias is None else bias.double()
    y = acc + b
    by = C1 * y.abs() + (K + 2) * 2.0 ** -23 * (mag + (0 if bias is None else bias.double().abs())) + FLOOR
    if bias2 is not None:
        y = y + bias2.double()
        by = by + C1 * y.abs()
    if epi == EPI_NONE:
        return y, by
    if epi == EPI_RESID:
        v = y + res.double()
        return v, by + C1 * v.abs()
    if epi == EPI_SILU:
        s = _silu64(y)
        return s, 1.1 * by + C1 * s.abs() + FLOOR
    if epi == EPI_GELU:
        s = _gelu64(y)
        return s, 1.13 * by + C1 * s.abs() + FLOOR
    y0, y1, b0, b1 = y[..., 0::2], y[..., 1::2], by[..., 0::2], by[..., 1::2]
    if epi == EPI_SWIGLU:
        g, bg, u, bu = _silu64(y0), None, y1, b1
        bg = 1.1 * b0 + C1 * g.abs() + FLOOR
    else:
        g, u, bu = _gelu64(y1), y0, b0
        bg = 1.13 * b1 + C1 * g.abs() + FLOOR
    p = g * u
    return p, g.abs() * bu + u.abs() * bg + bg * bu + C1 * p.abs() + FLOOR


@functools.lru_cache(maxsize=8)
def _gemm_sums(M, N, K, kind):
    x, w, _, _ = gemm_inputs(M, N, K, kind)
    return acc64(x, w)


def gemm_reference(M, N, K, kind, epi):
    """(ref, bound) float64 [M, N] (GLU: [M, N / 2]) of ops.linear(x, w, bias, res, epi) on gemm_inputs; the bias goes with every
    epilogue, the residual with RESID."""
    _, _, bias, res = gemm_inputs(M, N, K, kind)
    acc, mag = _gemm_sums(M, N, K, kind)
    return epilogue64(acc, mag, K, epi, bias=bias, res=res)


def epilogue_chain(acc, epi, bias=None, bias2=None, res=None, mutant=None):
    """The kernel's epilogue on fp32 sums: ``.to(bfloat16)`` wherever quad_value rounds.  bf16 [M, N] (GLU: [M, N / 2])."""
    store = trunc_bf16 if mutant == "truncating_store" else (lambda t: t.to(BF16))
    pre = rb(acc) if mutant == "bias_after_rounding" else acc                # the fp32 value ahead of the next rounding
    if bias is not None:
        pre = pre + bias.float()
    if bias2 is not None:
        pre = rb(pre) + bias2.float()
    if epi == EPI_NONE:
        return store(pre)
    y = rb(pre)
    if epi == EPI_RESID:
        return store(y + res.float())
    if epi == EPI_SILU:
        return store(y * torch.sigmoid(y))
    if epi == EPI_GELU:
        return store(torch.nn.functional.gelu(y))
    n = y.shape[-1]
    y0, y1 = (y[..., :n // 2], y[..., n // 2:]) if mutant == "glu_halves" else (y[..., 0::2], y[..., 1::2])
    if epi == EPI_SWIGLU:
        return store(rb(y0 * torch.sigmoid(y0)) * y1)
    return store(y0 * rb(torch.nn.functional.gelu(y1)))


def accumulate32(x, w, kgroups=1, ksplit=1, mutant=None):
    """sum_k x w in fp32 in the tiles' order: see the module docstring."""
    xf, wf = x.float(), w.float()
    M, K = xf.shape
    if mutant == "ragged_k_chunk_dropped" and K % 64:
        xf = xf.clone()
        xf[:, K - 8:] = 0
    nk = (K + 63) // 64
    total = torch.zeros(M, wf.shape[0], dtype=F32)
    for s in range(ksplit):
        groups = [torch.zeros_like(total) for _ in range(kgroups)]
        for t in range(s * nk // ksplit, (s + 1) * nk // ksplit):
            for g in range(kgroups):
                w_ = 64 // kgroups
                lo, hi = t * 64 + g * w_, min(K, t * 64 + (g + 1) * w_)
                if lo < hi:
                    groups[g] = groups[g] + xf[:, lo:hi] @ wf[:, lo:hi].t()
        part = groups[0]
        for g in groups[1:]:
            part = part + g
        total = part if ksplit == 1 else total + part
    return total


def gemm_restate(M, N, K, kind, epi, cfg, ksplit=1, mutant=None):
    x, w, bias, res = gemm_inputs(M, N, K, kind)
    acc = accumulate32(x, w, CONFIGS[cfg][4], ksplit, mutant)
    return epilogue_chain(acc, epi, bias=bias, res=res, mutant=mutant)


def gemm_exact(M, N, K, epi):
    """The bits of the ``coded`` kind under NONE / RESID: its sums are exact integers below 2^24, so the epilogue roundings of the
    exact values are what every correct kernel stores."""
    assert epi in (EPI_NONE, EPI_RESID)
    _, _, bias, res = gemm_inputs(M, N, K, "coded")
    acc, mag = _gemm_sums(M, N, K, "coded")
    assert float(mag.max()) < 2 ** 24 - 64
    return epilogue_chain(acc.float(), epi, bias=bias, res=res)


# ------------------------------------------------------------------------------------------------------------ conv
CONV_MODES = (1, 2, 3)                           # 3 x 3, 3 x 3 stride 2, nearest x2 upsample + 3 x 3
CONV_IMAGES = ((5, 8), (7, 4), (1, 9), (9, 1))
CONV_CH = ((64, 4), (64, 36), (64, 130), (128, 4), (128, 36), (128, 130))        # (Cin, Cout)
CONV_B = 3
CONV_CFGS = ("0", "B", "C", "K", "P", "Q", "W")  # "0": the dispatcher's own choice (the 128 x 64 tile at these sizes)
CONV_KINDS = ("rand", "coded")
SLOW_GATHER = (1, 3, 3, 4160, 8)                 # B, H, W, Cin, Cout: K = 37440; Cin / 64 = 65 > 64 switches the fast gather off
TAP_CHANNELS = 4


def conv_out_hw(mode, H, W):
    return (H, W) if mode == 1 else ((H + 1) // 2, (W + 1) // 2) if mode == 2 else (2 * H, 2 * W)


def conv_fast_gather(B, H, W, Cin, mode):
    """plan_args' rule for ConvGeom::cpt_magic, restated."""
    cpt, src = Cin // 64, B * H * W
    return cpt <= 64 and src < ((1 << 21) if mode == 3 else (1 << 23)) and src * Cin * 2 < (1 << 31)


def conv_tap(mode, H, W, py, px, ky, kx):
    """gemm_tile.h::conv_tap on integer tensors -> (inside, yi, xi)."""
    if mode == 2:
        yi, xi = 2 * py + ky - 1, 2 * px + kx - 1
        return (yi >= 0) & (yi < H) & (xi >= 0) & (xi < W), yi, xi
    if mode == 3:
        yu, xu = py + ky - 1, px + kx - 1
        return (yu >= 0) & (yu < 2 * H) & (xu >= 0) & (xu < 2 * W), yu >> 1, xu >> 1
    yi, xi = py + ky - 1, px + kx - 1
    return (yi >= 0) & (yi < H) & (xi >= 0) & (xi < W), yi, xi


def conv_gather(x, mode, mutant=None):
    """The implicit GEMM's A matrix: x [B, H, W, Cin] -> [B Ho Wo, 9 Cin], column (3 ky + kx) Cin + c, zeros outside the image.
    Mutants: "s2_last_tap_inside" (stride 2: the tap one past the bottom / right edge of an odd side is read from the memory that
    follows instead of zeroed); "up2_parity_swapped" (upsampled: the source step of a tap takes py's parity for dx and px's for dy)."""
    assert mutant in (None,) + CONV_MUTANTS
    B, H, W, Cin = x.shape
    Ho, Wo = conv_out_hw(mode, H, W)
    py, px = torch.arange(Ho)[:, None].expand(Ho, Wo), torch.arange(Wo)[None, :].expand(Ho, Wo)
    flat = x.reshape(B * H * W, Cin)
    cols = []
    for ky in range(3):
        for kx in range(3):
            ok, yi, xi = conv_tap(mode, H, W, py, px, ky, kx)
            if mutant == "s2_last_tap_inside" and mode == 2:
                ok = (yi >= 0) & (yi <= H) & (xi >= 0) & (xi <= W)
            if mutant == "up2_parity_swapped" and mode == 3:
                yi = (py >> 1) + (((px & 1) + ky - 1) >> 1)
                xi = (px >> 1) + (((py & 1) + kx - 1) >> 1)
            idx = (torch.arange(B)[:, None, None] * H + yi[None]) * W + xi[None]                 # [B, Ho, Wo]
            v = flat[idx.clamp(0, B * H * W - 1).reshape(-1)]
            cols.append(torch.where(ok[None].expand(B, Ho, Wo).reshape(-1, 1), v, torch.zeros_like(v)))
    return torch.cat(cols, 1)


@functools.lru_cache(maxsize=16)
def conv_inputs(mode, H, W, Cin, Cout, kind, B=CONV_B):
    """x [B, H, W, Cin], w [Cout, 3, 3, Cin], bias [Cout], the bias2 table [B, Cout + 24] whose columns [8, 8 + Cout) are the
    per-batch bias, res [B, Ho, Wo, Cout]: bf16 on the CPU.  coded: small integers, every fp32 sum exact."""
    assert kind in CONV_KINDS
    g = _gen("conv", mode, H, W, Cin, Cout)
    Ho, Wo = conv_out_hw(mode, H, W)
    if kind == "coded":
        x = ((torch.arange(B * H * W * Cin) * 3) % 7 - 3).float().view(B, H, W, Cin)
        w = ((torch.arange(Cout * 9 * Cin) * 7) % 251 - 125).float().view(Cout, 3, 3, Cin)
        bias = (torch.arange(Cout) % 127 - 63).float()
        b2 = ((torch.arange(B * (Cout + 24)) * 5) % 31 - 15).float().view(B, Cout + 24)
        res = ((torch.arange(B * Ho * Wo * Cout) * 11) % 125 - 62).float().view(B, Ho, Wo, Cout)
    else:
        x = torch.randn(B, H, W, Cin, generator=g)
        w = torch.randn(Cout, 3, 3, Cin, generator=g) * 0.05
        bias, b2 = torch.randn(Cout, generator=g), torch.randn(B, Cout + 24, generator=g)
        res = torch.randn(B, Ho, Wo, Cout, generator=g)
    return x.to(BF16), w.to(BF16), bias.to(BF16), b2.to(BF16), res.to(BF16)


def _conv_rows(t, B, Ho, Wo):
    """A per-batch [B, Cout] operand as rows of the implicit GEMM."""
    return t[:, None, :].expand(B, Ho * Wo, t.shape[-1]).reshape(B * Ho * Wo, -1)


def conv_reference(x, w, mode, bias=None, bias2=None, res=None):
    """(ref, bound) float64 [B, Ho, Wo, Cout] of ops.conv3x3_nhwc: the gather of conv_tap, then the GEMM's reference."""
    B, H, W, Cin = x.shape
    Ho, Wo = conv_out_hw(mode, H, W)
    acc, mag = acc64(conv_gather(x, mode), w.reshape(w.shape[0], -1))
    ref, bound = epilogue64(acc, mag, 9 * Cin, EPI_RESID if res is not None else EPI_NONE, bias=bias,
                            bias2=None if bias2 is None else _conv_rows(bias2, B, Ho, Wo),
                            res=None if res is None else res.reshape(B * Ho * Wo, -1))
    return ref.view(B, Ho, Wo, -1), bound.view(B, Ho, Wo, -1)


def conv_restate(x, w, mode, bias=None, bias2=None, res=None, kgroups=2, ksplit=1, mutant=None):
    B, H, W, Cin = x.shape
    Ho, Wo = conv_out_hw(mode, H, W)
    acc = accumulate32(conv_gather(x, mode, mutant), w.reshape(w.shape[0], -1), kgroups, ksplit)
    out = epilogue_chain(acc, EPI_RESID if res is not None else EPI_NONE, bias=bias,
                         bias2=None if bias2 is None else _conv_rows(bias2, B, Ho, Wo),
                         res=None if res is None else res.reshape(B * Ho * Wo, -1))
    return out.view(B, Ho, Wo, -1)


def conv_f64(x, w, mode):
    """torch's own convolution in float64 -> [B, Ho, Wo, Cout]."""
    import torch.nn.functional as F
    xi = x.double().permute(0, 3, 1, 2)
    if mode == 3:
        xi = F.interpolate(xi, scale_factor=2.0, mode="nearest")
    return F.conv2d(xi, w.double().permute(0, 3, 1, 2), None, stride=2 if mode == 2 else 1, padding=1).permute(0, 2, 3, 1)


def tap_channels(Cin):
    return (0, 1, Cin // 2 + 3, Cin - 1)


def tap_inputs(B, H, W, Cin):
    """x: distinct bf16 values per (b, y, x, channel) -- the bit patterns 0x0800 + index of the normal numbers, the first 0x7000
    positive, the next 0x7000 negative --, w [36, 3, 3, Cin] one-hot: output channel 4 tap + j picks channel tap_channels(Cin)[j]
    under that tap.  Every product is x or +-0 and every sum has one non-zero term: the output is the source pixel's bits."""
    n = B * H * W * Cin
    assert n <= 2 * 0x7000
    i = torch.arange(n, dtype=torch.int32)
    x = (0x0800 + i % 0x7000 + (i // 0x7000) * 0x8000).to(torch.int16).view(BF16).view(B, H, W, Cin)
    w = torch.zeros(9 * TAP_CHANNELS, 3, 3, Cin)
    for tap in range(9):
        for j, c in enumerate(tap_channels(Cin)):
            w[tap * TAP_CHANNELS + j, tap // 3, tap % 3, c] = 1
    return x, w.to(BF16)


def tap_expected(x, mode):
    """[B, Ho, Wo, 36]: the source pixel conv_tap names for every output channel's tap, +0 outside the image."""
    B, H, W, Cin = x.shape
    Ho, Wo = conv_out_hw(mode, H, W)
    out = torch.zeros(B, Ho, Wo, 9 * TAP_CHANNELS, dtype=BF16)
    for py in range(Ho):
        for px in range(Wo):
            for tap in range(9):
                ok, yi, xi = conv_tap(mode, H, W, torch.tensor(py), torch.tensor(px), tap // 3, tap % 3)
                if bool(ok):
                    for j, c in enumerate(tap_channels(Cin)):
                        out[:, py, px, tap * TAP_CHANNELS + j] = x[:, int(yi), int(xi), c]
    return out


def rel_l2_passes(got, want, tol=1e-2):
    """The criterion of the conv tests in tests/test_gpu_unet.py: relative L2 below 1e-2 over the whole output."""
    got, want = got.double(), want.double()
    return float((got - want).norm() / want.norm().clamp_min(1e-12)) < tol
