"""CPU: the planner of the 13-bit packed few-row stream (emu_gemv_pack_thin_plan: gemv.hip's gemv_pack_thin_plan) and the rule that
sends a 4..16-row bf16 projection to it (emu_llama_pack_thin_kernel: engine.hip's pack_thin_kernel) -- integers only, no GPU, no HIP
call.  The expectations are written from include/emu_hip.h: the plan exists exactly where emu_gemv_plan names the bf16 thin stream
(family 4) at kch 32, for sets of 2 / 4 rows and 4..16 activation rows; the rule answers 8 only for a bf16 projection with both
switches on and a set of its own shape.  The older hooks answer what they answered."""
import ctypes as C

import pytest

from emu_amd import _lib
from tests.test_capi_symbols import _ensure_built
from tests.test_gemv_plan import FP4, FP8, PlanC, ShapeC, llama33, shape

THIN, PACK_THIN = 4, 10
BF16, FP8_ROWS, FP8_GEMM, FP4_ROWS, FP4_THIN, FP4_GEMM, BF16_PACK, FP8_THIN, BF16_PACK_THIN = range(9)
NONE, RESID, SWIGLU, SILU, GELU = range(5)
PIN16, PIN32 = 1 << 28, 2 << 28
ROWS = list(range(4, 17))
# (name, N, K, epi) of the 33B projections and the head as a few-row step runs them (the RMSNorm is its own launch there), TP 1 and 2
PROJ = [(name, N, K, epi) for tp in (1, 2) for name, N, K, _, epi in llama33(tp)]


@pytest.fixture(scope="module")
def L():
    _ensure_built()
    return _lib.lib()


def plan(L, sh, set_rows, tune=0):
    out = PlanC()
    st = L.emu_gemv_pack_thin_plan(C.byref(ShapeC(*sh)), set_rows, tune, C.byref(out))
    assert st == out.status
    return out


def bf16_plan(L, sh, tune=0, hook="emu_gemv_plan"):
    out = PlanC()
    getattr(L, hook)(C.byref(ShapeC(*sh)), tune, C.byref(out))
    return out


def refused(p):
    return all(getattr(p, n) == (-22 if n == "status" else 0) for n, _ in PlanC._fields_)


# ------------------------------------------------------------------------------------------------------------------ the planner
# The built tiles of include/emu_hip.h -- (weight rows, ring depth, workgroups per CU) -- and the rule restated from it: the tile whose
# grid fills the largest share of its whole rounds of 256 x (workgroups per CU) places, the first of equals
TILES = {8: [(16, 4, 3), (32, 4, 2), (16, 6, 2), (32, 3, 3)], 16: [(16, 3, 3), (32, 3, 2), (16, 5, 2)]}
# ... and what it comes to at the 33B widths, written out: N -> (rows, stages) up to 8 activation rows, then up to 16
BY_HAND = {19968: ((16, 4), (16, 3)), 6656: ((16, 6), (16, 5)), 35840: ((16, 4), (16, 3)), 32274: ((32, 4), (32, 3)),
           9984: ((16, 4), (16, 3)), 17920: ((16, 4), (16, 3))}


def tile_by_rule(M, N, pin=0):
    from fractions import Fraction
    best = None
    for rows, stages, per_cu in TILES[8 if M <= 8 else 16]:
        if pin and rows != pin:
            continue
        grid, places = -(-N // rows), 256 * per_cu
        fill = Fraction(grid, -(-grid // places) * places)
        if best is None or fill > best[0]:
            best = (fill, rows, stages)
    return best[1], best[2]


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("M", ROWS)
def test_33b_projections_plan_the_twin_of_the_bf16_thin_stream(L, M, R):
    for name, N, K, epi in PROJ:
        sh = shape(M, N, K, epi)
        b = bf16_plan(L, sh)
        assert (b.status, b.family, b.kch) == (0, THIN, 32), name          # what the issue is about: these all plan the thin stream
        p = plan(L, sh, R)
        rows, stages = BY_HAND[N][M > 8]
        assert (rows, stages) == tile_by_rule(M, N), name
        assert (p.status, p.family, p.rows, p.mb, p.stages, p.kch, p.grid, p.block) == \
            (0, PACK_THIN, rows, 8 if M <= 8 else 16, stages, b.kch, (N + rows - 1) // rows, 256), name
        assert (p.form, p.waves, p.trips, p.vb, p.tpr, p.row_sets, p.rpl, p.partition) == (0, 4, 0, 0, 0, 0, 0, 0)
        for tune, pinned in ((PIN16, 16), (PIN32, 32)):
            q = plan(L, sh, R, tune)
            assert (q.status, q.rows, q.stages, q.grid, q.kch) == (0, pinned, tile_by_rule(M, N, pinned)[1], (N + pinned - 1) // pinned, 32)
        assert plan(L, sh, R, PIN16 | PIN32).rows == rows                   # both bits: no pin, as for the byte-fed streams


def test_lds_of_every_built_tile_fits_its_workgroups_per_cu(L):
    """A stage image is rows / 4 + rows / 8 + 1 + mb / 2 KiB (low bytes, nibbles, signs, activation rows); a flagged workgroup's bf16
    ring is 3 stages of (rows + mb) * 512 bytes where that fits the packed ring, else 2."""
    for mb, tiles in TILES.items():
        for rows, stages, per_cu in tiles:
            ring = stages * (rows // 4 + rows // 8 + 1 + mb // 2) * 1024
            bf16_stage = (rows + mb) * 512
            ring = max(ring, (3 if 3 * bf16_stage <= ring else 2) * bf16_stage)
            assert per_cu * ring <= 160 * 1024 < (per_cu + 1) * ring, (mb, rows, stages, ring)


REFUSALS = {
    "M 1": dict(M=1), "M 2": dict(M=2), "M 3": dict(M=3), "M 17": dict(M=17),
    "K 128": dict(K=128), "K 260": dict(K=260), "K 896": dict(K=896),
    "set_rows 0": dict(set_rows=0), "set_rows 3": dict(set_rows=3), "set_rows 8": dict(set_rows=8),
    "norm": dict(norm=1), "fp8": dict(kind=FP8), "fp4": dict(kind=FP4), "fp8 flag on bf16 strides": dict(fp8=1), "fp4 flag on bf16 strides": dict(fp4=1),
    "W unaligned": dict(w_aligned=0), "x unaligned": dict(x_aligned=0), "ldw % 8": dict(ldw=772), "ldx % 8": dict(ldx=772),
    "SwiGLU, odd N": dict(N=263, epi=SWIGLU), "SiLU": dict(epi=SILU), "GELU": dict(epi=GELU), "N 0": dict(N=0),
    "thin stream switched off": dict(tune=4), "kch 64 has no twin": dict(K=1024, tune=3 << 8),
}


@pytest.mark.parametrize("why", sorted(REFUSALS))
def test_refusals_one_at_a_time(L, why):
    kw = dict(M=5, N=264, K=768)
    extra = dict(set_rows=4, tune=0)
    assert plan(L, shape(**kw), **extra).status == 0
    assert plan(L, shape(**dict(kw, K=1024)), **extra).status == 0            # (the base of the kch 64 case)
    for k, v in REFUSALS[why].items():
        (extra if k in extra else kw)[k] = v
    assert refused(plan(L, shape(**kw), **extra)), why


def test_null_arguments(L):
    out = PlanC()
    assert L.emu_gemv_pack_thin_plan(None, 4, 0, C.byref(out)) == -22
    assert L.emu_gemv_pack_thin_plan(C.byref(ShapeC(*shape(5, 264, 768))), 4, 0, None) == -22


# ------------------------------------------------------------------------------------------------------------------ the rule
def rule(L, kernel=BF16, rows=5, pack_rows=4, set_n=None, set_k=None, on=1, wide=1, N=19968, K=6656, norm=0, epi=NONE, tune=0):
    return L.emu_llama_pack_thin_kernel(kernel, rows, pack_rows, N if set_n is None else set_n, K if set_k is None else set_k, on, wide,
                                        N, K, norm, epi, tune)


@pytest.mark.parametrize("rows", ROWS)
def test_rule_takes_the_packed_stream(L, rows):
    for name, N, K, epi in PROJ:
        for pr in (2, 4):
            assert rule(L, rows=rows, pack_rows=pr, N=N, K=K, epi=epi) == BF16_PACK_THIN, name


@pytest.mark.parametrize("kernel", [FP8_ROWS, FP8_GEMM, FP4_ROWS, FP4_THIN, FP4_GEMM, BF16_PACK, FP8_THIN, BF16_PACK_THIN])
def test_rule_passes_other_kernels_through(L, kernel):
    for name, N, K, epi in PROJ:
        assert rule(L, kernel=kernel, N=N, K=K, epi=epi) == kernel
    assert L.emu_llama_weight_kernel(3, 0, 5, 6656, 6656, 17920) == FP8_THIN and L.emu_llama_weight_kernel(0, 2, 5, 6656, 6656, 17920) == FP4_THIN
    assert rule(L, kernel=-1) == -22 and rule(L, kernel=9) == -22


def test_rule_answers_bf16_otherwise(L):
    for name, N, K, epi in PROJ:
        kw = dict(N=N, K=K, epi=epi)
        assert rule(L, **kw) == BF16_PACK_THIN
        assert rule(L, on=0, **kw) == BF16 and rule(L, wide=0, **kw) == BF16 and rule(L, on=0, wide=0, **kw) == BF16
        assert rule(L, pack_rows=0, **kw) == BF16                             # no set (also: a set released with the bf16 weights)
        assert rule(L, set_n=N - 8, **kw) == BF16 and rule(L, set_k=K - 256, **kw) == BF16        # a set of another matrix
        assert rule(L, norm=1, **kw) == BF16                                  # a fused norm has no thin stream
        assert rule(L, tune=4, **kw) == BF16                                  # the bf16 thin stream switched off
        for rows in (1, 2, 3, 17, 770):
            assert rule(L, rows=rows, **kw) == BF16, rows
    assert rule(L, N=6656, K=896, epi=RESID) == BF16                          # the TP = 8 o_proj: K % 256 != 0


# ------------------------------------------------------------------------------------------------------------------ old hooks
def test_old_hooks_answer_what_they_answered(L):
    """emu_llama_pack_kernel: 6 for one row only, never 8; emu_gemv_thin_plan / emu_gemv_plan: family 4 at 4..16 rows."""
    for name, N, K, norm, epi in llama33(1):
        for rows in (1, 2, 5, 8, 16, 17):
            got = L.emu_llama_pack_kernel(BF16, rows, 4 if norm else 2, 1, 0, 0, 0, N, K, norm, epi, 0)
            assert got == (BF16_PACK if rows == 1 else BF16), (name, rows)
    assert L.emu_llama_pack_kernel(BF16_PACK_THIN, 1, 4, 1, 0, 0, 0, 19968, 6656, 1, NONE, 0) == -22       # its range is unchanged
    for M in ROWS:
        for name, N, K, epi in PROJ:
            sh = shape(M, N, K, epi)
            t, b = bf16_plan(L, sh, hook="emu_gemv_thin_plan"), bf16_plan(L, sh)
            for p in (t, b):
                assert (p.status, p.family, p.rows, p.mb, p.stages, p.kch, p.grid, p.block) == \
                    (0, THIN, 16, 8 if M <= 8 else 16, 4, 32, (N + 15) // 16, 256), (name, M)
