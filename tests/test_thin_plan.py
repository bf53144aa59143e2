"""CPU: the one planner of the three matrix-core few-row weight streams (emu_gemv_thin_plan: gemv.hip's gemv_thin_plan, no GPU, no
HIP call) -- bf16 (csrc/gemv_thin.hip, family 4), fp8 (csrc/gemv_fp8_thin.hip, family 8) and MXFP4 (csrc/gemv_fp4_thin.hip, family 9).
The expectations are older than the planner: the MXFP4 tile table is the four-way choice the kernel file used to make at launch
time, written out by hand; the fp8 figures are the literal ones of tests/test_fp8_wide_host.py; the bf16 ones are the launches
recorded in tests/test_gemv_plan.py::EXPECTED."""
import ctypes as C

import pytest

from emu_amd import _lib
from tests.test_capi_symbols import _ensure_built
from tests.test_fp8_wide_host import BUCKETS, PROJECTIONS
from tests.test_gemv_plan import (BF16, EXPECTED, FP4, FP8, NO_THIN, OPS_THIN, PlanC, ShapeC, cases, llama33, render, scale_stride,
                                  shape)

THIN, FP8_THIN, FP4_THIN = 4, 8, 9
NONE, RESID, SWIGLU, SILU, GELU = range(5)
PIN16, PIN32 = 1 << 28, 2 << 28


def plan(sh, tune=0):
    _ensure_built()
    out = PlanC()
    st = _lib.lib().emu_gemv_thin_plan(C.byref(ShapeC(*sh)), tune, C.byref(out))
    assert st == out.status
    return out


def fields(p):
    return (p.status, p.family, p.rows, p.mb, p.stages, p.kch, p.grid, p.block)


def every_field(p):
    return tuple(getattr(p, n) for n, _ in PlanC._fields_)


def refused(p):
    return all(getattr(p, n) == (-22 if n == "status" else 0) for n, _ in PlanC._fields_)


# ------------------------------------------------------------------------------------------------------------------ MXFP4
#          (M <= 8, weight rows pinned to 16): (rows, mb, stages)
FP4_TILE = {(True, False): (32, 8, 5), (True, True): (16, 8, 6), (False, False): (32, 16, 4), (False, True): (16, 16, 4)}
# the five 33B projections of every tensor-parallel degree (TP 4 / 8: widths 1664 and 896 and K = 2240 end in a partial stage)
FP4_SHAPES = [(N, K, epi) for tp in (1, 2, 4, 8) for _, N, K, _, epi in llama33(tp)] + [(37, 256, NONE)]


@pytest.mark.parametrize("tune", [0, PIN16, PIN32])
@pytest.mark.parametrize("M", [1, 2, 3, 5, 8, 9, 16])
def test_mxfp4_tile_table(M, tune):
    assert any(K % 256 for _, K, _ in FP4_SHAPES) and any(K % 256 == 0 for _, K, _ in FP4_SHAPES)
    rows, mb, stages = FP4_TILE[(M <= 8, tune == PIN16)]
    for N, K, epi in FP4_SHAPES:
        p = plan(shape(M, N, K, epi, kind=FP4), tune)
        assert fields(p) == (0, FP4_THIN, rows, mb, stages, 8, (N + rows - 1) // rows, 256), (N, K)
        assert (p.form, p.waves, p.trips, p.vb, p.tpr, p.row_sets, p.rpl, p.partition) == (0, 4, 0, 0, 0, 0, 0, 0)


K4 = 768
FP4_REFUSALS = {
    "M 0": dict(M=0), "M 17": dict(M=17), "N 0": dict(N=0), "K 224": dict(K=224), "K 128": dict(K=128), "K % 32": dict(K=784, ldw=400),
    "ldw % 16": dict(ldw=K4 // 2 + 8), "ldx % 8": dict(ldx=K4 + 4), "lds % 4": dict(lds=scale_stride(K4) + 2),
    "ldw < K / 2": dict(ldw=K4 // 2 - 16), "ldx < K": dict(ldx=K4 - 8), "lds < stride": dict(lds=scale_stride(K4) - 4),
    "lds < stride, partial stage": dict(K=896, lds=28), "norm": dict(norm=1), "fp8 as well": dict(fp8=1),
    "W unaligned": dict(w_aligned=0), "x unaligned": dict(x_aligned=0), "SiLU": dict(epi=SILU), "GELU": dict(epi=GELU),
    "epi 5": dict(epi=5), "epi -1": dict(epi=-1), "SwiGLU, odd N": dict(N=263, epi=SWIGLU),
}


@pytest.mark.parametrize("why", sorted(FP4_REFUSALS))
def test_mxfp4_refusals_one_at_a_time(why):
    kw = dict(M=5, N=264, K=K4, kind=FP4)
    assert plan(shape(**kw)).status == 0
    kw.update(FP4_REFUSALS[why])
    assert refused(plan(shape(**kw))), why


def test_mxfp4_partial_stage_scale_rows():
    """K = 896: 28 scale bytes per row, fetched as 4 stages of 8 -- a stride of 32 is the least that is taken"""
    assert scale_stride(896) == 32
    assert plan(shape(5, 264, 896, kind=FP4)).status == 0 and plan(shape(5, 264, 896, kind=FP4, lds=36)).status == 0


# -------------------------------------------------------------------------------------------------------------------- fp8
def lds_fp8(p):
    return p.stages * (p.rows * 256 + p.mb * 512)


@pytest.mark.parametrize("name", sorted(PROJECTIONS))
@pytest.mark.parametrize("M", sorted(BUCKETS))
def test_fp8_plan_of_the_33b_projections(name, M):
    N, K, grid = PROJECTIONS[name]
    mb, stages = BUCKETS[M]
    p = plan(shape(M, N, K, SWIGLU if name == "gate/up" else RESID if name in ("o", "down") else NONE, kind=FP8))
    assert fields(p) == (0, FP8_THIN, 32, mb, stages, 16, grid, 256)
    assert lds_fp8(p) == 49152
    assert (p.form, p.waves, p.trips, p.vb, p.tpr, p.row_sets, p.rpl, p.partition) == (0, 4, 0, 0, 0, 0, 0, 0)


def test_fp8_plan_small_n_and_pinned_rows():
    for N in (16, 37, 64, 1000, 4064):
        assert fields(plan(shape(5, N, 512, kind=FP8))) == (0, FP8_THIN, 16, 8, 6, 16, (N + 15) // 16, 256)
    assert plan(shape(5, 4065, 512, kind=FP8)).rows == 32
    assert fields(plan(shape(16, 64, 512, kind=FP8))) == (0, FP8_THIN, 16, 16, 4, 16, 4, 256)
    assert fields(plan(shape(16, 64, 512, kind=FP8), PIN32)) == (0, FP8_THIN, 32, 16, 3, 16, 2, 256)
    assert fields(plan(shape(5, 3 * 6656, 6656, kind=FP8), PIN16)) == (0, FP8_THIN, 16, 8, 6, 16, 1248, 256)
    for M in (1, 2):
        assert fields(plan(shape(M, 64, 256, kind=FP8)))[:4] == (0, FP8_THIN, 16, 8)
    for p in (plan(shape(5, 64, 512, kind=FP8)), plan(shape(16, 64, 512, kind=FP8)), plan(shape(16, 64, 512, kind=FP8), PIN32)):
        assert lds_fp8(p) == 49152


@pytest.mark.parametrize("kw", [dict(M=5, N=64, K=384), dict(M=5, N=64, K=128), dict(M=5, N=64, K=896), dict(M=17, N=64, K=256),
                                dict(M=0, N=64, K=256), dict(M=5, N=0, K=256), dict(M=5, N=64, K=256, ldw=264),
                                dict(M=5, N=64, K=256, ldx=260), dict(M=5, N=64, K=512, ldw=256), dict(M=5, N=64, K=512, ldx=256),
                                dict(M=5, N=63, K=256, epi=SWIGLU), dict(M=5, N=64, K=256, epi=GELU), dict(M=5, N=64, K=256, epi=SILU),
                                dict(M=5, N=64, K=256, epi=5), dict(M=5, N=64, K=256, epi=-1), dict(M=5, N=64, K=256, norm=1),
                                dict(M=5, N=64, K=256, fp4=1), dict(M=5, N=64, K=256, w_aligned=0), dict(M=5, N=64, K=256, x_aligned=0)])
def test_fp8_refusals(kw):
    assert refused(plan(shape(kind=FP8, **kw)))


# ------------------------------------------------------------------------------------------------------------------- bf16
def recorded_thin():
    return [(cid, sh, t) for cid, sh, t in cases() if sh[0] >= 4 and EXPECTED[cid].startswith("0 | thin ")]


def test_bf16_plan_is_the_recorded_thin_launch():
    rec = recorded_thin()
    assert len(rec) > 100 and {t for _, _, t in rec} >= {0, 1 << 8, 2 << 8, 3 << 8}
    bad = [f"{cid}: {render(plan(sh, t))}  (recorded: {EXPECTED[cid]})" for cid, sh, t in rec if render(plan(sh, t)) != EXPECTED[cid]]
    assert not bad, "\n".join(bad[:40])


def test_bf16_two_and_three_rows_and_bit_2():
    for N, K in OPS_THIN:
        for M in (2, 3):
            assert fields(plan(shape(M, N, K))) == (0, THIN, 16, 8, 4, 32, (N + 15) // 16, 256)
        assert refused(plan(shape(1, N, K))) and refused(plan(shape(17, N, K)))
    for cid, sh, t in recorded_thin():                             # bit 2 is gemv_plan's routing, not the stream's
        assert render(plan(sh, t | NO_THIN)) == EXPECTED[cid], cid


@pytest.mark.parametrize("kw", [dict(K=260), dict(K=128), dict(K=896), dict(ldw=772), dict(ldx=772), dict(norm=1), dict(w_aligned=0),
                                dict(x_aligned=0), dict(N=0), dict(N=263, epi=SWIGLU), dict(epi=5), dict(epi=-1)])
def test_bf16_refusals(kw):
    base = dict(M=5, N=264, K=768)
    assert plan(shape(**base)).status == 0
    base.update(kw)
    assert refused(plan(shape(**base)))


# -------------------------------------------------------------------------------------------------------------- tune bits
def test_thin_plan_reads_bits_8_to_11_for_bf16_and_28_to_29_for_the_byte_kinds_only():
    every = 0x7fffffff
    for kind, read in ((BF16, 15 << 8), (FP8, 3 << 28), (FP4, 3 << 28)):
        for M in (3, 5, 9, 16):
            for N, K in ((264, 768), (19968, 6656), (6656, 17920), (37, 256)):
                sh = shape(M, N, K, kind=kind)
                for t in (0, 1 << 8, 2 << 8, 3 << 8, PIN16, PIN32):
                    assert every_field(plan(sh, (t & read) | (every & ~read))) == every_field(plan(sh, t & read)), (kind, M, N, K, t)
    assert plan(shape(5, 19968, 6656), 1 << 8).rows == 32 and plan(shape(5, 19968, 6656, kind=FP4), PIN16).rows == 16


def test_symbol_and_prototype():
    _ensure_built()
    assert "emu_gemv_thin_plan" in _lib.declared_symbols() and "emu_gemv_thin_plan" in _lib._PROTOS
    assert hasattr(_lib.lib(), "emu_gemv_thin_plan") and _lib.lib().emu_version() == _lib.ABI_VERSION
