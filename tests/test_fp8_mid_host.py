"""CPU: the host side of the fp8 W8A16 GEMM for steps of 17..64 rows (csrc/gemm_fp8.hip, fp8 modes 5 / 6) -- the rule that picks a
projection's kernel (emu_llama_weight_kernel) over fp8 modes 0..6, written out, not computed, and the launch plan
(emu_gemm_fp8w_plan): form by row count, grid, block, ring depth, LDS bytes and the refusals.  Integers only, no GPU, no HIP call."""
import ctypes as C

import pytest

from emu_amd import _lib
from tests.test_capi_symbols import _ensure_built
from tests.test_llama_weight_kernel import WIDTHS

BF16, FP8_ROWS, FP8_GEMM, FP8_THIN, FP8_STREAM = 0, 1, 2, 7, 9               # include/emu_hip.h
ROWS = (1, 2, 3, 16, 17, 20, 32, 33, 64, 65, 770)
_, R8, G8, T8, S8 = BF16, FP8_ROWS, FP8_GEMM, FP8_THIN, FP8_STREAM
# (widths, fp8 mode) -> the kernel at each of ROWS (fp4 mode 0).  Modes 0..2: tests/test_llama_weight_kernel.py; 3 / 4:
# tests/test_fp8_wide_host.py; 5 / 6 = 3 / 4 plus 17..64 rows where the three widths are multiples of 256
EXPECTED = {
    #                        1   2   3   16  17  20  32  33  64  65  770
    ("33b", 0):             (_,  _,  _,  _,  _,  _,  _,  _,  _,  _,  _),
    ("33b", 1):             (R8, R8, _,  _,  _,  _,  _,  _,  _,  _,  _),
    ("33b", 2):             (R8, R8, _,  _,  G8, G8, G8, G8, G8, G8, G8),
    ("33b", 3):             (R8, R8, T8, T8, _,  _,  _,  _,  _,  _,  _),
    ("33b", 4):             (R8, R8, T8, T8, G8, G8, G8, G8, G8, G8, G8),
    ("33b", 5):             (R8, R8, T8, T8, S8, S8, S8, S8, S8, _,  _),
    ("33b", 6):             (R8, R8, T8, T8, S8, S8, S8, S8, S8, G8, G8),
    # 896 and 2240: no multiples of 256 (nor of 128), so neither matrix-core stream nor the W8A8 GEMM
    ("33b tp8 shard", 0):   (_,  _,  _,  _,  _,  _,  _,  _,  _,  _,  _),
    ("33b tp8 shard", 1):   (R8, R8, _,  _,  _,  _,  _,  _,  _,  _,  _),
    ("33b tp8 shard", 2):   (R8, R8, _,  _,  _,  _,  _,  _,  _,  _,  _),
    ("33b tp8 shard", 3):   (R8, R8, _,  _,  _,  _,  _,  _,  _,  _,  _),
    ("33b tp8 shard", 4):   (R8, R8, _,  _,  _,  _,  _,  _,  _,  _,  _),
    ("33b tp8 shard", 5):   (R8, R8, _,  _,  _,  _,  _,  _,  _,  _,  _),
    ("33b tp8 shard", 6):   (R8, R8, _,  _,  _,  _,  _,  _,  _,  _,  _),
    ("1024/2048", 0):       (_,  _,  _,  _,  _,  _,  _,  _,  _,  _,  _),
    ("1024/2048", 1):       (R8, R8, _,  _,  _,  _,  _,  _,  _,  _,  _),
    ("1024/2048", 2):       (R8, R8, _,  _,  G8, G8, G8, G8, G8, G8, G8),
    ("1024/2048", 3):       (R8, R8, T8, T8, _,  _,  _,  _,  _,  _,  _),
    ("1024/2048", 4):       (R8, R8, T8, T8, G8, G8, G8, G8, G8, G8, G8),
    ("1024/2048", 5):       (R8, R8, T8, T8, S8, S8, S8, S8, S8, _,  _),
    ("1024/2048", 6):       (R8, R8, T8, T8, S8, S8, S8, S8, S8, G8, G8),
}
EPI_NONE, EPI_RESID, EPI_SWIGLU = 0, 1, 2
NARROW, ONE_TILE = 1, 2
LDS_PER_CU = 160 * 1024


def test_grid_is_the_table():
    assert set(EXPECTED) == {(w, f8) for w in WIDTHS for f8 in range(7)} and all(len(v) == len(ROWS) for v in EXPECTED.values())


@pytest.mark.parametrize("w,f8", sorted(EXPECTED))
def test_weight_kernel_over_fp8_modes_0_to_6(w, f8):
    _ensure_built()
    assert tuple(_lib.lib().emu_llama_weight_kernel(f8, 0, r, *WIDTHS[w]) for r in ROWS) == EXPECTED[(w, f8)]


def test_weight_kernel_modes_0_to_4_are_what_the_older_table_pins():
    """The rows both tables hold, under the modes the older one holds: the same kernels."""
    from tests.test_llama_weight_kernel import EXPECTED as OLD, ROWS as OLD_ROWS
    for (w, f8, f4), kernels in OLD.items():
        if f4 == 0:
            for r, k in zip(OLD_ROWS, kernels):
                if r in ROWS:
                    assert EXPECTED[(w, f8)][ROWS.index(r)] == k, (w, f8, r)


def plan(M, N, K, ldx=None, ldw=None, epi=EPI_NONE, tune=0):
    _ensure_built()
    p = _lib.GemmFp8wPlanC()
    st = _lib.lib().emu_gemm_fp8w_plan(M, N, K, K if ldx is None else ldx, K if ldw is None else ldw, epi, tune, C.byref(p))
    assert st == p.status
    return p


@pytest.mark.parametrize("M,form,bm", [(17, NARROW, 32), (32, NARROW, 32), (33, ONE_TILE, 64), (64, ONE_TILE, 64)])
def test_plan_form_by_rows(M, form, bm):
    for tune in (0, 1 << 20):
        p = plan(M, 1000, 6656, tune=tune)
        assert (p.status, p.form, p.bm, p.kc, p.block) == (0, form, bm, 256, 256)
        assert p.stages >= 2 and p.lds_bytes == p.stages * (64 * 256 + bm * 512) and p.lds_bytes <= LDS_PER_CU


@pytest.mark.parametrize("N,grid", [(16, 1), (37, 1), (64, 1), (1000, 16), (32274, 505)])
def test_plan_grid_is_ceil_n_over_64(N, grid):
    for M in (17, 32, 33, 64):
        p = plan(M, N, 512)
        assert p.status == 0 and p.grid == grid and p.block == 256


def test_plan_ring_depths_and_the_two_workgroup_twin():
    """One workgroup per CU by default: the ring as deep as 160 KiB hold (narrow 4 x 32 KiB, one tile 3 x 48 KiB).  emu_gemm_tune
    bit 20: the narrow form at ring 2, 64 KiB, so two workgroups fit a CU; the one-tile form does not read the bit."""
    assert (plan(20, 6656, 6656).stages, plan(20, 6656, 6656).lds_bytes) == (4, 128 * 1024)
    assert (plan(64, 6656, 6656).stages, plan(64, 6656, 6656).lds_bytes) == (3, 144 * 1024)
    two = plan(20, 6656, 6656, tune=1 << 20)
    assert (two.stages, two.lds_bytes) == (2, 64 * 1024) and 2 * two.lds_bytes <= LDS_PER_CU
    assert plan(64, 6656, 6656, tune=1 << 20).stages == 3


@pytest.mark.parametrize("kw", [dict(M=16), dict(M=65), dict(M=0), dict(K=384), dict(K=128), dict(ldw=264), dict(N=37, epi=EPI_SWIGLU),
                                dict(N=0), dict(ldx=260), dict(ldx=248), dict(epi=3)])
def test_plan_refusals(kw):
    a = dict(M=20, N=64, K=256)
    a.update(kw)
    p = plan(**a)
    assert p.status == -22
    assert (p.form, p.bm, p.kc, p.stages, p.lds_bytes, p.grid, p.block) == (0,) * 7


def test_plan_takes_what_the_kernel_takes():
    assert plan(20, 38, 512, epi=EPI_SWIGLU).status == 0
    assert plan(20, 37, 512, epi=EPI_RESID).status == 0
    assert plan(20, 64, 256, ldw=272, ldx=264).status == 0                        # strided rows on 16-byte boundaries
