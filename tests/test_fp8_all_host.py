"""CPU: the host side of running LLaMA from the fp8 weights alone (the fp8_all switch beside fp8 modes 5 / 6, kernel 10 = the 64 x 128
form of csrc/gemm_fp8.hip for 65 rows and more) -- the rule that picks a projection's kernel (emu_llama_projection_kernel) under the
switch, written out by hand, not computed; the head site; the refusals; the launch plan (emu_gemm_fp8t_plan); and the agreement of
header, ctypes prototypes and exported symbols for what is new.  Integers only, no GPU, no HIP call."""
import ctypes as C
import re

import pytest

from emu_amd import _lib
from tests.test_capi_symbols import _ensure_built
from tests.test_llama_weight_kernel import WIDTHS

BF16, FP8_ROWS, FP8_GEMM, FP8_THIN, FP8_STREAM, FP8_TILE = 0, 1, 2, 7, 9, 10      # include/emu_hip.h
ROWS = (1, 2, 3, 16, 17, 64, 65, 128, 770)
_, R8, G8, T8, S8, X8 = BF16, FP8_ROWS, FP8_GEMM, FP8_THIN, FP8_STREAM, FP8_TILE
# (widths, fp8 mode) -> the kernel of a layer matrix with an fp8 copy at each of ROWS.  OFF: the switch off (what tests/test_fp8_mid_host.py
# pins for the call-level rule); ON: fp8_all = 1 -- up to 64 rows the same, from 65 rows mode 5 runs kernel 10 and mode 6 keeps the W8A8
# GEMMs where the three widths are whole multiples of 256 (896 and 2240 are not: today's answer)
OFF = {
    #                        1   2   3   16  17  64  65  128 770
    ("33b", 5):             (R8, R8, T8, T8, S8, S8, _,  _,  _),
    ("33b", 6):             (R8, R8, T8, T8, S8, S8, G8, G8, G8),
    ("33b tp8 shard", 5):   (R8, R8, _,  _,  _,  _,  _,  _,  _),
    ("33b tp8 shard", 6):   (R8, R8, _,  _,  _,  _,  _,  _,  _),
    ("1024/2048", 5):       (R8, R8, T8, T8, S8, S8, _,  _,  _),
    ("1024/2048", 6):       (R8, R8, T8, T8, S8, S8, G8, G8, G8),
}
ON = {
    #                        1   2   3   16  17  64  65  128 770
    ("33b", 5):             (R8, R8, T8, T8, S8, S8, X8, X8, X8),
    ("33b", 6):             (R8, R8, T8, T8, S8, S8, G8, G8, G8),
    ("33b tp8 shard", 5):   (R8, R8, _,  _,  _,  _,  _,  _,  _),
    ("33b tp8 shard", 6):   (R8, R8, _,  _,  _,  _,  _,  _,  _),
    ("1024/2048", 5):       (R8, R8, T8, T8, S8, S8, X8, X8, X8),
    ("1024/2048", 6):       (R8, R8, T8, T8, S8, S8, G8, G8, G8),
}
EPI_NONE, EPI_RESID, EPI_SWIGLU = 0, 1, 2
LDS_PER_CU = 160 * 1024
VOCAB = 32274
NEW_SYMBOLS = ("emu_gemm_fp8t_plan", "emu_linear_fp8w_tile_bf16", "emu_llama_use_fp8_all", "emu_llama_projection_kernel")


@pytest.fixture(scope="module")
def L():
    _ensure_built()
    return _lib.lib()


def ask(L, fp8, rows, widths, fp4=0, N=6656, K=6656, **facts):
    q = _lib.ProjectionC(fp8=fp8, fp4=fp4, rows=rows, hidden=widths[0], heads_dim_local=widths[1], ffn_local=widths[2], N=N, K=K, **facts)
    return L.emu_llama_projection_kernel(C.byref(q))


# ------------------------------------------------------------------------------------------------------------------ the rule
def test_tables_cover_the_grid():
    want = {(w, f8) for w in WIDTHS for f8 in (5, 6)}
    assert set(OFF) == want and set(ON) == want and all(len(v) == len(ROWS) for t in (OFF, ON) for v in t.values())


@pytest.mark.parametrize("w,f8", sorted(ON))
def test_layer_matrix_under_the_switch(L, w, f8):
    assert tuple(ask(L, f8, r, WIDTHS[w], has_fp8=1, fp8_all=1) for r in ROWS) == ON[(w, f8)]


@pytest.mark.parametrize("w,f8", sorted(OFF))
def test_switch_off_is_todays_answer(L, w, f8):
    got = tuple(ask(L, f8, r, WIDTHS[w], has_fp8=1, fp8_all=0) for r in ROWS)
    assert got == OFF[(w, f8)]
    assert got == tuple(L.emu_llama_weight_kernel(f8, 0, r, *WIDTHS[w]) for r in ROWS)        # the older hook answers with the switch off
    assert all(a == b for a, b, r in zip(ON[(w, f8)], OFF[(w, f8)], ROWS) if r <= 64)


@pytest.mark.parametrize("rows", [65, 770])
def test_head_site(L, rows):
    head = dict(widths=WIDTHS["33b"], N=VOCAB, K=6656, head=1, ws_fits=1, fp8_all=1)
    for f8 in (5, 6):
        assert ask(L, f8, rows, has_fp8=1, **head) == FP8_TILE
        assert ask(L, f8, rows, has_fp8=0, **head) == BF16
        assert ask(L, f8, rows, has_fp8=1, **dict(head, fp8_all=0)) == BF16     # the switch off: no W8A8 GEMM at the head, mode 5 is bf16


def test_head_few_row_stream_stays_after_a_release(L):
    head = dict(widths=WIDTHS["33b"], N=VOCAB, K=6656, head=1, has_fp8=1, fp8_all=1)
    for f8 in (5, 6):
        assert ask(L, f8, 5, ws_fits=0, bf16_released=1, **head) == FP8_THIN
        assert ask(L, f8, 5, ws_fits=0, bf16_released=0, **head) == BF16
        assert ask(L, f8, 5, ws_fits=1, bf16_released=0, **head) == FP8_THIN


def test_refusals(L):
    w = WIDTHS["33b"]
    for f8 in range(5):
        assert ask(L, f8, 65, w, has_fp8=1, fp8_all=1) == -22, f8
    assert ask(L, 0, 65, w, fp4=1, has_fp8=1, fp8_all=1) == -22
    assert ask(L, 5, 65, w, fp4=1, has_fp8=1, fp8_all=1) == -22
    assert ask(L, 5, 65, w, has_fp8=1, fp8_all=2) == -22
    assert ask(L, 5, 65, w, has_fp8=1, fp8_all=-1) == -22
    assert L.emu_llama_projection_kernel(None) == -22
    for f8 in (7, -1):                                                       # the mode itself stays 0..6
        assert ask(L, f8, 65, w, has_fp8=1, fp8_all=0) == -22


# ------------------------------------------------------------------------------------------------------------------ the plan
def plan(M, N, K, ldx=None, ldw=None, epi=EPI_NONE, tune=0):
    _ensure_built()
    p = _lib.GemmFp8tPlanC()
    st = _lib.lib().emu_gemm_fp8t_plan(M, N, K, K if ldx is None else ldx, K if ldw is None else ldw, epi, tune, C.byref(p))
    assert st == p.status
    return p


@pytest.mark.parametrize("M,N,K,gx,gy", [(65, 64, 256, 1, 1), (128, 37, 512, 1, 1), (129, 1000, 6656, 2, 16), (770, 32274, 6656, 7, 505)])
def test_plan(M, N, K, gx, gy):
    for tune in (0, 1 << 20):
        p = plan(M, N, K, tune=tune)
        assert (p.status, p.form, p.bm, p.kc, p.grid_x, p.grid_y, p.block) == (0, 3, 128, 256, gx, gy, 256)
        assert p.stages >= 2 and p.lds_bytes == p.stages * (64 * 256 + 128 * 512) and p.lds_bytes <= LDS_PER_CU == 163840


@pytest.mark.parametrize("kw", [dict(M=64), dict(K=384), dict(K=0), dict(ldw=256 + 8), dict(ldx=256 + 4), dict(N=64 * 65536), dict(M=0),
                                dict(N=0), dict(N=37, epi=EPI_SWIGLU), dict(epi=3), dict(ldx=248), dict(K=128)])
def test_plan_refusals(kw):
    a = dict(M=65, N=64, K=256)
    a.update(kw)
    p = plan(**a)
    assert p.status == -22
    assert (p.form, p.bm, p.kc, p.stages, p.lds_bytes, p.grid_x, p.grid_y, p.block) == (0,) * 8


def test_plan_takes_what_the_kernel_takes():
    assert plan(65, 38, 512, epi=EPI_SWIGLU).status == 0
    assert plan(65, 37, 512, epi=EPI_RESID).status == 0
    assert plan(65, 64, 256, ldw=272, ldx=264).status == 0                   # strided rows on 16-byte boundaries
    assert plan(65, 64 * 65535, 256).grid_y == 65535
    # the sibling keeps its range: 65 rows are refused there, 64 here
    p = _lib.GemmFp8wPlanC()
    assert _lib.lib().emu_gemm_fp8w_plan(65, 64, 256, 256, 256, 0, 0, C.byref(p)) == -22


# ------------------------------------------------------------------------------------------------------------------ consistency
def test_header_prototypes_and_exports_agree(L):
    txt = open(_lib.HEADER_PATH).read()
    declared = _lib.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and s in _lib._PROTOS and hasattr(L, s), s
    tile = _lib._PROTOS["emu_linear_fp8w_tile_bf16"]
    assert tile == _lib._PROTOS["emu_linear_fp8w_gemm_bf16"]                 # the sibling's argument list
    assert _lib._PROTOS["emu_gemm_fp8t_plan"] == _lib._PROTOS["emu_gemm_fp8w_plan"]
    # the struct mirrors: the plan's fields and the appended mode field, in the header's order
    m = re.search(r"typedef struct \{\s*int ([^;]+);\s*\} emu_gemm_fp8t_plan_t;", txt)
    assert m and [f.strip() for f in m.group(1).split(",")] == [n for n, _ in _lib.GemmFp8tPlanC._fields_]
    m = re.search(r"typedef struct emu_weight_mode \{ int ([^;]+); \} emu_weight_mode;", txt)
    mode = [f.strip() for f in m.group(1).split(",")]
    assert mode[-1] == "fp8_all" and mode == [n for n, _ in _lib.ProjectionC._fields_[:len(mode)]]
    assert L.emu_version() == 6 == _lib.ABI_VERSION
