"""CPU: the rule that picks a LLaMA projection's weight set and kernel (emu_llama_weight_kernel: engine.hip's weight_kernel, the one
function emu_llama_forward's plan and emu_llama_logits' head both ask; integers only, no GPU, no HIP call).  EXPECTED is written out
from the documented behaviour of LlamaEngine.use_fp8 / use_fp4 (emu_amd/llama.py) and emu_llama_use_fp8 / emu_llama_use_fp4
(include/emu_hip.h), not computed: 1..2 rows stream the 4-bit or the fp8 set when either mode is on, 3..16 rows stream the 4-bit set
from fp4 mode 2, 17 rows and more run the 4-bit GEMM in fp4 mode 3 and W8A8 GEMMs in fp8 mode 2 when every reduction width is a
multiple of 128; everything else is bf16."""
import pytest

from emu_amd import _lib
from tests.test_capi_symbols import _ensure_built

BF16, FP8_ROWS, FP8_GEMM, FP4_ROWS, FP4_THIN, FP4_GEMM = range(6)       # include/emu_hip.h
ROWS = (1, 2, 3, 8, 9, 16, 17, 770)
# (hidden, heads_local * head_dim, ffn_local)
WIDTHS = {
    "33b": (6656, 6656, 17920),
    "33b tp8 shard": (6656, 896, 2240),          # 7 heads, ffn 17920 / 8 = 17.5 x 128: no whole 128-element k tiles
    "1024/2048": (1024, 1024, 2048),
}
_, R8, G8, R4, T4, G4 = BF16, FP8_ROWS, FP8_GEMM, FP4_ROWS, FP4_THIN, FP4_GEMM
# (widths, fp8 mode, fp4 mode) -> the kernel at each of ROWS; fp8 and fp4 are exclusive (the setters refuse both): not in the grid
EXPECTED = {
    #                            1   2   3   8   9   16  17  770
    ("33b", 0, 0):              (_,  _,  _,  _,  _,  _,  _,  _),
    ("33b", 1, 0):              (R8, R8, _,  _,  _,  _,  _,  _),
    ("33b", 2, 0):              (R8, R8, _,  _,  _,  _,  G8, G8),
    ("33b", 0, 1):              (R4, R4, _,  _,  _,  _,  _,  _),
    ("33b", 0, 2):              (R4, R4, T4, T4, T4, T4, _,  _),
    ("33b", 0, 3):              (R4, R4, T4, T4, T4, T4, G4, G4),
    ("33b tp8 shard", 0, 0):    (_,  _,  _,  _,  _,  _,  _,  _),
    ("33b tp8 shard", 1, 0):    (R8, R8, _,  _,  _,  _,  _,  _),
    ("33b tp8 shard", 2, 0):    (R8, R8, _,  _,  _,  _,  _,  _),
    ("33b tp8 shard", 0, 1):    (R4, R4, _,  _,  _,  _,  _,  _),
    ("33b tp8 shard", 0, 2):    (R4, R4, T4, T4, T4, T4, _,  _),
    ("33b tp8 shard", 0, 3):    (R4, R4, T4, T4, T4, T4, G4, G4),
    ("1024/2048", 0, 0):        (_,  _,  _,  _,  _,  _,  _,  _),
    ("1024/2048", 1, 0):        (R8, R8, _,  _,  _,  _,  _,  _),
    ("1024/2048", 2, 0):        (R8, R8, _,  _,  _,  _,  G8, G8),
    ("1024/2048", 0, 1):        (R4, R4, _,  _,  _,  _,  _,  _),
    ("1024/2048", 0, 2):        (R4, R4, T4, T4, T4, T4, _,  _),
    ("1024/2048", 0, 3):        (R4, R4, T4, T4, T4, T4, G4, G4),
}
# the row range each kernel's call sites hand it (fp4_mfma_ok refuses the rest: Fp4Thin 1..16, Fp4Gemm 17 and more; the two
# few-row streams take 1..2 rows, the W8A8 GEMM more than 16)
ROW_RANGE = {BF16: (1, None), FP8_ROWS: (1, 2), FP8_GEMM: (17, None), FP4_ROWS: (1, 2), FP4_THIN: (1, 16), FP4_GEMM: (17, None)}


def grid():
    return [(w, f8, f4) for w in WIDTHS for f8 in (0, 1, 2) for f4 in (0, 1, 2, 3) if not (f8 and f4)]


def kernel(w, f8, f4, rows):
    return _lib.lib().emu_llama_weight_kernel(f8, f4, rows, *WIDTHS[w])


def test_grid_is_the_table():
    assert set(grid()) == set(EXPECTED) and all(len(v) == len(ROWS) for v in EXPECTED.values())


@pytest.mark.parametrize("w,f8,f4", grid())
def test_weight_kernel_matches_the_documented_rule(w, f8, f4):
    _ensure_built()
    assert tuple(kernel(w, f8, f4, r) for r in ROWS) == EXPECTED[(w, f8, f4)]


@pytest.mark.parametrize("w,f8,f4", grid())
def test_weight_kernel_implies_its_row_range(w, f8, f4):
    """No row count reaches a kernel whose argument check excludes it."""
    _ensure_built()
    for r in ROWS:
        lo, hi = ROW_RANGE[kernel(w, f8, f4, r)]
        assert lo <= r and (hi is None or r <= hi), (r, kernel(w, f8, f4, r))
