"""CPU: the rule that says what a UNet transformer's blocks fuse and in which format their GEMMs run (emu_unet_block_plan:
unet_engine.hip's unet_block_plan, the one function run_transformer asks; integers only, no GPU, no HIP call).  EXPECTED is written out
from the documented behaviour of emu_unet_set_fusion / emu_unet_use_fp8 (include/emu_hip.h; UNetEngine.set_fusion / use_fp8), not
computed: above 8 rows, fusion bit 0 folds the LayerNorms into their consumer GEMMs where the channels fill whole 128-column statistics
slots, bit 1 lets the qkv projection store V^T and bit 2 runs the cross-attention inside the to_q projection where a batch element's
tokens fill whole 64-key groups (bit 2: and the prompt has no more than 64 tokens); fp8 mode takes the six GEMMs of a block where the
channels are a multiple of 128 and no more than 2048, keeps bits 1 and 2 and has no form of bit 0; every bf16 GEMM chain of at least one
block prefetches its successor's weights; 8 rows and fewer stream and fuse nothing."""
import pytest

from emu_amd import _lib
from tests.test_capi_symbols import _ensure_built

FACTS = "8LVXP"       # bits 0..4 of the result: fp8, ln_fold, vt_epilogue, cross_epilogue, prefetch (include/emu_hip.h)
# (M = rows, C, HW, n_ctx, depth)
SHAPES = {
    "level 1": (2048, 640, 1024, 64, 2),                 # the true widths of the two attention levels, the CFG pair
    "level 2": (512, 1280, 256, 64, 10),
    "level 1, 65 keys": (2048, 640, 1024, 65, 2),
    "level 1, 70 keys": (2048, 640, 1024, 70, 2),
    "level 2, 65 keys": (512, 1280, 256, 65, 10),
    "level 2, 70 keys": (512, 1280, 256, 70, 10),
    "C 320": (2048, 320, 1024, 64, 2),                   # no whole 128-column slots
    "C 2176": (2048, 2176, 1024, 64, 2),                 # whole slots, above the 2048 columns the quantising LayerNorm holds
    "HW 16": (32, 640, 16, 64, 2),                       # no whole 64-key groups
    "M 8": (8, 640, 4, 64, 2),
    "M 9": (9, 640, 9, 64, 2),
    "one CFG row": (1024, 640, 1024, 64, 2),             # M = HW
    "depth 0": (2048, 640, 1024, 64, 0),
}
# (shape, fp8) -> the facts under fusion masks 0..7
EXPECTED = {
    #                          0     1     2     3      4     5      6      7
    ("level 1", 0):           ("P",  "LP", "VP", "LVP", "XP", "LXP", "VXP", "LVXP"),
    ("level 1", 1):           ("8",  "8",  "8V", "8V",  "8X", "8X",  "8VX", "8VX"),
    ("level 2", 0):           ("P",  "LP", "VP", "LVP", "XP", "LXP", "VXP", "LVXP"),
    ("level 2", 1):           ("8",  "8",  "8V", "8V",  "8X", "8X",  "8VX", "8VX"),
    ("level 1, 65 keys", 0):  ("P",  "LP", "VP", "LVP", "P",  "LP",  "VP",  "LVP"),
    ("level 1, 65 keys", 1):  ("8",  "8",  "8V", "8V",  "8",  "8",   "8V",  "8V"),
    ("level 1, 70 keys", 0):  ("P",  "LP", "VP", "LVP", "P",  "LP",  "VP",  "LVP"),
    ("level 1, 70 keys", 1):  ("8",  "8",  "8V", "8V",  "8",  "8",   "8V",  "8V"),
    ("level 2, 65 keys", 0):  ("P",  "LP", "VP", "LVP", "P",  "LP",  "VP",  "LVP"),
    ("level 2, 65 keys", 1):  ("8",  "8",  "8V", "8V",  "8",  "8",   "8V",  "8V"),
    ("level 2, 70 keys", 0):  ("P",  "LP", "VP", "LVP", "P",  "LP",  "VP",  "LVP"),
    ("level 2, 70 keys", 1):  ("8",  "8",  "8V", "8V",  "8",  "8",   "8V",  "8V"),
    ("C 320", 0):             ("P",  "P",  "VP", "VP",  "XP", "XP",  "VXP", "VXP"),
    ("C 320", 1):             ("P",  "P",  "VP", "VP",  "XP", "XP",  "VXP", "VXP"),
    ("C 2176", 0):            ("P",  "LP", "VP", "LVP", "XP", "LXP", "VXP", "LVXP"),
    ("C 2176", 1):            ("P",  "LP", "VP", "LVP", "XP", "LXP", "VXP", "LVXP"),
    ("HW 16", 0):             ("P",  "LP", "P",  "LP",  "P",  "LP",  "P",   "LP"),
    ("HW 16", 1):             ("8",  "8",  "8",  "8",   "8",  "8",   "8",   "8"),
    ("M 8", 0):               ("",   "",   "",   "",    "",   "",    "",    ""),
    ("M 8", 1):               ("",   "",   "",   "",    "",   "",    "",    ""),
    ("M 9", 0):               ("P",  "LP", "P",  "LP",  "P",  "LP",  "P",   "LP"),
    ("M 9", 1):               ("8",  "8",  "8",  "8",   "8",  "8",   "8",   "8"),
    ("one CFG row", 0):       ("P",  "LP", "VP", "LVP", "XP", "LXP", "VXP", "LVXP"),
    ("one CFG row", 1):       ("8",  "8",  "8V", "8V",  "8X", "8X",  "8VX", "8VX"),
    ("depth 0", 0):           ("",   "L",  "V",  "LV",  "X",  "LX",  "VX",  "LVX"),
    ("depth 0", 1):           ("8",  "8",  "8V", "8V",  "8X", "8X",  "8VX", "8VX"),
}


def grid():
    return [(s, f8) for s in SHAPES for f8 in (0, 1)]


def plan(shape, fp8, mask):
    return _lib.lib().emu_unet_block_plan(fp8, mask, *SHAPES[shape])


def facts(bits):
    assert 0 <= bits < 1 << len(FACTS), bits
    return "".join(c for i, c in enumerate(FACTS) if bits >> i & 1)


def test_grid_is_the_table():
    assert set(grid()) == set(EXPECTED) and all(len(v) == 8 for v in EXPECTED.values())


@pytest.mark.parametrize("shape,fp8", grid())
def test_block_plan_matches_the_documented_rule(shape, fp8):
    _ensure_built()
    assert tuple(facts(plan(shape, fp8, mask)) for mask in range(8)) == EXPECTED[(shape, fp8)]


@pytest.mark.parametrize("shape,fp8", grid())
def test_block_plan_facts_exclude_and_imply(shape, fp8):
    """fp8 excludes the LayerNorm fold and the prefetch (the fp8 GEMM takes neither argument); 8 rows and fewer fuse nothing (gemm()
    refuses any fused epilogue there); the two attention epilogues need whole 64-key groups."""
    _ensure_built()
    M, _, HW, _, _ = SHAPES[shape]
    for mask in range(8):
        f = facts(plan(shape, fp8, mask))
        assert not ("8" in f and ("L" in f or "P" in f)), (mask, f)
        assert M > 8 or f == "", (mask, f)
        assert HW % 64 == 0 or not ("V" in f or "X" in f), (mask, f)
        assert fp8 or "8" not in f, (mask, f)


@pytest.mark.parametrize("args", [(2, 7, 2048, 640, 1024, 64, 2), (0, 8, 2048, 640, 1024, 64, 2), (0, -1, 2048, 640, 1024, 64, 2),
                                  (0, 7, 0, 640, 1024, 64, 2), (0, 7, 1000, 640, 1024, 64, 2), (0, 7, 2048, 0, 1024, 64, 2),
                                  (0, 7, 2048, 640, 0, 64, 2), (0, 7, 2048, 640, 1024, 0, 2), (0, 7, 2048, 640, 1024, 64, -1)])
def test_block_plan_refuses_nonsense(args):
    _ensure_built()
    assert _lib.lib().emu_unet_block_plan(*args) == -22
