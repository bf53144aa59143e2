"""CPU: the 12-bit twin of the packed few-row stream as far as integers and refusals go -- no device, no HIP call.
emu_linear_bf16pack12_thin refuses (-22) on its argument checks, the planner's and the launcher's pointer checks, all of which run
before anything is launched, so the pointers here are made-up addresses that nothing dereferences.  The matrix-level rule treats
switch value 2 as it treats 1 (what value 2 changes is the pack_rows the engine feeds it, which only a model can show)."""
import ctypes as C
import os
import re

import pytest

from emu_amd import _lib
from emu_amd._lib import Bf16Pack12SetC
from tests.test_capi_symbols import _ensure_built
from tests.test_pack_thin_plan import BF16, BF16_PACK_THIN, NONE, PROJ, RESID, ROWS, rule

A, W, OUT, LO, NIB, PATCH, FLAGS = (0x10000 * (i + 1) for i in range(7))      # 16-byte aligned, never read on the host


@pytest.fixture(scope="module")
def L():
    _ensure_built()
    return _lib.lib()


def call(L, M=5, N=264, K=768, epi=NONE, lo=LO, nib=NIB, patch=PATCH, flags=FLAGS, hb=56, rows=4, a=A, w=W, out=OUT, null_set=False):
    s = Bf16Pack12SetC(lo, nib, patch, flags, hb, rows)
    return L.emu_linear_bf16pack12_thin(a, w, None if null_set else C.byref(s), None, out, M, N, K, epi, None)


def test_symbol_is_exported_and_declared(L):
    assert hasattr(L, "emu_linear_bf16pack12_thin") and "emu_linear_bf16pack12_thin" in _lib._PROTOS
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "emu_hip.h")).read()
    assert re.search(r"^int emu_linear_bf16pack12_thin\(const void\* A, const void\* W, const emu_bf16_pack12_set\* set,", header, re.M)


REFUSALS = {
    "null set": dict(null_set=True), "no patch pointer": dict(patch=None), "no low plane": dict(lo=None), "no flags": dict(flags=None),
    "null A": dict(a=None), "null W": dict(w=None), "null C": dict(out=None),
    "R 0": dict(rows=0), "R 1": dict(rows=1), "R 3": dict(rows=3), "R 8": dict(rows=8),
    "M 1": dict(M=1), "M 3": dict(M=3), "M 17": dict(M=17),
    "K 128": dict(K=128), "K 260": dict(K=260), "K 896": dict(K=896),
    "hb 121": dict(hb=121), "hb -1": dict(hb=-1),
    "low plane off 16 bytes": dict(lo=LO + 8), "nibbles off 16 bytes": dict(nib=NIB + 4), "records off 16 bytes": dict(patch=PATCH + 4),
    "x off 16 bytes": dict(a=A + 2), "W off 16 bytes": dict(w=W + 2),
    "RESID without res": dict(epi=RESID),
}


@pytest.mark.parametrize("why", sorted(REFUSALS))
def test_refusals_before_any_launch(L, why):
    assert call(L, **REFUSALS[why]) == -22, why


def test_k_bound_keeps_vi_clear_of_the_empty_slot(L):
    """K / 8 must stay below 2^18 (PACK12_MAX_KV): an empty slot's vector index is the largest a slot can hold.  The planner takes
    the shape (asserted), and every other argument is the accepted base call's, so the bound is what refuses."""
    from tests.test_gemv_plan import PlanC, ShapeC, shape
    K = 8 << 18
    for k in (K, K - 256):                                # at the bound and the last K below it: the plan is not what tells them apart
        out = PlanC()
        assert L.emu_gemv_pack_thin_plan(C.byref(ShapeC(*shape(5, 264, k, NONE))), 4, 0, C.byref(out)) == 0 and (out.status, out.kch) == (0, 32)
    assert call(L, N=264, K=K) == -22


@pytest.mark.parametrize("rows", ROWS)
def test_rule_answers_for_switch_value_2_as_for_1(L, rows):
    for name, N, K, epi in PROJ:
        for pr in (2, 4):
            assert rule(L, rows=rows, pack_rows=pr, N=N, K=K, epi=epi, wide=2) == rule(L, rows=rows, pack_rows=pr, N=N, K=K, epi=epi, wide=1) \
                == BF16_PACK_THIN, name
        kw = dict(N=N, K=K, epi=epi, rows=rows, wide=2)
        assert rule(L, on=0, **kw) == BF16 and rule(L, pack_rows=0, **kw) == BF16 and rule(L, norm=1, **kw) == BF16
        assert rule(L, set_n=N - 8, **kw) == BF16 and rule(L, set_k=K - 256, **kw) == BF16 and rule(L, tune=4, **kw) == BF16
    for r in (1, 2, 3, 17, 770):
        assert rule(L, rows=r, wide=2) == rule(L, rows=r, wide=1) == BF16
