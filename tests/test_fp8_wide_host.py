"""CPU: the host side of the few-row fp8 weight stream (csrc/gemv_fp8_thin.hip, ``LlamaEngine.use_fp8(True, wide=True)``): the rule
that picks a projection's kernel in the new fp8 modes 3 and 4 (emu_llama_weight_kernel), the launch plan of the kernel for the five
LLaMA-33B projections (emu_gemv_fp8_thin_plan), the symbols, and the argument checks of ``ops.linear_fp8w_thin``, which raise
before any library call.  The expected tables are written out by hand from include/emu_hip.h, not computed.  No GPU, no HIP call."""
import ctypes as C
import re

import pytest
import torch

from emu_amd import _lib, ops
from tests.test_capi_symbols import _ensure_built
from tests.test_llama_weight_kernel import ROWS, WIDTHS

BF16 = torch.bfloat16
_, R8, G8, T8 = 0, 1, 2, 7                       # bf16, the 1..2-row fp8 stream, W8A8 GEMMs, the few-row fp8 stream (include/emu_hip.h)
assert ROWS == (1, 2, 3, 8, 9, 16, 17, 770)
NEW_MODES = {
    #                        1   2   3   8   9   16  17  770
    ("33b", 3):             (R8, R8, T8, T8, T8, T8, _,  _),
    ("33b", 4):             (R8, R8, T8, T8, T8, T8, G8, G8),
    ("1024/2048", 3):       (R8, R8, T8, T8, T8, T8, _,  _),
    ("1024/2048", 4):       (R8, R8, T8, T8, T8, T8, G8, G8),
    ("33b tp8 shard", 3):   (R8, R8, _,  _,  _,  _,  _,  _),
    ("33b tp8 shard", 4):   (R8, R8, _,  _,  _,  _,  _,  _),
}
OLD_MODES = {
    ("33b", 0, 0):            (_,  _,  _,  _,  _,  _,  _,  _),
    ("33b", 1, 0):            (R8, R8, _,  _,  _,  _,  _,  _),
    ("33b", 2, 0):            (R8, R8, _,  _,  _,  _,  G8, G8),
    ("33b", 0, 2):            (3,  3,  4,  4,  4,  4,  _,  _),
    ("33b", 0, 3):            (3,  3,  4,  4,  4,  4,  5,  5),
    ("33b tp8 shard", 2, 0):  (R8, R8, _,  _,  _,  _,  _,  _),
    ("1024/2048", 1, 0):      (R8, R8, _,  _,  _,  _,  _,  _),
    ("1024/2048", 2, 0):      (R8, R8, _,  _,  _,  _,  G8, G8),
}


def kernel(w, f8, f4, rows):
    return _lib.lib().emu_llama_weight_kernel(f8, f4, rows, *WIDTHS[w])


@pytest.mark.parametrize("w,f8", sorted(NEW_MODES))
def test_weight_kernel_fp8_modes_3_and_4(w, f8):
    _ensure_built()
    assert tuple(kernel(w, f8, 0, r) for r in ROWS) == NEW_MODES[(w, f8)]


@pytest.mark.parametrize("w,f8,f4", sorted(OLD_MODES))
def test_weight_kernel_old_modes_keep_their_answers(w, f8, f4):
    _ensure_built()
    assert tuple(kernel(w, f8, f4, r) for r in ROWS) == OLD_MODES[(w, f8, f4)]


def test_few_row_fp8_stream_needs_every_width_in_whole_stages():
    """One width that is no multiple of 256 is enough to keep 3..16 rows on bf16 (the setter refuses such a model)."""
    _ensure_built()
    l = _lib.lib()
    for widths in ((6656, 6656, 17920), (1024, 256, 512)):
        assert l.emu_llama_weight_kernel(3, 0, 5, *widths) == T8
    for widths in ((6656 + 128, 6656, 17920), (6656, 6656 - 128, 17920), (6656, 6656, 17920 + 128), (6656, 3328 + 128, 8960)):
        assert l.emu_llama_weight_kernel(3, 0, 5, *widths) == _
        assert l.emu_llama_weight_kernel(4, 0, 16, *widths) == _
    assert l.emu_llama_weight_kernel(3, 0, 5, 6656, 3328, 8960) == T8          # the TP = 2 shard of the 33B shape


# ---------------------------------------------------------------------------------------------------- the launch plan
def plan(M, N, K, ldx=None, ldw=None, epi=ops.EPI_NONE, tune=0):
    _ensure_built()
    p = _lib.GemvFp8ThinPlanC()
    st = _lib.lib().emu_gemv_fp8_thin_plan(M, N, K, K if ldx is None else ldx, K if ldw is None else ldw, epi, tune, C.byref(p))
    assert st == p.status
    return p


H, F, V = 6656, 17920, 32274
#                 N        K   grid at 32 rows per workgroup
PROJECTIONS = {
    "qkv":     (3 * H,     H,  624),
    "o":       (H,         H,  208),
    "gate/up": (2 * F,     H,  1120),
    "down":    (H,         F,  208),
    "head":    (V,         H,  1009),
}
#      M: (activation-row bucket, stages)
BUCKETS = {3: (8, 4), 5: (8, 4), 8: (8, 4), 9: (16, 3), 16: (16, 3)}


@pytest.mark.parametrize("name", sorted(PROJECTIONS))
@pytest.mark.parametrize("M", sorted(BUCKETS))
def test_plan_of_the_33b_projections(name, M):
    N, K, grid = PROJECTIONS[name]
    mb, stages = BUCKETS[M]
    p = plan(M, N, K, epi=ops.EPI_SWIGLU if name == "gate/up" else ops.EPI_RESID if name in ("o", "down") else ops.EPI_NONE)
    assert (p.status, p.rows, p.mb, p.kc, p.stages, p.grid, p.block) == (0, 32, mb, 256, stages, grid, 256)
    assert p.grid * p.rows >= N > (p.grid - 1) * p.rows                        # the grid covers N, no workgroup without a row
    assert p.lds_bytes == p.stages * (p.rows * 256 + p.mb * 512) == 49152      # three workgroups share a CU's 160 KiB


def test_plan_small_n_and_pinned_rows():
    for N in (16, 37, 64, 1000, 4064):                                         # fewer than 128 workgroups of 32 rows: 16 rows
        p = plan(5, N, 512)
        assert (p.status, p.rows, p.mb, p.stages, p.grid) == (0, 16, 8, 6, (N + 15) // 16)
    assert plan(5, 4065, 512).rows == 32
    assert (plan(16, 64, 512).rows, plan(16, 64, 512).mb, plan(16, 64, 512).stages) == (16, 16, 4)
    p = plan(16, 64, 512, tune=2 << 28)                                        # emu_gemm_tune bits 28-29: 1 / 2 = 16 / 32 rows
    assert (p.rows, p.mb, p.stages, p.grid) == (32, 16, 3, 2)
    p = plan(5, 3 * H, H, tune=1 << 28)
    assert (p.rows, p.mb, p.stages, p.grid) == (16, 8, 6, 1248)
    for M in (1, 2):                                                           # the kernel takes them, the engine does not send them
        assert (plan(M, 64, 256).status, plan(M, 64, 256).mb) == (0, 8)


@pytest.mark.parametrize("kw", [dict(M=5, N=64, K=384), dict(M=5, N=64, K=128), dict(M=5, N=64, K=896), dict(M=17, N=64, K=256),
                                dict(M=0, N=64, K=256), dict(M=5, N=0, K=256), dict(M=5, N=64, K=256, ldw=264),
                                dict(M=5, N=64, K=256, ldx=260), dict(M=5, N=64, K=512, ldw=256), dict(M=5, N=63, K=256, epi=ops.EPI_SWIGLU),
                                dict(M=5, N=64, K=256, epi=ops.EPI_GELU)])
def test_no_plan_outside_the_kernels_range(kw):
    p = plan(**kw)
    assert p.status == -22
    assert (p.rows, p.mb, p.kc, p.stages, p.lds_bytes, p.grid, p.block) == (0,) * 7


# ---------------------------------------------------------------------------------------------------- ABI
def test_symbols_prototypes_and_version():
    _ensure_built()
    protos = next(v for v in vars(_lib).values() if isinstance(v, dict) and "emu_version" in v)
    declared = _lib.declared_symbols()
    for name in ("emu_linear_fp8w_thin_bf16", "emu_gemv_fp8_thin_plan"):
        assert name in declared and name in protos and hasattr(_lib.lib(), name)
    assert len(protos["emu_linear_fp8w_thin_bf16"][1]) == 15
    assert _lib.lib().emu_version() == _lib.ABI_VERSION
    hdr = open(_lib.HEADER_PATH).read()
    assert re.search(r"emu_llama_use_fp8\(m, 3\) is mode 1 and \(m, 4\) is mode 2 plus", hdr)


# ---------------------------------------------------------------------------------------------------- ops.linear_fp8w_thin
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} during argument checking")


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(ops, "lib", lambda: _NoLibrary())


def _args(M=5, N=64, K=256, **kw):
    a = dict(x=torch.zeros(M, K, dtype=BF16), w8=torch.zeros(N, K, dtype=torch.uint8), wscale=torch.ones(N))
    a.update(kw)
    return a


@pytest.mark.parametrize("kw,msg", [
    (_args(K=384), "multiple of 256"),
    (_args(K=128), "multiple of 256"),
    (_args(M=17), "1..16 rows"),
    (_args(M=0), "1..16 rows"),
    (_args(w8=torch.zeros(64, 264, dtype=torch.uint8)[:, :256]), "16-byte"),
    (_args(x=torch.zeros(5, 260, dtype=BF16)[:, :256]), "16-byte"),
    (_args(x=torch.zeros(5, 256)), "x must be torch.bfloat16"),
    (_args(w8=torch.zeros(64, 256, dtype=torch.int8)), "w8 must be torch.uint8"),
    (_args(wscale=torch.ones(63)), "wscale"),
    (_args(wscale=torch.ones(64, dtype=torch.float64)), "wscale must be torch.float32"),
    (_args(w8=torch.zeros(64, 512, dtype=torch.uint8)), "agree in K"),
    (_args(N=63, epi=ops.EPI_SWIGLU), "even N"),
    (_args(epi=ops.EPI_GELU), "epi"),
    (_args(epi=ops.EPI_RESID), "res"),
    (_args(epi=ops.EPI_RESID, res=torch.zeros(5, 32, dtype=BF16)), "res"),
    (_args(bias=torch.zeros(32, dtype=BF16)), "bias"),
    (_args(out=torch.zeros(5, 32, dtype=BF16)), "out"),
    (_args(x=None), "x must be a tensor"),
    (_args(), "GPU tensor"),                                                  # everything else in order: only then the device
])
def test_linear_fp8w_thin_argument_errors_come_before_any_library_call(no_library, kw, msg):
    with pytest.raises(ValueError, match=re.escape(msg)):
        ops.linear_fp8w_thin(**kw)
