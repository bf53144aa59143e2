"""CPU: the one further rule that sends a bf16 projection to the 13-bit packed stream (emu_llama_pack_kernel: engine.hip's
pack_kernel, asked by every layer projection and by the head; integers only, no GPU, no HIP call), against a literal table written
from include/emu_hip.h: the packed kernel (6) only for ONE row on the bf16 kernel, with the switch on, a registered set of the planned
form's rows per group, and no fused-layer / decode-tail / L2-warm mode; everything else keeps the kernel it had."""
import pytest

from emu_amd import _lib
from tests.test_capi_symbols import _ensure_built

BF16, FP8_ROWS, FP8_GEMM, FP4_ROWS, FP4_THIN, FP4_GEMM, BF16_PACK = range(7)
EPI_NONE, EPI_RESID, EPI_SWIGLU = 0, 1, 2
VOCAB = 32274
# name -> (N, K, norm, epi, rows per group of the set): the four launches of the headline decode step and its head
HEADLINE = {
    "qkv": (19968, 6656, 1, EPI_NONE, 4),          # head form
    "lm_head": (VOCAB, 6656, 1, EPI_NONE, 4),      # head form
    "gate/up": (35840, 6656, 1, EPI_SWIGLU, 4),    # head form, SwiGLU epilogue
    "o_proj": (6656, 6656, 0, EPI_RESID, 2),       # preload form
    "down": (6656, 17920, 0, EPI_RESID, 2),        # single round trip
}
# shapes the planner sends to a family without a packed twin: the wave form of the TP = 8 shards, small matrices (single round trip
# of 4 rows x 4 trips), K % 32 != 0
NO_TWIN = {
    "tp8 o_proj": (6656, 896, 0, EPI_RESID),
    "tp8 down": (6656, 2240, 0, EPI_RESID),
    "tiny qkv": (768, 256, 1, EPI_NONE),
    "tiny down": (256, 512, 0, EPI_RESID),
    "K % 32": (6656, 6664, 0, EPI_RESID),
}


@pytest.fixture(scope="module")
def L():
    _ensure_built()
    return _lib.lib()


def rule(L, kernel=BF16, rows=1, pack_rows=4, on=1, fused=0, tail=0, warm=0, N=19968, K=6656, norm=1, epi=EPI_NONE, tune=0):
    return L.emu_llama_pack_kernel(kernel, rows, pack_rows, on, fused, tail, warm, N, K, norm, epi, tune)


@pytest.mark.parametrize("name", list(HEADLINE))
def test_headline_shapes_take_the_packed_kernel(L, name):
    N, K, norm, epi, pr = HEADLINE[name]
    assert L.emu_bf16_pack_rows(N, K, norm, epi, 0) == pr
    assert rule(L, pack_rows=pr, N=N, K=K, norm=norm, epi=epi) == BF16_PACK
    assert rule(L, pack_rows=6 - pr, N=N, K=K, norm=norm, epi=epi) == BF16          # a set laid out for another form
    assert rule(L, pack_rows=0, N=N, K=K, norm=norm, epi=epi) == BF16               # no set registered
    assert rule(L, pack_rows=pr, on=0, N=N, K=K, norm=norm, epi=epi) == BF16        # switched off


@pytest.mark.parametrize("rows", [2, 3, 5, 8, 16, 17, 770])
@pytest.mark.parametrize("name", list(HEADLINE))
def test_every_other_row_count_is_bf16(L, name, rows):
    N, K, norm, epi, pr = HEADLINE[name]
    assert rule(L, rows=rows, pack_rows=pr, N=N, K=K, norm=norm, epi=epi) == BF16


@pytest.mark.parametrize("mode", [dict(fused=1), dict(fused=2), dict(fused=3), dict(fused=4), dict(tail=1), dict(warm=1), dict(warm=0x1f),
                                  dict(warm=0x1020)])
@pytest.mark.parametrize("name", list(HEADLINE))
def test_fused_tail_and_warm_modes_keep_bf16(L, name, mode):
    N, K, norm, epi, pr = HEADLINE[name]
    assert rule(L, pack_rows=pr, N=N, K=K, norm=norm, epi=epi, **mode) == BF16


@pytest.mark.parametrize("kernel", [FP8_ROWS, FP8_GEMM, FP4_ROWS, FP4_THIN, FP4_GEMM])
def test_fp8_and_fp4_kernels_pass_through(L, kernel):
    for N, K, norm, epi, pr in HEADLINE.values():
        assert rule(L, kernel=kernel, pack_rows=pr, N=N, K=K, norm=norm, epi=epi) == kernel
    assert L.emu_llama_weight_kernel(1, 0, 1, 6656, 6656, 17920) == FP8_ROWS and L.emu_llama_weight_kernel(0, 1, 1, 6656, 6656, 17920) == FP4_ROWS


@pytest.mark.parametrize("name", list(NO_TWIN))
def test_other_families_stay_bf16(L, name):
    N, K, norm, epi = NO_TWIN[name]
    assert L.emu_bf16_pack_rows(N, K, norm, epi, 0) == 0
    for pr in (2, 4):
        assert rule(L, pack_rows=pr, N=N, K=K, norm=norm, epi=epi) == BF16


def test_block_only_tune_reaches_the_preload_form_on_small_matrices(L):
    # emu_gemm_tune bit 17 (tests: no wave / single-round-trip form): a small plain matrix takes the preload form of two rows
    assert L.emu_bf16_pack_rows(256, 512, 0, EPI_RESID, 1 << 17) == 2
    assert rule(L, pack_rows=2, N=256, K=512, norm=0, epi=EPI_RESID, tune=1 << 17) == BF16_PACK
    assert rule(L, pack_rows=2, N=256, K=512, norm=0, epi=EPI_RESID, tune=0) == BF16
