"""CPU: the composed rule that picks the kernel of ONE LLaMA projection (emu_llama_projection_kernel: engine.hip's call_kernel and
matrix_kernel, the functions LlamaCall::project and llama_head ask) -- integers only, no GPU, no HIP call.  (a) the head site against
a table written out by hand from include/emu_hip.h, (b) agreement with the three older hooks wherever those can be asked, (c) a kernel
the older hooks refuse passes through, (d) the refusals."""
import ctypes as C

import pytest

from emu_amd import _lib
from tests.test_bf16_pack_rule import HEADLINE, VOCAB
from tests.test_capi_symbols import _ensure_built
from tests.test_llama_weight_kernel import ROWS as CALL_ROWS, WIDTHS, grid
from tests.test_pack_thin_plan import PROJ, ROWS as THIN_ROWS

W33 = (6656, 6656, 17920)               # hidden, heads_local * head_dim, ffn_local: all multiples of 256


@pytest.fixture(scope="module")
def L():
    _ensure_built()
    return _lib.lib()


def ask(L, fp8=0, fp4=0, rows=1, widths=W33, N=VOCAB, K=6656, **facts):
    """(kernel, norm in the stream); facts: the other fields of emu_projection, 0 unless given."""
    q = _lib.ProjectionC(fp8=fp8, fp4=fp4, rows=rows, hidden=widths[0], heads_dim_local=widths[1], ffn_local=widths[2], N=N, K=K, **facts)
    k = L.emu_llama_projection_kernel(C.byref(q))
    return k, q.norm_in_stream


# ------------------------------------------------------------------------------------------------------------------ (a) the head
HEAD_ROWS = (1, 2, 5, 8, 9, 16, 20)
# (fp8 mode, fp4 mode) -> (workspace fits, fp8 copy) -> the cells at HEAD_ROWS with the pack stream off, and on (the head has a set of
# 4 rows per group, the head form's; the wide switch off).  A cell: the kernel, then n = the norm rides in the stream, - = it is a
# launch of its own.  The head: no W8A8 GEMM (2 -> 0); 1, 7, 9 need the fp8 copy (else 0); 7 and 4 need the workspace (else 0); 1 and 3
# fuse the norm, 0 at one row and, without the workspace, up to 8 rows; 0 at one row -> 6 under the pack stream.
BF16_FITS = ("0n 0- 0- 0- 0- 0- 0-", "6n 0- 0- 0- 0- 0- 0-")
BF16_NO_WS = ("0n 0n 0n 0n 0- 0- 0-", "6n 0n 0n 0n 0- 0- 0-")
AS_BF16 = {(1, 0): BF16_FITS, (0, 0): BF16_NO_WS}                 # a mode without its fp8 copy
FP8_ROWS_ONLY = {(1, 1): ("1n 1n 0- 0- 0- 0- 0-",) * 2, (0, 1): ("1n 1n 0n 0n 0- 0- 0-",) * 2, **AS_BF16}
HEAD = {
    (0, 0): {(1, 1): BF16_FITS, (0, 1): BF16_NO_WS, **AS_BF16},
    (1, 0): FP8_ROWS_ONLY,
    (2, 0): FP8_ROWS_ONLY,
    (3, 0): {(1, 1): ("1n 1n 7- 7- 7- 7- 0-",) * 2, (0, 1): ("1n 1n 0n 0n 0- 0- 0-",) * 2, **AS_BF16},
    (5, 0): {(1, 1): ("1n 1n 7- 7- 7- 7- 9-",) * 2, (0, 1): ("1n 1n 0n 0n 0- 0- 9-",) * 2, **AS_BF16},
    (0, 1): {(1, 1): ("3n 3n 0- 0- 0- 0- 0-",) * 2, (0, 1): ("3n 3n 0n 0n 0- 0- 0-",) * 2,
             (1, 0): ("3n 3n 0- 0- 0- 0- 0-",) * 2, (0, 0): ("3n 3n 0n 0n 0- 0- 0-",) * 2},
    (0, 2): {(1, 1): ("3n 3n 4- 4- 4- 4- 0-",) * 2, (0, 1): ("3n 3n 0n 0n 0- 0- 0-",) * 2,
             (1, 0): ("3n 3n 4- 4- 4- 4- 0-",) * 2, (0, 0): ("3n 3n 0n 0n 0- 0- 0-",) * 2},
    (0, 3): {(1, 1): ("3n 3n 4- 4- 4- 4- 5-",) * 2, (0, 1): ("3n 3n 0n 0n 0- 0- 5-",) * 2,
             (1, 0): ("3n 3n 4- 4- 4- 4- 5-",) * 2, (0, 0): ("3n 3n 0n 0n 0- 0- 5-",) * 2},
}
# after release_bf16 there is no bf16 to fall back to: the MXFP4 few-row stream stays whatever the workspace; every other cell as above
RELEASED = {
    (0, 2): {(0, 1): ("3n 3n 4- 4- 4- 4- 0-",) * 2, (0, 0): ("3n 3n 4- 4- 4- 4- 0-",) * 2},
    (0, 3): {(0, 1): ("3n 3n 4- 4- 4- 4- 5-",) * 2, (0, 0): ("3n 3n 4- 4- 4- 4- 5-",) * 2},
}


@pytest.mark.parametrize("released", [0, 1])
@pytest.mark.parametrize("mode", sorted(HEAD))
def test_head_site_matches_the_table(L, mode, released):
    assert L.emu_bf16_pack_rows(VOCAB, 6656, 1, 0, 0) == 4
    for (ws_fits, has_fp8), cells in HEAD[mode].items():
        if released:
            cells = RELEASED.get(mode, {}).get((ws_fits, has_fp8), cells)
        for pack, want in zip((0, 1), cells):
            got = [ask(L, *mode, rows=r, head=1, ws_fits=ws_fits, has_fp8=has_fp8, bf16_released=released, pack=pack, pack_rows=4,
                       set_n=VOCAB, set_k=6656) for r in HEAD_ROWS]
            assert " ".join(f"{k}{'n' if n else '-'}" for k, n in got) == want, (mode, ws_fits, has_fp8, released, pack)


def test_head_site_inhibitors_and_the_wide_switch(L):
    head = dict(head=1, ws_fits=1, pack=1, pack_rows=4, set_n=VOCAB, set_k=6656)
    for inhibitor in (dict(fused_mode=1), dict(tail_mode=1), dict(warm_mask=1)):
        assert ask(L, **head, **inhibitor) == (0, 1)
    assert ask(L, **dict(head, set_n=VOCAB - 1)) == (0, 1)                    # a set of other rows of the vocabulary (a shard)
    assert ask(L, rows=5, **head) == (0, 0) and ask(L, rows=5, pack_wide=1, **head) == (8, 0)
    assert ask(L, rows=5, pack_wide=1, **dict(head, ws_fits=0)) == (0, 1)     # the norm rides in the bf16 stream: no packed twin


# ------------------------------------------------------------------------------------------------------------------ (b) the old hooks
@pytest.mark.parametrize("w,f8,f4", grid())
def test_call_level_view_is_the_weight_kernel_hook(L, w, f8, f4):
    for rows in CALL_ROWS:                                              # (a layer matrix with an fp8 copy, no pack: the identity)
        k, n = ask(L, f8, f4, rows, WIDTHS[w], N=6656, K=6656, has_fp8=1)
        assert k == L.emu_llama_weight_kernel(f8, f4, rows, *WIDTHS[w]) and n == 0


@pytest.mark.parametrize("name", list(HEADLINE))
def test_one_row_pack_answers_are_the_pack_hook(L, name):
    N, K, norm, epi, pr = HEADLINE[name]
    for rows, pack_rows, on, inhibit in [(1, pr, 1, (0, 0, 0)), (1, 6 - pr, 1, (0, 0, 0)), (1, 0, 1, (0, 0, 0)), (1, pr, 0, (0, 0, 0)),
                                         (1, pr, 1, (2, 0, 0)), (1, pr, 1, (0, 1, 0)), (1, pr, 1, (0, 0, 0x1020)), (2, pr, 1, (0, 0, 0)),
                                         (5, pr, 1, (0, 0, 0)), (17, pr, 1, (0, 0, 0))]:
        want = L.emu_llama_pack_kernel(0, rows, pack_rows, on, *inhibit, N, K, norm, epi, 0)
        got = ask(L, rows=rows, N=N, K=K, norm=norm, epi=epi, pack=on, pack_rows=pack_rows, set_n=N, set_k=K, fused_mode=inhibit[0],
                  tail_mode=inhibit[1], warm_mask=inhibit[2])
        assert got == (want, norm), (name, rows, pack_rows, on, inhibit)
    assert ask(L, N=N, K=K, norm=norm, epi=epi, pack=1, pack_rows=pr, set_n=N, set_k=K)[0] == 6


@pytest.mark.parametrize("rows", THIN_ROWS)
def test_few_row_pack_answers_are_the_pack_thin_hook(L, rows):
    for name, N, K, epi in PROJ:
        for pack_rows, set_n, on, wide, norm in [(2, N, 1, 1, 0), (4, N, 1, 1, 0), (0, N, 1, 1, 0), (4, N - 8, 1, 1, 0), (4, N, 0, 1, 0),
                                                 (4, N, 1, 0, 0), (4, N, 1, 1, 1)]:
            want = L.emu_llama_pack_thin_kernel(0, rows, pack_rows, set_n, K, on, wide, N, K, norm, epi, 0)
            got = ask(L, rows=rows, N=N, K=K, norm=norm, epi=epi, pack=on, pack_wide=wide, pack_rows=pack_rows, set_n=set_n, set_k=K)
            assert got == (want, norm), (name, rows, pack_rows, set_n, on, wide, norm)
        assert ask(L, rows=rows, N=N, K=K, epi=epi, pack=1, pack_wide=1, pack_rows=4, set_n=N, set_k=K)[0] == 8


# ------------------------------------------------------------------------------------------------------------------ (c), (d)
def test_the_fp8_gemm_of_17_to_64_rows_passes_through(L):
    """fp8 mode 5 at 20 rows is kernel 9, which the two older pack hooks refuse (-22) and the engine passes through."""
    assert L.emu_llama_weight_kernel(5, 0, 20, *W33) == 9
    assert L.emu_llama_pack_kernel(9, 20, 2, 1, 0, 0, 0, 6656, 6656, 0, 1, 0) == -22
    assert L.emu_llama_pack_thin_kernel(9, 20, 2, 6656, 6656, 1, 1, 6656, 6656, 0, 1, 0) == -22
    assert ask(L, 5, 0, 20, N=6656, K=6656, epi=1, has_fp8=1, pack=1, pack_wide=1, pack_rows=2, set_n=6656, set_k=6656) == (9, 0)


def test_null_and_out_of_range_records(L):
    assert L.emu_llama_projection_kernel(None) == -22
    assert ask(L)[0] == 0
    for bad in (dict(fp8=-1), dict(fp8=7), dict(fp4=-1), dict(fp4=4), dict(fp8=1, fp4=1), dict(rows=0), dict(widths=(0, 6656, 17920)),
                dict(widths=(6656, 0, 17920)), dict(widths=(6656, 6656, 0)), dict(N=0), dict(K=0), dict(pack_rows=-1), dict(warm_mask=-1)):
        assert ask(L, **bad)[0] == -22, bad
