"""CPU: the L2-warming plan (csrc/l2_warm.h) through emu_l2_warm_plan_make / emu_l2_warm_enumerate -- the enumerator calls the very
function (warm_line) the kernels' touch loop calls, so what is checked here is the arithmetic the GPU runs.

For every plan: the union of the lines over all toucher workgroups has no duplicate; every line lies wholly inside the successor
array (or its twin); the total stays within the budget; the toucher's linear workgroup id and the reader's are congruent modulo 8
(the reader is recovered from the line's address by the successor's own geometry, not by the plan's arithmetic); workgroups outside
[first, first + ntouch) request nothing; the plan is empty where it must be.  And the successor geometry (emu_gemv_geometry, which
launch_gemv dispatches on) agrees with the block kernels' rows-per-workgroup heuristic and the column partition on these shapes."""
import ctypes as C

import pytest

from emu_amd import _lib
from emu_amd._lib import WarmPlanC
from tests.test_capi_symbols import _ensure_built

MIB = 1 << 20
BASE = 0x7F0000000000                         # a line-aligned address: nothing is dereferenced on the host
EPI_NONE, EPI_RESID, EPI_SWIGLU = 0, 1, 2
ROLLING, HEAD, PRELOAD, RT, WAVE = range(5)
# LLaMA-33B: hidden 6656, 52 heads x 128, ffn 17920, vocabulary 32274 (+ the image tokens: bench.py's VOCAB_EMU2_CHAT)
H33, F33, V33 = 6656, 17920, 32274


def _l():
    _ensure_built()
    return _lib.lib()


def geometry(N, K, norm, epi):
    out = (C.c_int * 4)()
    assert _l().emu_gemv_geometry_query(N, K, int(norm), epi, out) == 0
    return tuple(out)                         # form, rows, rows_per_block heuristic, partition


def make(base, twin, rows, row_bytes, used, nrows, gx, groups, pred_wgs, extra, lanes, budget, shape):
    p = WarmPlanC()
    assert _l().emu_l2_warm_plan_make(base, twin, rows, row_bytes, used, nrows, gx, groups, pred_wgs, int(extra), lanes, budget, shape,
                                      C.byref(p)) == 0
    return p


def lines_of(p, wg):
    n = _l().emu_l2_warm_enumerate(C.byref(p), wg, None, 0)
    buf = (C.c_longlong * max(n, 1))()
    assert _l().emu_l2_warm_enumerate(C.byref(p), wg, buf, n) == n
    return list(buf[:n])


def gemv_plan(pred, succ, budget=16 * MIB, shape=0, ldw=None):
    """pred / succ = (N, K, norm, epi) of two one-row streams that follow each other; the successor's rows are ldw elements apart."""
    pf, pr, _, _ = geometry(*pred)
    sf, sr, _, _ = geometry(*succ)
    assert pf in (HEAD, PRELOAD, RT)
    N, K = succ[0], succ[1]
    ldw = ldw or K
    p = make(BASE, 0, sr, ldw * 2, K * 2, N, 0, 1, -(-pred[0] // pr), False, 256, budget, shape)
    return p, dict(N=N, K=K, ldw=ldw, R=sr, pred_wgs=-(-pred[0] // pr))


def check_flat(p, g, budget, want_empty=False):
    """The invariants of a plan against a flat [N, ldw] successor read R rows per workgroup."""
    if want_empty:
        assert p.ntouch == 0
        for wg in (0, 1, 7, g["pred_wgs"] - 1):
            assert lines_of(p, wg) == []
        return 0
    assert p.ntouch > 0 and p.xcds == 8
    row_bytes, size = g["ldw"] * 2, g["N"] * g["ldw"] * 2
    seen = set()
    for wg in range(p.first, p.first + p.ntouch):
        for off in lines_of(p, wg):
            assert off % 128 == 0 and 0 <= off and off + 128 <= size, (wg, off)
            assert off not in seen, (wg, off)
            seen.add(off)
            row = off // row_bytes                           # the row the line starts in, hence the workgroup that reads it first
            assert off - row * row_bytes < g["K"] * 2
            assert (row // g["R"]) % 8 == wg % 8, (wg, off, row)
            assert row // g["R"] < p.nsucc
    assert 0 < len(seen) * 128 <= budget
    for wg in (0, p.first - 1, p.first + p.ntouch, p.first + p.ntouch + 5):
        if wg < p.first or wg >= p.first + p.ntouch:
            assert lines_of(p, wg) == []
    return len(seen)


QKV = (3 * H33, H33, True, EPI_NONE)
OPROJ = (H33, H33, False, EPI_RESID)
GATEUP = (2 * F33, H33, True, EPI_SWIGLU)
DOWN = (H33, F33, False, EPI_RESID)
LMHEAD = (V33, H33, True, EPI_NONE)


def test_geometry_of_the_33b_streams_and_agreement_with_the_heuristics():
    assert geometry(*QKV)[:2] == (HEAD, 4)
    assert geometry(*OPROJ)[:2] == (PRELOAD, 2)
    assert geometry(*GATEUP)[:2] == (HEAD, 4)
    assert geometry(*DOWN)[:2] == (RT, 2)
    assert geometry(*LMHEAD)[:2] == (HEAD, 4)
    shapes = [QKV, OPROJ, GATEUP, DOWN, LMHEAD, (40, 6656, True, EPI_NONE), (38, 520, False, EPI_NONE), (38, 17920, False, EPI_NONE),
              (40, 264, False, EPI_NONE), (38, 264, False, EPI_NONE), (6656, 896, False, EPI_RESID), (6656, 2240, False, EPI_RESID),
              (2496, 6656, True, EPI_NONE), (4480, 6656, True, EPI_SWIGLU), (1024, 1024, False, EPI_NONE), (512, 512, True, EPI_NONE)]
    for s in shapes:
        form, rows, heur, part = geometry(*s)
        assert (part == 1) == (form == WAVE), s            # the column partition: one wave per row only in the wave form
        if form in (ROLLING, HEAD, PRELOAD):
            assert rows == heur, s                         # the block kernels own what the heuristic says
        elif form == RT:
            assert rows == (4 if s[1] <= 8192 else 2), s   # 4 rows x 4 trips, 2 rows x 9 trips
        else:
            assert rows == 16, s


@pytest.mark.parametrize("shape", [0, 1])
@pytest.mark.parametrize("pred,succ", [(OPROJ, GATEUP), (GATEUP, DOWN), (DOWN, QKV), (DOWN, LMHEAD)])
def test_33b_stream_boundaries(pred, succ, shape):
    p, g = gemv_plan(pred, succ, shape=shape)
    n = check_flat(p, g, 16 * MIB)
    # the budget is used: whole blocks of 8 workgroups at a time, so at most 8 blocks short of it
    per_block = g["R"] * (-(-min(g["K"] * 2, 4096 if shape else 1 << 30) // 128))
    assert n > 16 * MIB // 128 - 8 * per_block
    assert p.first + p.ntouch == g["pred_wgs"]             # the LAST workgroups of the predecessor


def test_33b_combine_warms_o_proj_from_extra_workgroups():
    _, sr, _, _ = geometry(*OPROJ)
    p = make(BASE, 0, sr, H33 * 2, H33 * 2, H33, 0, 1, 52, True, 128, 16 * MIB, 0)
    assert p.first == 52 and p.ntouch % 8 == 0 and p.lanes == 128
    check_flat(p, dict(N=H33, K=H33, ldw=H33, R=sr, pred_wgs=52), 16 * MIB)


def test_33b_qkv_warms_the_cache_rows_of_a_3d_attention_grid():
    """Reader: decode attention's grid (ns = 7, H = 52, B = 1), linear id = split + 7 * head, 128 slots of 256 bytes per workgroup out
    of K and V caches of S_max slots per head; S_max is no multiple of 128 here, so the last split's block would leave its head."""
    ns, Hh, S_max = 7, 52, 808
    twin = Hh * S_max * 256 + 4096
    pf, pr, _, _ = geometry(*QKV)
    p = make(BASE, twin, 128, 256, 256, S_max, ns, Hh, -(-QKV[0] // pr), False, 256, 24 * MIB, 0)
    assert p.ntouch > 0 and p.gx == ns
    size = Hh * S_max * 256
    seen = set()
    for wg in range(p.first, p.first + p.ntouch):
        for off in lines_of(p, wg):
            arr, o = (1, off - twin) if off >= twin else (0, off)
            assert o % 128 == 0 and 0 <= o and o + 128 <= size, (wg, off)
            assert (arr, o) not in seen
            seen.add((arr, o))
            head, slot = divmod(o // 256, S_max)
            split = slot // 128
            assert split < ns and (split + 1) * 128 <= S_max          # a block that would leave its head is skipped whole
            assert (split + ns * head) % 8 == wg % 8, (wg, off)
    assert 0 < len(seen) * 128 <= 24 * MIB
    assert {a for a, _ in seen} == {0, 1}                             # both caches
    # the covered workgroups' whole splits (6 of a head's 7), K and V, 2 lines per slot; blocks are covered 8 at a time
    assert p.nsucc == ns * Hh - ns * Hh % 8
    assert len(seen) == sum(1 for j in range(p.nsucc) if j % ns < 6) * 128 * 2 * 2


@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("shape", [0, 1])
def test_ragged_pair(R, shape):
    """Predecessor N = 40, successor N = 38, K = 264 at ldw = 264: rows of 528 bytes, so lines straddle rows and blocks, and with
    R = 4 the last block has two rows.  The predecessor's 20 (R = 2) / 10 (R = 4) workgroups stand for any grid of that size."""
    N, K = 38, 264
    p = make(BASE, 0, R, K * 2, K * 2, N, 0, 1, 40 // R, False, 256, 16 * MIB, shape)
    n = check_flat(p, dict(N=N, K=K, ldw=K, R=R, pred_wgs=40 // R), 16 * MIB)
    nblocks = -(-N // R)
    covered = nblocks - nblocks % 8 if nblocks >= 8 else nblocks
    # every line that starts inside a covered block and ends inside the matrix, once
    want = sum(1 for off in range(0, N * K * 2 - 127, 128) if off // (K * 2) // R < covered)
    assert n == want


def test_successor_smaller_than_the_budget_is_covered_whole():
    N, K = 512, 1024                                       # 1 MiB
    p = make(BASE, 0, 2, K * 2, K * 2, N, 0, 1, 3328, False, 256, 16 * MIB, 0)
    assert check_flat(p, dict(N=N, K=K, ldw=K, R=2, pred_wgs=3328), 16 * MIB) == N * K * 2 // 128
    assert p.nsucc == N // 2


def test_successor_with_fewer_than_eight_workgroups():
    N, K = 10, 1024                                        # 5 workgroups of 2 rows: classes 5..7 have nothing to do
    p = make(BASE, 0, 2, K * 2, K * 2, N, 0, 1, 64, False, 256, 16 * MIB, 0)
    assert p.nsucc == 5
    assert check_flat(p, dict(N=N, K=K, ldw=K, R=2, pred_wgs=64), 16 * MIB) == N * K * 2 // 128
    for wg in range(p.first, p.first + p.ntouch):
        if wg % 8 >= 5:
            assert lines_of(p, wg) == []


def test_predecessor_with_fewer_workgroups_than_touchers():
    p16, g = gemv_plan(OPROJ, GATEUP)
    assert p16.ntouch > 16
    sr = g["R"]
    p = make(BASE, 0, sr, H33 * 2, H33 * 2, 2 * F33, 0, 1, 16, False, 256, 16 * MIB, 0)
    assert p.first == 0 and p.ntouch == 16                  # all 16 touch, in more trips
    a = check_flat(p, dict(N=2 * F33, K=H33, ldw=H33, R=sr, pred_wgs=16), 16 * MIB)
    b = check_flat(p16, g, 16 * MIB)
    assert a == b


def test_empty_plans():
    ok = dict(base=BASE, twin=0, rows=4, row_bytes=2048, used=2048, nrows=4096, gx=0, groups=1, pred_wgs=64, extra=False, lanes=256,
              budget=16 * MIB, shape=0)
    assert make(**ok).ntouch > 0
    for change in (dict(nrows=3),                          # the successor is smaller than one block
                   dict(pred_wgs=7),                       # the predecessor has fewer workgroups than XCDs
                   dict(base=BASE + 64),                   # not line-aligned
                   dict(base=0),                           # no successor
                   dict(budget=4 * 2048 - 128)):           # the budget buys no whole block
        p = make(**{**ok, **change})
        assert p.ntouch == 0, change
        assert all(lines_of(p, wg) == [] for wg in range(0, 70))


@pytest.mark.parametrize("budget_mib", [8, 16, 24])
def test_budget_sweep_points(budget_mib):
    for shape in (0, 1):
        p, g = gemv_plan(GATEUP, DOWN, budget=budget_mib * MIB, shape=shape)
        check_flat(p, g, budget_mib * MIB)
