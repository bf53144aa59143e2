"""GPU: the few-row (4..16) stream over the 12-bit packed bf16 sets (csrc/gemv_pack_thin.hip at BITS = 12, emu_linear_bf16pack12_thin,
LlamaEngine.use_bf16_pack_wide(keep12=True)).  Every comparison is on the raw bits with a NaN guard band behind the output: the
primitive against emu_linear_bf16 on the bf16 matrix (the bf16 few-row stream), the decode and the patches against the matrix itself
through one-hot activations over a poisoned bf16 matrix, flagged and unflagged workgroups with a witness of which branch ran, a small
engine and one true-shape layer.  Before any device work every case asserts from emu_amd/bf16pack.py::pack12 which groups are flagged
and how many patch slots are in use, so a case that means to exercise patches cannot pass on an empty record."""
import ctypes as C

import pytest
import torch

from tests.test_gpu_bf16_pack12 import _clean, _fields, _random, _tiny
from tests.test_gpu_bf16_pack_wide import (BF16, BLOCK_ONLY, EPI_NONE, EPI_RESID, EPI_SWIGLU, FLAG_CASES, PIN16, PIN32, ROWS, SHAPES, _beam,
                                           _engine, _five_row_steps, _guarded, _lib, _lookup, _plan, _Tune, bits)

pytestmark = pytest.mark.gpu

PINS = (PIN16, PIN32)


def _restated(W, R, flagged, slots=None, used=None):
    """pack12's dict of W after asserting the witness: the flagged groups (list of bool, or None = none), the slots in use in all
    (``slots``) or group by group (``used``)."""
    from emu_amd import bf16pack
    p = bf16pack.pack12(W, R)
    fl = bf16pack.flagged_groups(p).tolist()
    assert fl == (list(flagged) if flagged is not None else [False] * len(fl))
    u = bf16pack.slots_used(p)
    assert int(u.max()) <= 8
    assert slots is None or int(u.sum()) == slots, int(u.sum())
    assert used is None or u.tolist() == list(used), u.tolist()
    return p


def _packed(Wd, want_p):
    """The device's 12-bit set of Wd, the same records as the restatement's."""
    from emu_amd import ops
    p = ops.pack12_bf16_rows(Wd, want_p["rows"])
    assert p["hb"] == want_p["hb"] and p["flagged"] == want_p["flagged"] and torch.equal(p["patch"].cpu(), want_p["patch"])
    return p


def _one_hot(cols, K):
    x = torch.zeros(len(cols), K, dtype=BF16, device="cuda")
    x[torch.arange(len(cols)), torch.tensor(cols)] = 1.0
    return x


def _one_hot_witness(Wd, p, cols, M, tune, poisoned=True, cold=False):
    """out[m, n] must be W[n, cols[m]] bit for bit, M columns per launch (the last launch filled up from the front), the bf16 matrix
    poisoned (not where the set has flagged groups, which read it): an unpatched miss decodes to code 0 of the window and fails this.
    ``cold``: a GiB is written before every launch, so the planes and the patch records come from HBM, not from a cache."""
    from emu_amd import ops
    N, K = Wd.shape
    poison = torch.full_like(Wd, float("nan")) if poisoned else Wd
    cols = list(cols)
    with _Tune(tune):
        for c0 in range(0, len(cols), M):
            chunk = (cols[c0:c0 + M] + cols)[:M]
            out, guard = _guarded(M, N)
            x = _one_hot(chunk, K)
            if cold:
                torch.empty(2 ** 30, dtype=torch.uint8, device="cuda").fill_(c0 & 255)
            ops.linear_bf16pack_thin(x, poison, p, out=out)
            torch.cuda.synchronize()
            assert torch.equal(bits(out), bits(Wd[:, chunk].t())), (c0, chunk)
            assert bool(torch.isnan(guard.float()).all())


def _against_linear(Wd, p, M, tune, seed, epis=(EPI_NONE,), finite=True):
    from emu_amd import ops
    N, K = Wd.shape
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, K, generator=g) * 0.5).to(BF16).cuda()
    res = torch.randn(M, N, generator=g).to(BF16).cuda()
    for epi in epis:
        r = res if epi == EPI_RESID else None
        want = ops.linear(x, Wd, res=r, epi=epi)                               # emu_gemm_tune 0: the bf16 few-row stream
        out, guard = _guarded(M, N // 2 if epi == EPI_SWIGLU else N)
        with _Tune(tune):
            ops.linear_bf16pack_thin(x, Wd, p, res=r, epi=epi, out=out)
        torch.cuda.synchronize()
        assert not finite or bool(torch.isfinite(want.float()).all())
        assert torch.equal(bits(out), bits(want)), (M, epi)
        assert bool(torch.isnan(guard.float()).all()), (M, epi)                # nothing written past the rows


# ------------------------------------------------------------------------------------------------ 1. bit identity with the bf16 stream
# the weight law's natural misses (restated on the CPU): none in the two smallest, 4 / 20 / 12 in the next, 1169 in (2240, 6656) with no
# flagged group and, at R = 4, one group with a full record of 8
MISSES = {(37, 256): 0, (50, 1024): 4, (264, 768): 20, (64, 2560): 12, (2240, 6656): 1169}
CASES = [(N, K, R, tune) for N, K, Rs in SHAPES for R in Rs for tune in PINS]


@pytest.fixture(scope="module")
def law():
    """(N, K, R) -> (the matrix on the device, its restated set, its device set), made once."""
    made = {}

    def get(N, K, R):
        if (N, K, R) not in made:
            W = _random(N, K, seed=N + K)
            want_p = _restated(W, R, None, slots=MISSES[(N, K)])
            if (N, K, R) == (2240, 6656, 4):
                from emu_amd import bf16pack
                assert int((bf16pack.slots_used(want_p) == 8).sum()) == 1
            Wd = W.cuda()
            made[(N, K, R)] = (Wd, want_p, _packed(Wd, want_p))
        return made[(N, K, R)]
    return get


@pytest.mark.parametrize("N,K,R,tune", CASES)
def test_bits_of_the_bf16_stream(law, N, K, R, tune):
    Wd, _, p = law(N, K, R)
    epis = (EPI_NONE, EPI_RESID) + ((EPI_SWIGLU,) if N % 2 == 0 else ())
    for M in ROWS:
        for epi in epis:
            assert _plan(M, N, K, epi, R, tune) == ((32, 4 if M <= 8 else 3) if tune == PIN32 else (16, 6 if M <= 8 else 5))
        _against_linear(Wd, p, M, tune, seed=N * 3 + K + R + M, epis=epis)


# ------------------------------------------------------------------------------------------------ 2. decode exactness
def _all_codes_matrix():
    """[4096, 256]: column k holds every 12-bit code (sign, 3-bit exponent code, low byte) once, so every code meets every position
    of a stage; hb = 56 puts the exponent fields at 112 .. 127: all finite, none zero."""
    n = torch.arange(4096, dtype=torch.int32)[:, None]
    k = torch.arange(256, dtype=torch.int32)[None, :]
    code = (n + 37 * k) % 4096
    b = ((code >> 11) << 15) | ((((code >> 8) & 7) + 56) << 8) | (code & 255)
    return torch.where(b >= 2 ** 15, b - 2 ** 16, b).to(torch.int16).view(BF16)


@pytest.fixture(scope="module")
def all_codes():
    from emu_amd import bf16pack
    W = _all_codes_matrix()
    b = W.view(torch.int16).to(torch.int32) & 0xFFFF
    codes = ((b >> 15) << 11) | ((((b >> 8) & 0x7F) - 56) << 8) | (b & 255)
    assert all(sorted(codes[:, k].tolist()) == list(range(4096)) for k in (0, 1, 127, 255))
    assert bool(torch.isfinite(W.float()).all()) and bool((W.float() != 0).all())
    assert bf16pack.window_rule(bf16pack.histogram12(W)) == 56 and not bool(bf16pack.miss_rule12(W, 56).any())
    return W


@pytest.mark.parametrize("tune", PINS)
@pytest.mark.parametrize("R", [2, 4])
def test_every_code_decodes_exactly(all_codes, R, tune):
    """One-hot activation rows: out[m, n] must be W[n, k_m], independent of the bf16 kernel.  Sixteen k per launch, sixteen launches."""
    want_p = _restated(all_codes, R, None, slots=0)
    assert want_p["hb"] == 56
    Wd = all_codes.cuda()
    _one_hot_witness(Wd, _packed(Wd, want_p), range(256), 16, tune)


# ------------------------------------------------------------------------------------------------ 3. a patch wherever a lane can own one
E4 = (0, 3, 4, 7)                                                     # both halves of the first and of the last dword of a vector


def _spots():
    """(64, 2560), ten stages: (row, vector index, element) of 34 misses -- chunk c of stage (3 c + 1) % 10 for every c (so every wave,
    sub-step and g), rows over all four 16-row blocks, then the first row's last vector and the last row's first."""
    s = [((5 * c + 7) % 64, 32 * ((3 * c + 1) % 10) + c, E4[(c // 4 + c) % 4]) for c in range(32)]
    return s + [(0, 319, 7), (63, 0, 0)]


def _planted(values):
    W = _clean(64, 2560, seed=5)
    for k, (row, vi, j) in enumerate(_spots()):
        W[row, vi * 8 + j] = values(k)
    return W


def _tiny_k(k):
    """The k-th planted miss: far below the window, signs alternating (tests/test_gpu_bf16_pack12.py::_plant's values)."""
    return _tiny(k & 1, k % 100)


def _check_spots(want_p, R):
    got = _fields(want_p)                                              # (group, trip, lane, row, element); vi = 256 trip + lane
    assert got == {(row // R, vi >> 8, vi & 255, row % R, j) for row, vi, j in _spots()}
    from emu_amd import bf16pack
    assert int(bf16pack.slots_used(want_p).max()) <= 3
    spots = _spots()
    assert {vi >> 5 for _, vi, _ in spots} == set(range(10)) and {vi & 31 for _, vi, _ in spots} == set(range(32))
    assert {row % R for row, _, _ in spots} == set(range(R)) and {j for _, _, j in spots} == set(E4)
    assert {row >> 4 for row, _, _ in spots} == {0, 1, 2, 3} and {row & 15 for row, _, _ in spots} == set(range(16))


@pytest.mark.parametrize("tune", PINS)
@pytest.mark.parametrize("R", [2, 4])
def test_a_patch_wherever_a_lane_can_own_one(R, tune):
    W = _planted(_tiny_k)
    want_p = _restated(W, R, None, slots=34)
    _check_spots(want_p, R)
    Wd = W.cuda()
    p = _packed(Wd, want_p)
    cols = [vi * 8 + j for _, vi, j in _spots()]
    for M in (5, 16):
        assert _plan(M, 64, 2560, EPI_NONE, R, tune)[0] == (32 if tune == PIN32 else 16)
        _one_hot_witness(Wd, p, cols, M, tune)
    # the same spots with values a bf16 sum shows, against the bf16 stream on random activations
    big = _planted(lambda k: 4.0 if k % 2 == 0 else -3e4)
    want_big = _restated(big, R, None, slots=34)
    _check_spots(want_big, R)
    Bd = big.cuda()
    pb = _packed(Bd, want_big)
    for M in (5, 16):
        _against_linear(Bd, pb, M, tune, seed=R + M, epis=(EPI_NONE, EPI_RESID, EPI_SWIGLU))
        _one_hot_witness(Bd, pb, cols, M, tune)


# ------------------------------------------------------------------------------------------------ 4. a full record
@pytest.mark.parametrize("tune", PINS)
@pytest.mark.parametrize("R", [2, 4])
def test_a_full_record_of_eight_between_empty_ones(R, tune):
    """Group 1 of 40 / R uses all 8 slots: elements 0 and 1 of one vector of one row (both halves of one dword) and element 6 of the same
    vector, the group's last row at the same vector index, slots in the first and in the last stage."""
    K = 2560
    spots = [(0, 7, 0), (0, 7, 1), (0, 7, 6), (R - 1, 7, 2), (0, 40, 7), (R // 2, 100, 4), (R - 1, 300, 3), (0, 319, 5)]     # (row in group, vi, j)
    W = _clean(40, K, seed=R + 1)
    for k, (r, vi, j) in enumerate(spots):
        W[R + r, vi * 8 + j] = _tiny_k(k)
    want_p = _restated(W, R, None, used=[0, 8] + [0] * (40 // R - 2))
    assert {vi >> 5 for _, vi, _ in spots} >= {0, 9}
    Wd = W.cuda()
    _one_hot_witness(Wd, _packed(Wd, want_p), [vi * 8 + j for _, vi, j in spots], 8, tune)


# ------------------------------------------------------------------------------------------------ 5. Inf and NaN
@pytest.mark.parametrize("tune", PINS)
@pytest.mark.parametrize("R", [2, 4])
def test_inf_and_nan_travel_in_patches(R, tune):
    """Inf and NaN are misses like any other: they ride in patch slots, the groups stay unflagged and the outputs (Inf / NaN where the
    bf16 stream gives them) are the same bits.  (Against the bf16 stream only: 0 x Inf is NaN, so one-hot rows show nothing here.)"""
    W = _clean(64, 768, seed=9)
    W[1, 17] = float("inf"); W[2, 700] = float("nan"); W[37, 767] = float("-inf"); W[5, 0] = 0.0
    want_p = _restated(W, R, None, slots=4)
    Wd = W.cuda()
    p = _packed(Wd, want_p)
    for M in (5, 16):
        _against_linear(Wd, p, M, tune, seed=9 + M, finite=False)


# ------------------------------------------------------------------------------------------------ 6. flags
def _flag_planted(N, K, R):
    """9 misses in group 0 and 9 in the last group (both flagged: more than 8), 1 / 2 / 3 patches in three groups between them."""
    G, KV = (N + R - 1) // R, K // 8
    W = _clean(N, K, seed=11)
    k = 0
    for grp in (0, G - 1):
        for i in range(9):
            W[grp * R + i % R, ((3 + 5 * i) % KV) * 8 + (i + i // 8) % 8] = _tiny_k(k); k += 1
    for n, grp in ((1, G // 3), (2, G // 2), (3, 2 * G // 3)):
        for i in range(n):
            W[grp * R + (i + 1) % R, ((7 + 11 * i) % KV) * 8 + E4[i]] = _tiny_k(k); k += 1
    return W, [grp in (0, G - 1) for grp in range(G)], {G // 3: 1, G // 2: 2, 2 * G // 3: 3}


@pytest.mark.parametrize("case", sorted(FLAG_CASES))
@pytest.mark.parametrize("R", [2, 4])
def test_flagged_workgroups_stream_bf16_and_the_others_planes_and_patches(R, case):
    from emu_amd import bf16pack, ops
    N, K, M, tune = case
    W, flagged, patched = _flag_planted(N, K, R)
    want_p = _restated(W, R, flagged, slots=6)
    used = bf16pack.slots_used(want_p)
    assert {g: int(used[g]) for g in patched} == patched and int(used[0]) == 0 and int(used[-1]) == 0      # a flagged group's record is empty
    rn, stages = _plan(M, N, K, EPI_NONE, R, tune)                           # the workgroup extent
    assert (rn, stages) == FLAG_CASES[case]
    nwg = (N + rn - 1) // rn
    fl = torch.tensor(flagged)
    wg_flagged = torch.zeros(nwg, dtype=torch.bool)
    wg_flagged[(torch.nonzero(fl).flatten() * R) // rn] = True
    assert wg_flagged.tolist() == [True] + [False] * (nwg - 2) + [True]      # one in the first workgroup, one in the last
    assert all(not wg_flagged[g * R // rn] for g in patched)                 # the patched groups are in workgroups that stream the planes
    Wd = W.cuda()
    p = _packed(Wd, want_p)
    g = torch.Generator().manual_seed(R)
    x = (torch.randn(M, K, generator=g) * 0.5).to(BF16).cuda()
    want = ops.linear(x, Wd)
    row_flagged = wg_flagged.repeat_interleave(rn)[:N].cuda()
    # witness: the unflagged workgroups never read the bf16 rows, the flagged ones use neither the planes nor the patch records
    W_nan = Wd.clone()
    W_nan[~row_flagged] = float("nan")
    q = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in p.items()}
    grp_flagged = wg_flagged.repeat_interleave(rn // R)[:q["lo"].shape[0]].cuda()
    for name in ("lo", "nib"):
        noise = torch.randint(0, 256, q[name].shape, dtype=torch.uint8, generator=g).cuda()
        q[name][grp_flagged] = noise[grp_flagged]
    noise = torch.randint(-2 ** 31, 2 ** 31 - 1, q["patch"].shape, dtype=torch.int64, generator=g).to(torch.int32).cuda()
    q["patch"][grp_flagged] = noise[grp_flagged]
    with _Tune(tune):
        for w_arg, set_arg in ((Wd, p), (W_nan, p), (Wd, q), (W_nan, q)):
            out, guard = _guarded(M, N)
            ops.linear_bf16pack_thin(x, w_arg, set_arg, out=out)
            torch.cuda.synchronize()
            assert torch.equal(bits(out), bits(want))
            assert bool(torch.isnan(guard.float()).all())


# ------------------------------------------------------------------------------------------------ 7. ragged N
@pytest.mark.parametrize("tune", PINS)
@pytest.mark.parametrize("R", [2, 4])
def test_ragged_n_a_patch_in_the_last_real_row(R, tune):
    """(37, 256): the last group is padded (one real row of R), the last workgroup's further groups are clamped to it under both pins;
    a patch in row 36, one in row 35 (R = 2: the group before) and one in the first row."""
    N, K = 37, 256
    spots = [(36, 31, 7), (36, 12, 0), (35, 5, 3), (0, 0, 4), (20, 18, 1)]   # (row, vi, j)
    W = _clean(N, K, seed=7)
    for k, (row, vi, j) in enumerate(spots):
        W[row, vi * 8 + j] = _tiny_k(k)
    G = (N + R - 1) // R
    want_p = _restated(W, R, [False] * G, slots=5)
    assert want_p["lo"].shape[0] == G and G * R > N                          # the last group is padded
    assert (36 // R, 0, 31, 36 % R, 7) in _fields(want_p)
    Wd = W.cuda()
    p = _packed(Wd, want_p)
    _one_hot_witness(Wd, p, [vi * 8 + j for _, vi, j in spots], 5, tune)
    _against_linear(Wd, p, 9, tune, seed=R, epis=(EPI_NONE, EPI_RESID))


# ------------------------------------------------------------------------------------------------ 8. a small engine
def test_small_engine_keeps_its_12_bit_sets():
    """tests/test_gpu_bf16_pack.py's engine on 12-bit sets (o_proj and down of both layers, R = 2, made under the block-kernel-only tune
    bit).  A 5-beam search and a prompt-lookup generation with k = 4 (5-row chunk steps), eager and from a graph, give the ids and the
    last-step logits of the switch-off run with keep12; the sets still hold their patch records, and the GEMV profiler prices the
    5-row steps at the 12-bit sets' bytes -- the witness that the 12-bit twin ran.  Then off, and on without keep12: repacked to 13."""
    from emu_amd import bf16pack
    eng = _engine()
    keys = ["0.wdown", "0.wo", "1.wdown", "1.wo"]
    runs = {}
    with _Tune(BLOCK_ONLY):
        assert eng.pack_bf16(tune=BLOCK_ONLY, bits12=True)[0] == 4 and sorted(eng._pack) == keys
        assert all("patch" in v and v["flagged"] == 0 for v in eng._pack.values())
        with pytest.raises(RuntimeError, match="use_bf16_pack"):
            eng.use_bf16_pack_wide(True, keep12=True)                        # needs the packed stream on
        eng.use_bf16_pack(True)
        sets12 = sum(bf16pack.packed_bytes12(*v["shape"], 2) for v in eng._pack.values())
        sets13 = sum(bf16pack.packed_bytes(*v["shape"], 2) for v in eng._pack.values())
        for state in ("off", "keep12", "off again", "repacked"):
            epoch = eng.mode_epoch
            if state == "keep12":
                eng.use_bf16_pack_wide(True, keep12=True)
            else:
                eng.use_bf16_pack_wide(state == "repacked")
            assert eng.bf16_pack_wide == (state in ("keep12", "repacked"))
            assert eng.mode_epoch > epoch and not eng.__dict__.get("_loop_states")             # the captured graphs went with the mode
            assert sorted(eng._pack) == keys and all(("patch" in v) == (state != "repacked") for v in eng._pack.values()), state
            runs[state] = dict(beam={gr: _beam(eng, gr) for gr in (False, True)}, lookup={gr: _lookup(eng, gr) for gr in (False, True)},
                               prof=_five_row_steps(eng, 2))
        eng.use_bf16_pack_wide(False)
        eng.beam_graph = True
    off = runs["off"]
    for state in ("keep12", "off again", "repacked"):
        for loop in ("beam", "lookup"):
            for gr in (False, True):
                assert torch.equal(runs[state][loop][gr][0], off[loop][gr][0]), (state, loop, gr)
                assert torch.equal(bits(runs[state][loop][gr][1]), bits(off[loop][gr][1])), (state, loop, gr)
        for a, b in zip(runs[state]["prof"][2], off["prof"][2]):
            assert torch.equal(bits(a), bits(b))
    full = 2 * 2 * (256 * 256 + 256 * 512)                                   # the four matrices as bf16
    (b_off, n_off, _), (b_12, n_12, _), (b_again, n_again, _), (b_13, n_13, _) = (runs[s]["prof"] for s in ("off", "keep12", "off again", "repacked"))
    assert n_12 == n_off == n_again == n_13 and b_again == b_off
    assert b_off - b_12 == pytest.approx(2 * (full - sets12))                # two steps: the four matrices at their 12-bit sets
    assert b_off - b_13 == pytest.approx(2 * (full - sets13)) and b_12 < b_13 < b_off


# ------------------------------------------------------------------------------------------------ 9. one true-shape layer
def test_true_shape_layer_and_head_five_rows_then_one_on_the_same_sets():
    """One layer at 6656 / 52 heads / 17920 and a vocabulary of 8192, all five matrices on 12-bit sets.  A five-row chunk step plus the
    logits with keep12 are the bits of the switch-off run and the profiler prices the five launches at the 12-bit sets; a one-row
    step taken afterwards is priced at the same sets -- one resident set per matrix serves both."""
    from emu_amd import bf16pack, synth
    from emu_amd._lib import check
    from emu_amd.conf.emu_conf import LlamaCfg
    from emu_amd.llama import EmuHipContext, LlamaEngine
    cfg = LlamaCfg(hidden_size=6656, intermediate_size=17920, num_attention_heads=52, num_hidden_layers=1)
    dev = torch.device("cuda", 0)
    eng = LlamaEngine(cfg, 8192, EmuHipContext(dev, 0, 1))
    eng.load_weights(synth.iter_synth(synth.llama_param_shapes(cfg, 8192), seed=1, device=dev, dtype=BF16))
    eng.pack_bf16(head_form=True, bits12=True)
    keys = ["0.wqkv", "0.wo", "0.wgu", "0.wdown", "lm_head"]
    assert sorted(eng._pack) == sorted(keys) and [eng._pack[k]["rows"] for k in keys] == [4, 2, 4, 2, 4]
    for k in keys:
        p = eng._pack[k]
        G = -(-p["shape"][0] // p["rows"])
        assert "patch" in p and bf16pack.set_bits(p["flagged"], G, p["rows"], p["shape"][1]) == 12 and 100 * p["flagged"] < G, k
        assert int((p["patch"] != -1).sum()) > 100, k                       # the weight law's misses are there
    eng.use_bf16_pack(True)
    L = _lib()
    g = torch.Generator().manual_seed(2)
    eng.alloc_kv(1, 64)
    kv0 = (torch.randn(2, 1, 1, 52, 64, 128, generator=g) * 0.5).to(BF16).to(dev)
    x = (torch.randn(1, 6656, generator=g) * 0.5).to(BF16).to(dev)
    x5 = (torch.randn(5, 6656, generator=g) * 0.5).to(BF16).to(dev)
    pos = torch.tensor([63], device=dev, dtype=torch.int32)
    at = torch.tensor([59], device=dev, dtype=torch.int32)
    kstart = torch.zeros(1, device=dev, dtype=torch.int32)

    def profiled(step):
        eng.kcache.copy_(kv0[0]); eng.vcache.copy_(kv0[1])
        check(L.emu_profile_gemv(1), "emu_profile_gemv")
        try:
            got = step()
            torch.cuda.synchronize()
            ms, wb, nl = C.c_double(), C.c_double(), C.c_long()
            check(L.emu_profile_gemv_read(C.byref(ms), C.byref(wb), C.byref(nl)), "emu_profile_gemv_read")
        finally:
            L.emu_profile_gemv(0)
        return got, wb.value, nl.value

    def five_rows():
        h = eng.forward_chunk(x5.clone(), 1, 5, at, at, kstart, 64)
        lg = eng.logits(h)
        return h.clone(), lg.clone(), eng.kcache[0, 0, :, 59:64].clone(), eng.vcache[0, 0, :, 59:64].clone()

    def one_row():
        h = eng.decode_embeds(x, pos, 63, kstart)
        lg = eng.logits(h)
        return h.clone(), lg.clone(), eng.kcache[0, 0, :, 63].clone(), eng.vcache[0, 0, :, 63].clone()

    shapes = {k: tuple(eng._pack[k]["shape"]) for k in keys}
    sets12 = sum(eng._set_bytes(eng._pack[k]) for k in keys)
    as_bf16 = sum(2 * n * k for n, k in shapes.values())
    off5, bytes_off5, n_off5 = profiled(five_rows)
    off1, bytes_off1, n_off1 = profiled(one_row)
    assert (bytes_off5, n_off5) == (as_bf16, 5) and (bytes_off1, n_off1) == (sets12, 5)       # today's default: few rows on bf16, one row on 12 bits
    for R, (N, K), epi in zip((4, 2, 4, 2, 4), (shapes[k] for k in keys), (EPI_NONE, EPI_RESID, EPI_SWIGLU, EPI_RESID, EPI_NONE)):
        assert L.emu_llama_pack_thin_kernel(0, 5, R, N, K, 1, 2, N, K, 0, epi, 0) == 8
    eng.use_bf16_pack_wide(True, keep12=True)
    assert all("patch" in eng._pack[k] for k in keys)
    on5, bytes_on5, n_on5 = profiled(five_rows)
    on1, bytes_on1, n_on1 = profiled(one_row)
    eng.use_bf16_pack_wide(False)
    assert (bytes_on5, n_on5) == (sets12, 5)                                 # the 12-bit twin is what ran
    assert (bytes_on1, n_on1) == (sets12, 5)                                 # ... and the one-row step still streams the same sets
    assert bool(torch.isfinite(on5[0].float()).all()) and bool(torch.isfinite(on5[1].float()).all())
    for a, b in zip(on5 + on1, off5 + off1):
        assert torch.equal(bits(a), bits(b))
    # The weight law's misses are tiny values that a bf16 sum over random rows does not show, so the steps above cannot see a patch
    # that was not applied.  One-hot rows at naturally missed columns of o_proj and down can -- the 16-row tiles, eight row groups'
    # records to a workgroup, planes and records cold
    for key in ("0.wo", "0.wdown"):
        Wd, p = eng._keep[key], eng._pack[key]
        N, K = Wd.shape
        assert p["rows"] == 2 and all(_plan(M, N, K, EPI_NONE, 2, 0)[0] == 16 for M in (5, 16))
        pt = p["patch"].cpu().to(torch.int64) & 0xFFFFFFFF
        grp, sl = (pt != 0xFFFFFFFF).nonzero(as_tuple=True)
        slots = pt[grp, sl]
        rows, cols = grp * 2 + ((slots >> 11) & 3), (slots >> 13) * 8 + ((slots >> 8) & 7)
        missed = bits(Wd)[rows.cuda(), cols.cuda()].cpu().to(torch.int64) & 0xFFFF
        assert torch.equal(missed >> 8, slots & 255)                       # the records name these weights' high bytes
        live = ((missed & 0x7FFF) != 0).nonzero().flatten()                # (a signed zero is no witness: the sum gives + 0 either way)
        pick, seen = [], set()
        for i in live[:: max(1, len(live) // 64)].tolist():               # spread over the matrix, distinct columns
            if int(cols[i]) not in seen and len(pick) < 16:
                seen.add(int(cols[i])); pick.append(i)
        assert len(pick) == 16 and len({int(rows[i]) // 16 for i in pick}) >= 8      # sixteen misses in at least eight workgroups
        for M in (5, 16):
            _one_hot_witness(Wd, p, [int(cols[i]) for i in pick], M, 0, poisoned=False, cold=True)
