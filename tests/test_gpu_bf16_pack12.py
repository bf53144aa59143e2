"""GPU: the 12-bit lossless bf16 decode stream.  The device packer against emu_amd/bf16pack.py::pack12 byte for byte; the 12-bit twins
(emu_linear_bf16pack12) against emu_linear_bf16 on the raw bf16 bits with a NaN guard band behind the row -- sizes and tails of each
form, patches in every trip, row and half of a vector, a full record, flagged and clean groups in one workgroup, a lone last group
clean and flagged; a small engine on 12-bit sets, 13-bit sets and bf16.  Every case first asserts, from the Python restatement, which
path its row groups take and how many patch slots are in use, so a case that means to exercise patches cannot pass on an empty record.
Every comparison is bit-exact."""
import pytest
import torch

from tests.test_gpu_bf16_pack import BF16, BLOCK_ONLY, EPI_NONE, EPI_RESID, EPI_SWIGLU, HEAD, PRELOAD, RT, _Tune, _engine, _gemv_bytes, bits

pytestmark = pytest.mark.gpu

FORMS = {HEAD: (4, True), PRELOAD: (2, False), RT: (2, False)}        # form -> (rows per group, fused RMSNorm)


def _random(N, K, seed):
    """The bench's weight law: N(0, 0.02^2), natural misses and all."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=g) * 0.02).to(BF16)


def _clean(N, K, seed):
    """N(0, 0.02^2) with every weight inside exponent fields 112..123: window [54, 61], no miss -- the base the planted cases start from."""
    W = _random(N, K, seed)
    e8 = (bits(W).to(torch.int32) >> 7) & 0xFF
    return torch.where((e8 < 112) | (e8 > 123), torch.full_like(W, 0.01), W)


def _tiny(sign, k):
    """A value far below the window (exponent field 3 + k): a miss wherever it is planted."""
    v = (sign << 15) | ((3 + k) << 7) | (5 * k + 1)
    return torch.tensor([v - 65536 if v >= 32768 else v], dtype=torch.int16).view(BF16)[0]


def _plant(W, rows, spots):
    """spots: (row group, row in group, trip, lane, element) -> a miss at that weight."""
    for k, (g, r, t, lane, j) in enumerate(spots):
        W[g * rows + r, (256 * t + lane) * 8 + j] = _tiny(k & 1, k % 100)
    return W


def _fields(p):
    """The patch records of a packed dict as {(group, trip, lane, row, element)}."""
    pt = p["patch"].to(torch.int64) & 0xFFFFFFFF
    g, s = (pt != 0xFFFFFFFF).nonzero(as_tuple=True)
    sl = pt[g, s]
    return set(zip(g.tolist(), (sl >> 21).tolist(), ((sl >> 13) & 255).tolist(), ((sl >> 11) & 3).tolist(), ((sl >> 8) & 7).tolist()))


def _case(W, form, epi, seed, flagged, min_slots, finite=True):
    """emu_linear_bf16pack12 over the 12-bit set of W == emu_linear_bf16 on W, on the raw bits.  ``flagged``: the row groups the
    restatement must flag (list of bool); ``min_slots``: the fewest patch slots it must have in use over the unflagged groups."""
    from emu_amd import bf16pack, ops
    rows, norm = FORMS[form]
    N, K = W.shape
    want_p = bf16pack.pack12(W, rows)
    assert bf16pack.flagged_groups(want_p).tolist() == list(flagged)                     # the witness: which path each group takes
    used = bf16pack.slots_used(want_p)
    assert int(used.sum()) >= min_slots and int(used.max()) <= 8
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(1, K, generator=g) * 0.5).to(BF16).cuda()
    gain = (1 + 0.1 * torch.randn(K, generator=g)).to(BF16).cuda() if norm else None
    res = torch.randn(1, N, generator=g).to(BF16).cuda() if epi == EPI_RESID else None
    Wd = W.cuda()
    want = ops.linear(x, Wd, res=res, norm_w=gain, eps=1e-5, epi=epi)
    p = ops.pack12_bf16_rows(Wd, rows)
    assert torch.equal(p["patch"].cpu(), want_p["patch"]) and p["flagged"] == want_p["flagged"]
    n_out = N // 2 if epi == EPI_SWIGLU else N
    out = torch.full((1, n_out + 8), float("nan"), dtype=BF16, device="cuda")           # a guard band behind the row
    ops.linear_bf16pack(x, Wd, p, form, res=res, norm_w=gain, eps=1e-5, epi=epi, out=out)
    torch.cuda.synchronize()
    assert not finite or bool(torch.isfinite(want.float()).all())
    assert torch.equal(bits(out[:, :n_out]), bits(want))
    assert bool(torch.isnan(out[:, n_out:].float()).all())                               # nothing written past the row
    return want_p


# ------------------------------------------------------------------------------------------------ 1. the packer
def _pack_matrices():
    W = _clean(9, 2080, seed=5)                                       # a partial last group for both R; patches, a full record, a flagged group
    _plant(W, 1, [(0, 0, 0, 3, 0), (1, 0, 1, 3, 7), (2, 0, 0, 255, 4), (3, 0, 1, 0, 3)] +
           [(4, 0, 0, 10 + i, i) for i in range(4)] + [(5, 0, 0, 20 + i, 7 - i) for i in range(4)] +
           [(6, 0, 0, 30 + i, i % 8) for i in range(5)] + [(7, 0, 1, i, (3 * i) % 8) for i in range(4)] + [(8, 0, 0, 9, 2)])
    special = _clean(8, 64, seed=6)
    for c, v in enumerate([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e-40, 4.0, -3e4]):
        special[c % 8, 7 * c + 1] = v
    return {"random 8x6656": _random(8, 6656, 1), "random 10x17920": _random(10, 17920, 2), "short 6x32": _clean(6, 32, 3),
            "planted 9x2080": W, "special 8x64": special}


@pytest.mark.parametrize("rows", [2, 4])
@pytest.mark.parametrize("name", ["random 8x6656", "random 10x17920", "short 6x32", "planted 9x2080", "special 8x64"])
def test_device_packer_matches_python(name, rows):
    from emu_amd import bf16pack, ops
    W = _pack_matrices()[name]
    want = bf16pack.pack12(W, rows)
    got = ops.pack12_bf16_rows(W.cuda(), rows)
    assert got["hb"] == want["hb"] and got["rows"] == rows and tuple(got["shape"]) == tuple(W.shape) and got["flagged"] == want["flagged"]
    for k in ("lo", "nib", "patch", "flags"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert torch.equal(got[k].cpu(), want[k]), k
    back, fl = bf16pack.unpack12({**want, **{k: got[k].cpu() for k in ("lo", "nib", "patch", "flags")}})
    assert torch.equal(bits(back)[~fl], bits(W)[~fl])
    if name == "planted 9x2080":
        assert want["flagged"] == 1 and not bf16pack.flagged_groups(want).all()
        assert bf16pack.slots_used(want).tolist() == ([2, 2, 8, 0, 1] if rows == 2 else [4, 0, 1])     # a full record at R = 2; the flagged group's is empty
    if name.startswith("random"):
        assert want["flagged"] == 0 and int(bf16pack.slots_used(want).sum()) > 0       # the natural misses of the weight law


# ------------------------------------------------------------------------------------------------ 2. the twins: sizes and tails
# N in 4..20 (one group, a lone last group, a padded last group, whole pairs), every K, both epilogues (SwiGLU pairs rows: even N)
HEAD_CASES = [(N, K, epi) for N in range(4, 21) for K in (32, 64, 2080, 6656) for epi in (EPI_NONE, EPI_SWIGLU) if not (epi == EPI_SWIGLU and N & 1)]


@pytest.mark.parametrize("N,K,epi", HEAD_CASES)
def test_head_form(N, K, epi):
    G = (N + 3) // 4
    _case(_random(N, K, seed=N * 7 + K), HEAD, epi, seed=K + N + epi, flagged=[False] * G, min_slots=1 if K == 6656 else 0)


@pytest.mark.parametrize("K", [64, 6656])
@pytest.mark.parametrize("N", [2, 3, 4, 5, 6])
def test_preload_form(N, K):
    _case(_random(N, K, seed=N * 5 + K + 1), PRELOAD, EPI_RESID, seed=K + N, flagged=[False] * ((N + 1) // 2), min_slots=1 if K == 6656 else 0)


@pytest.mark.parametrize("K", [64, 17920])
@pytest.mark.parametrize("N", [2, 3, 4, 5, 6])
def test_single_round_trip_form(N, K):
    _case(_random(N, K, seed=N * 3 + K), RT, EPI_RESID, seed=K + N + 1, flagged=[False] * ((N + 1) // 2), min_slots=1 if K == 17920 else 0)


def test_random_rows_have_natural_misses_under_the_limit():
    """The seeds above: N(0, 0.02^2) rows at K = 6656 give a few misses per 4-row group and stay under 8 (on the CPU, no GPU work)."""
    from emu_amd import bf16pack
    used = bf16pack.slots_used(bf16pack.pack12(_random(20, 6656, seed=20 * 7 + 6656), 4))
    assert int(used.max()) <= 8 and int(used.sum()) >= 5 and int((used > 0).sum()) >= 3      # about 2 per group, most groups hit


# ------------------------------------------------------------------------------------------------ 3. patches
E4 = (0, 3, 4, 7)                                                     # both halves of the first and of the last dword of a vector


def _spread(form, K):
    """(N, spots): over four row groups, one patch in every trip, in every row of the group and in elements 0, 3, 4 and 7, at most
    8 to a group; the last trip's lane inside its ragged end."""
    rows = FORMS[form][0]
    KV = K // 8
    trips = (KV + 255) // 256
    spots = []
    for t in range(trips):
        for r in range(rows):
            g = (t + r) % 4
            lane = min(11 + 37 * r + 5 * t, KV - 256 * t - 1)
            spots.append((g, r, t, lane, E4[(t + r) % 4]))
    extra = [(g, r, 0, 200 + r, e) for g in range(4) for r, e in ((0, E4[g]), (rows - 1, E4[(g + 1) % 4]))]   # every element in every group's reach
    return 4 * rows, spots + extra


@pytest.mark.parametrize("form,K,epi", [(HEAD, 6656, EPI_NONE), (HEAD, 6656, EPI_SWIGLU), (PRELOAD, 6656, EPI_RESID), (RT, 17920, EPI_RESID)],
                         ids=["head", "head-swiglu", "preload", "rt"])
def test_a_patch_in_every_trip_row_and_half(form, K, epi):
    rows = FORMS[form][0]
    N, spots = _spread(form, K)
    W = _plant(_clean(N, K, seed=form + K), rows, spots)
    p = _case(W, form, epi, seed=form * 3 + epi, flagged=[False] * 4, min_slots=len(spots))
    got = _fields(p)
    assert got == {(g, t, lane, r, j) for g, r, t, lane, j in spots}
    trips = (K // 8 + 255) // 256
    assert {f[1] for f in got} == set(range(trips)) and {f[3] for f in got} == set(range(rows)) and {f[4] for f in got} == set(E4)
    assert trips == {HEAD: 4, PRELOAD: 4, RT: 9}[form]


@pytest.mark.parametrize("form,K,epi", [(HEAD, 6656, EPI_NONE), (PRELOAD, 6656, EPI_RESID), (RT, 17920, EPI_RESID)], ids=["head", "preload", "rt"])
def test_a_full_record_of_eight(form, K, epi):
    """Group 1 uses all 8 slots: two patches in one lane's vector (same trip and row), two lanes of one trip, every element once."""
    rows = FORMS[form][0]
    last = (K // 8 - 1) // 256
    spots = [(1, 0, 0, 7, 0), (1, 0, 0, 7, 1), (1, rows - 1, 0, 8, 2), (1, rows - 1, 1, 255, 3), (1, 0, 1, 0, 4), (1, rows - 1, last, 1, 5),
             (1, 0, last, 0, 6), (1, rows // 2, 2, 100, 7)]
    W = _plant(_clean(3 * rows, K, seed=form + 1), rows, spots)
    p = _case(W, form, epi, seed=form, flagged=[False] * 3, min_slots=8)
    from emu_amd import bf16pack
    assert bf16pack.slots_used(p).tolist() == [0, 8, 0]


def _ragged(form, K):
    """A full record in group 0 whose slots 4..7 (the slots are sorted by vector) sit in the last four vectors of the row, slots 0..3
    in the first ones.  Where KV % 64 == 4 those four vectors are all that the last wave of the last trip holds: the patch test
    must see the whole record all the same.  K = 32: the row IS four vectors, two misses in each."""
    rows = FORMS[form][0]
    KV = K // 8
    if KV == 4:
        return [(0, (i // 4) % rows if rows == 2 else i // 2, 0, i % 4, (3 * i) % 8) for i in range(8)]
    first = [(0, i % rows, 0, i, (3 * i) % 8) for i in range(4)]
    last = [(0, (i + 1) % rows, (KV - 4 + i) // 256, (KV - 4 + i) % 256, (5 * i + 1) % 8) for i in range(4)]
    return first + last


@pytest.mark.parametrize("form,K,epi", [(HEAD, 32, EPI_NONE), (HEAD, 2080, EPI_NONE), (HEAD, 2080, EPI_SWIGLU), (HEAD, 4128, EPI_NONE),
                                        (PRELOAD, 32, EPI_RESID), (PRELOAD, 544, EPI_RESID), (PRELOAD, 2080, EPI_RESID), (RT, 32, EPI_RESID),
                                        (RT, 544, EPI_RESID), (RT, 2080, EPI_RESID)])
def test_the_last_slots_in_the_last_four_vectors(form, K, epi):
    from emu_amd import bf16pack
    rows = FORMS[form][0]
    KV = K // 8
    assert KV % 64 == 4
    spots = _ragged(form, K)
    W = _plant(_clean(2 * rows, K, seed=form + K), rows, spots)
    p = _case(W, form, epi, seed=form + K + epi, flagged=[False, False], min_slots=8)
    assert bf16pack.slots_used(p).tolist() == [8, 0]
    vis = [(int(sl) & 0xFFFFFFFF) >> 13 for sl in p["patch"][0].tolist()]
    assert vis == sorted(vis) and (vis[4:] == list(range(KV - 4, KV)) or KV == 4 and vis == [0, 0, 1, 1, 2, 2, 3, 3])


# ------------------------------------------------------------------------------------------------ 4. flagged workgroups
def _nine(g, rows):
    return [(g, i % rows, 0, 3 + 5 * i, (i + i // 8) % 8) for i in range(9)]     # more than 8 misses: the group is flagged


@pytest.mark.parametrize("epi", [EPI_NONE, EPI_SWIGLU])
@pytest.mark.parametrize("K", [64, 6656])
@pytest.mark.parametrize("order", ["CF", "FC", "CFC", "FCF", "FF"])
def test_head_form_flagged_and_clean_groups(order, K, epi):
    """A head-form workgroup owns two groups.  C: a clean group with two patches; F: a flagged one (9 misses).  CF / FC: one of each in
    a workgroup (it streams the bf16 rows of all 8, the clean group's patches not applied to them); CFC: a lone last group, clean;
    FCF: a lone last group, flagged; FF: both flagged."""
    spots = []
    for g, c in enumerate(order):
        spots += _nine(g, 4) if c == "F" else [(g, 1, 0, 2, 3), (g, 2, (K // 8 - 1) // 256, 1, 4)]
    if K == 64:
        spots = [(g, r, 0, lane % 8, j) for g, r, t, lane, j in spots]
        spots = sorted(set(spots))
    W = _plant(_clean(4 * len(order), K, seed=len(order) + K), 4, spots)
    _case(W, HEAD, epi, seed=K + epi, flagged=[c == "F" for c in order], min_slots=order.count("C"))


@pytest.mark.parametrize("form,K", [(PRELOAD, 64), (PRELOAD, 6656), (RT, 64), (RT, 17920)])
def test_two_row_forms_flagged_and_clean_groups(form, K):
    """One workgroup per group: clean with patches, flagged, and a flagged lone last row (N = 5: the last group is half padding)."""
    last = (K // 8 - 1) // 256
    spots = [(0, 1, 0, 2, 3), (0, 0, last, 1, 4)] + [(1, i % 2, 0, (3 + 5 * i) % (K // 8), (i + i // 8) % 8) for i in range(9)] + \
            [(2, 0, 0, (4 + 3 * i) % (K // 8), (i + 1 + i // 8) % 8) for i in range(9)]
    W = _plant(_clean(5, K, seed=form + K), 2, spots)
    _case(W, form, EPI_RESID, seed=form + K, flagged=[False, True, True], min_slots=2)


def test_inf_and_nan_travel_in_patches():
    """Inf and NaN are misses like any other: they ride in patch slots, the group stays unflagged, and the outputs (Inf / NaN where the
    bf16 kernel gives them) are the same bits."""
    W = _clean(8, 2080, seed=9)
    W[1, 17] = float("inf"); W[2, 900] = float("nan"); W[6, 2079] = float("-inf"); W[5, 0] = 0.0
    _case(W, HEAD, EPI_NONE, seed=9, flagged=[False, False], min_slots=4, finite=False)


# ------------------------------------------------------------------------------------------------ 5. a small engine
def _four_steps(eng, graph):
    """Four greedy steps after a 40-token prefill -> (ids, logits per step, hidden state of the last step, K cache, V cache)."""
    from emu_amd import ops
    from emu_amd.llama import GreedyState
    dev = eng.device
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(1, 40, eng.cfg.hidden_size, generator=g) * 0.1).to(BF16).to(dev)
    hidden, kstart, next_pos = eng.prefill(x, torch.ones(1, 40, dtype=torch.long), eng.kv_capacity(40 + 4 + 8))
    cur = ops.argmax(eng.logits(hidden[:, -1, :].contiguous()), suppress_id=2)
    out = torch.zeros(4 + 2, 1, device=dev, dtype=torch.int32)
    st = GreedyState(eng, 1, cur, next_pos, 40, kstart, out)
    lg = []
    for _ in range(4):
        (st.step_graph if graph else st.step)()
        lg.append(st.logits.clone())
    torch.cuda.synchronize()
    return out.clone(), torch.stack(lg), st.hidden.clone(), eng.kcache.clone(), eng.vcache.clone()


def _same(a, b):
    assert torch.equal(a[0], b[0])
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(bits(x), bits(y))


def test_small_engine_on_12_bits_13_bits_and_bf16():
    """tests/test_gpu_bf16_pack.py's engine under the block-kernel-only tune bit, where o_proj and down take the preload form in both
    layers: four greedy steps on bf16, on 13-bit sets and on 12-bit sets give the same ids, logits, hidden state and KV cache, eager
    and from a hipGraph; the GEMV profiler's bytes say the 12-bit twins are what ran."""
    from emu_amd import bf16pack
    eng = _engine()
    keys = ["0.wdown", "0.wo", "1.wdown", "1.wo"]
    with _Tune(BLOCK_ONLY):
        ref = {graph: _four_steps(eng, graph) for graph in (False, True)}
        bytes_off, launches = _gemv_bytes(eng, 2)
        assert eng.pack_bf16(tune=BLOCK_ONLY)[0] == 4 and sorted(eng._pack) == keys and not any("patch" in v for v in eng._pack.values())
        eng.use_bf16_pack(True)
        on13 = {graph: _four_steps(eng, graph) for graph in (False, True)}
        bytes_13, _ = _gemv_bytes(eng, 2)
        eng._drop_bf16_pack(keys)
        assert not eng._pack
        n, nbytes = eng.pack_bf16(tune=BLOCK_ONLY, bits12=True)
        assert n == 4 and sorted(eng._pack) == keys and all("patch" in v and v["flagged"] == 0 for v in eng._pack.values())
        sets12 = sum(bf16pack.packed_bytes12(*v["shape"], 2) for v in eng._pack.values())
        assert nbytes == sets12 == sum(eng._set_bytes(v) for v in eng._pack.values())
        full = 2 * 2 * (256 * 256 + 256 * 512)                                              # the four matrices as bf16
        eng.use_bf16_pack(False)
        base = eng.weight_bytes_per_token()
        eng.use_bf16_pack(True)
        assert eng.weight_bytes_per_token() == base - full + sets12
        on12 = {graph: _four_steps(eng, graph) for graph in (False, True)}
        bytes_12, launches_12 = _gemv_bytes(eng, 2)
        assert launches_12 == launches
        assert bytes_off - bytes_12 == pytest.approx(2 * (full - sets12)) and bytes_12 < bytes_13 < bytes_off
        eng.use_bf16_pack_wide(True)                                   # the few-row twin reads 13-bit sets only: the sets are repacked
        assert sorted(eng._pack) == keys and not any("patch" in v for v in eng._pack.values())
        wide = _four_steps(eng, False)
        bytes_wide, _ = _gemv_bytes(eng, 2)
        assert bytes_wide == bytes_13
        eng.use_bf16_pack_wide(False)
    for graph in (False, True):
        _same(on13[graph], ref[graph])
        _same(on12[graph], ref[graph])
    _same(ref[False], ref[True])
    _same(wide, ref[False])


# ------------------------------------------------------------------------------------------------ 6. one true-shape layer and a head
def test_true_shape_layer_and_head_on_12_bit_sets():
    """One layer at 6656 / 52 heads / 17920 and a vocabulary of 8192, one cached decode row: qkv and gate/up (head form), o_proj
    (preload form), down (single round trip) and the lm_head (head form, through the head's own setter) all hold 12-bit sets; hidden
    state, the appended K / V rows and the logits are the bits of the run with the stream off, and the GEMV profiler prices the five
    launches at their 12-bit sets.  Then five rows with the library's few-row switch on: a 12-bit set is not offered to that twin,
    so the step runs the bf16 kernels and gives the bits of the switch off."""
    import ctypes as C
    from emu_amd import synth
    from emu_amd._lib import check, lib
    from emu_amd.conf.emu_conf import LlamaCfg
    from emu_amd.llama import EmuHipContext, LlamaEngine
    cfg = LlamaCfg(hidden_size=6656, intermediate_size=17920, num_attention_heads=52, num_hidden_layers=1)
    dev = torch.device("cuda", 0)
    eng = LlamaEngine(cfg, 8192, EmuHipContext(dev, 0, 1))
    eng.load_weights(synth.iter_synth(synth.llama_param_shapes(cfg, 8192), seed=1, device=dev, dtype=BF16))
    assert eng.bf16_pack_on and sorted(eng._pack) == ["0.wdown", "0.wo"]                          # the engine's own default
    assert eng.pack_bf16(head_form=True, bits12=True)[0] == 3
    keys = ["0.wqkv", "0.wo", "0.wgu", "0.wdown", "lm_head"]
    assert sorted(eng._pack) == sorted(keys) and [eng._pack[k]["rows"] for k in keys] == [4, 2, 4, 2, 4]
    # (of the thousands of row groups of a true-shape matrix a few reach 9 misses -- about 4 of down's 3328 -- and are flagged: those
    # stream their bf16 rows; the share stays far under the rule's break-even of one group in 16)
    from emu_amd import bf16pack
    for k in keys:
        p = eng._pack[k]
        G = -(-p["shape"][0] // p["rows"])
        assert "patch" in p and bf16pack.set_bits(p["flagged"], G, p["rows"], p["shape"][1]) == 12 and 100 * p["flagged"] < G, k
    assert all(int((eng._pack[k]["patch"] != -1).sum()) > 100 for k in keys)                     # the weight law's misses are there
    L = lib()
    g = torch.Generator().manual_seed(2)
    eng.alloc_kv(1, 64)
    kv0 = (torch.randn(2, 1, 1, 52, 64, 128, generator=g) * 0.5).to(BF16).to(dev)
    x = (torch.randn(1, 6656, generator=g) * 0.5).to(BF16).to(dev)
    x5 = (torch.randn(5, 6656, generator=g) * 0.5).to(BF16).to(dev)
    pos = torch.tensor([63], device=dev, dtype=torch.int32)
    at = torch.tensor([59], device=dev, dtype=torch.int32)
    kstart = torch.zeros(1, device=dev, dtype=torch.int32)

    def one_row():
        eng.kcache.copy_(kv0[0]); eng.vcache.copy_(kv0[1])
        check(L.emu_profile_gemv(1), "emu_profile_gemv")
        try:
            h = eng.decode_embeds(x, pos, 63, kstart)
            lg = eng.logits(h)
            torch.cuda.synchronize()
            ms, wb, nl = C.c_double(), C.c_double(), C.c_long()
            check(L.emu_profile_gemv_read(C.byref(ms), C.byref(wb), C.byref(nl)), "emu_profile_gemv_read")
        finally:
            L.emu_profile_gemv(0)
        return (h.clone(), lg.clone(), eng.kcache[0, 0, :, 63].clone(), eng.vcache[0, 0, :, 63].clone()), wb.value, nl.value

    def five_rows():
        eng.kcache.copy_(kv0[0]); eng.vcache.copy_(kv0[1])
        h = eng.forward_chunk(x5.clone(), 1, 5, at, at, kstart, 64)
        torch.cuda.synchronize()
        return h.clone(), eng.kcache[0, 0, :, 59:64].clone(), eng.vcache[0, 0, :, 59:64].clone()

    on, bytes_on, n_on = one_row()
    eng.use_bf16_pack(False)
    off, bytes_off, n_off = one_row()
    shapes = {k: tuple(eng._pack[k]["shape"]) for k in keys}
    assert n_on == n_off == 5
    assert bytes_off == sum(2 * n * k for n, k in shapes.values())
    assert bytes_on == sum(eng._set_bytes(eng._pack[k]) for k in keys)                           # the 12-bit twins are what ran
    assert bool(torch.isfinite(on[0].float()).all()) and bool(torch.isfinite(on[1].float()).all())
    for a, b in zip(on, off):
        assert torch.equal(bits(a), bits(b))
    want5 = five_rows()
    eng.use_bf16_pack(True)
    check(L.emu_llama_use_bf16_pack_wide(eng.handle, 1), "emu_llama_use_bf16_pack_wide")       # the library's switch alone: the sets stay 12-bit
    try:
        got5 = five_rows()
    finally:
        check(L.emu_llama_use_bf16_pack_wide(eng.handle, 0), "emu_llama_use_bf16_pack_wide")
    assert all("patch" in eng._pack[k] for k in keys)
    for a, b in zip(got5, want5):
        assert torch.equal(bits(a), bits(b))

