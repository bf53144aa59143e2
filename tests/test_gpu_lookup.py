"""GPU: prompt-lookup speculative greedy decoding -- the chunk forward of the engine, the selection kernels (csrc/lookup.hip)
against their specification (emu_amd/speculate.py), and the device loop (``LlamaEngine.lookup_generate``) against plain greedy
search on the tiny fixtures.

The loop tests compare ids with ``greedy_generate``'s.  Both are greedy, but the chunk step runs the few-row weight streams and
the one-row step does not, so they may differ where a top-2 logit margin is inside bf16 rounding.  PRECONDITION, asserted: along
the plain greedy path of every prompt that is compared, every step's top-2 logit margin is at least 0.08 (``lookup_cases.MARGIN``,
the project's divergence threshold, tests/test_gpu_fp4_gemm.py).  The screen runs on the CPU through tests/fake_engine.py the way
tests/test_host_logic.py::test_product_beam_modes_on_margin_fixtures screens this very fixture (fp32 arithmetic on the fixture's
weights as loaded); a row of ``pen_ids`` that does not satisfy it is not compared (no step of a compared row is skipped), and at
least one row must remain.  Under the fp8 stream the screen runs on the fp8-dequantised weights (tests/test_gpu_fp8.py's
``fake_quant``)."""
import functools

import numpy as np
import pytest
import torch

from emu_amd import speculate
from tests import lookup_cases as lc
from tests import tiny

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
MAX_NEW = 8
# the b5 prompt: its greedy output first repeats at index 6, so the first draft the lookup can make is the id at index 7, which is
# row 1 of the step that emits index 7 -- with 8 new ids the specification itself predicts that no draft is ever accepted
# (speculate.simulate: 7 steps for 7 ids).  12 is where the repeated run ends: the drafts inside it are accepted.
MAX_NEW_B5 = 12


def _t(a):
    return torch.from_numpy(np.asarray(a))


def rel_err(got, want):
    got, want = got.float().cpu(), want.float().cpu()
    return float((got - want).norm() / want.norm().clamp_min(1e-12))


@pytest.fixture(scope="module")
def model(golden_dir):
    """emu_amd.EmuModel (HIP) on the margin fixture + the oracle's weights, configuration and the fixture."""
    from emu_amd import EmuModel, TextDecoderCfg
    z = tiny.load(golden_dir, "generate_margin_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    m = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda")
    m.load_state_dict(W, strict=True)
    return m, W, tiny.oracle_cfg(v, l, vocab), z, l, vocab


# ------------------------------------------------------------------------------------------------ 1. the chunk forward
@pytest.mark.parametrize("B", [1, 2])
def test_forward_chunk_on_top_of_the_cache(model, B):
    """prefill(S = 24), then ONE chunk forward of T = 5 rows per batch element on top == rows 24..28 of prefill(S = 29); B = 2 with
    one row left-padded.  The bound is test_continuation_forward_on_top_of_the_cache's (tests/test_gpu_scoring.py)."""
    m, _, cfg, *_ = model
    lm = m.decoder.lm
    g = torch.Generator().manual_seed(5)
    S, n, H = 24, 5, cfg.llama.hidden
    x = (torch.randn(B, S + n, H, generator=g) * 0.5).to(BF16).cuda()
    mask = torch.ones(B, S + n, dtype=torch.long)
    if B > 1:
        mask[1, :5] = 0
    full, _, _ = lm.prefill(x, mask)
    want = full[:, S:, :].clone()
    _, kstart, pos = lm.prefill(x[:, :S].contiguous(), mask[:, :S])
    hid = x[:, S:, :].reshape(B * n, H).contiguous().clone()
    slot0 = torch.full((B,), S, dtype=torch.int32, device="cuda")
    lm.forward_chunk(hid, B, n, pos, slot0, kstart, ctx=S + n)
    e = rel_err(hid.view(B, n, H), want)
    print(f"chunk forward B={B} vs prefill rows: {e:.3e}")
    assert e < 1.5e-2


def test_forward_chunk_refusals(model):
    m, _, cfg, *_ = model
    lm = m.decoder.lm
    H = cfg.llama.hidden
    x = torch.zeros(1, 24, H, dtype=BF16, device="cuda")
    _, kstart, pos = lm.prefill(x, torch.ones(1, 24, dtype=torch.long))
    slot0 = torch.full((1,), 24, dtype=torch.int32, device="cuda")
    for T in (1, 9):
        with pytest.raises(ValueError, match="T in 2..8"):
            lm.forward_chunk(torch.zeros(T, H, dtype=BF16, device="cuda"), 1, T, pos, slot0, kstart, ctx=40)
    with pytest.raises(ValueError, match="B \\* T <= 16"):
        lm.forward_chunk(torch.zeros(24, H, dtype=BF16, device="cuda"), 3, 8, pos, slot0, kstart, ctx=40)
    hid = torch.zeros(4, H, dtype=BF16, device="cuda")
    from emu_amd import ops
    from emu_amd._lib import lib
    ws = lm._workspace_chunk(2, 4)

    def direct(h, B, p, s, ks):                                            # the library's own refusal, past the Python checks
        return lib().emu_llama_forward_chunk(lm.handle, h.data_ptr(), B, 4, p.data_ptr(), s.data_ptr(), ks.data_ptr(), None, 40,
                                             ws.data_ptr(), ws.numel(), ops.stream(lm.device))
    try:
        _, ks2, pos2 = lm.prefill(torch.zeros(2, 24, H, dtype=BF16, device="cuda"), torch.ones(2, 24, dtype=torch.long))
        slot2, hid2 = torch.full((2,), 24, dtype=torch.int32, device="cuda"), torch.zeros(8, H, dtype=BF16, device="cuda")
        lm.set_kv_share(2, 8)
        with pytest.raises(ValueError, match="shared-prefix"):
            lm.forward_chunk(hid2, 2, 4, pos2, slot2, ks2, ctx=40)
        assert direct(hid2, 2, pos2, slot2, ks2) == -22
    finally:
        lm.set_kv_share(0, 0)
    _, kstart, pos = lm.prefill(x, torch.ones(1, 24, dtype=torch.long))
    try:
        lm.set_decode_fused(1)
        with pytest.raises(ValueError, match="fused decode"):
            lm.forward_chunk(hid, 1, 4, pos, slot0, kstart, ctx=40)
        assert direct(hid, 1, pos, slot0, kstart) == -22
    finally:
        lm.set_decode_fused(0)
    with pytest.raises(ValueError, match="ctx out of range"):              # the library's own -22, with its message
        lm.forward_chunk(hid, 1, 4, pos, slot0, kstart, ctx=lm.s_max + 1)


# ------------------------------------------------------------------------------------------------ 2. the selection kernels
V = 32274
EOS = 2


def _spec_select(logits, cur, st, pos0, slot0, ctx, out_ids, hist, k, max_ngram, max_new, min_len, stop_on_eos, drafts):
    """One call of the selection on CPU copies of the state, by emu_amd/speculate.py."""
    cur, st, out_ids, hist = cur.clone(), st.clone(), out_ids.clone(), hist.clone()
    step, fin, nd, hl = (int(t) for t in st[:4])
    if step >= max_new or fin:
        return cur, st, pos0, slot0, ctx, out_ids, hist
    a = speculate.row_argmax(logits, step, min_len, EOS)
    n_emit, fin = speculate.accept(cur[1:].tolist(), nd, a, step, max_new, min_len, EOS, stop_on_eos)
    for i in range(n_emit):
        out_ids[step + i] = a[i]
        hist[hl + i] = a[i]
    now, L = step + n_emit, hl + n_emit
    d = []
    if not fin:
        d = drafts[now].tolist() if drafts is not None else speculate.lookup_draft(hist[:L].tolist(), k, max_ngram)
        cur[0] = a[n_emit - 1]
        cur[1:] = torch.tensor(d + [0] * (k - len(d)), dtype=torch.int32)
    st[:6] = torch.tensor([now, int(fin), len(d), L, int(st[4]) + 1, int(st[5]) + n_emit], dtype=torch.int32)
    return cur, st, pos0 + n_emit, slot0 + n_emit, ctx + n_emit, out_ids, hist


@pytest.mark.parametrize("T", [2, 5, 8])
def test_select_kernels_against_the_specification(T):
    """Random bf16 logits [T, 32274] whose arg-maxes are planted (some rows agree with the draft, some not; EOS on top in some rows,
    below and above min_len), low-entropy histories, with the lookup and with a table of drafts, stop_on_eos on and off, and calls
    at / past the end: every word of the state equals the specification's."""
    from emu_amd import ops
    k, max_new, cap = T - 1, 24, 96
    g = torch.Generator().manual_seed(900 + T)
    ri = lambda lo, hi: int(torch.randint(lo, hi, (1,), generator=g))
    n_cases = 0
    for case in range(40):
        logits = torch.randn(T, V, generator=g).to(BF16)
        max_ngram, min_len, stop = ri(1, 4), ri(0, 6), case % 5 != 0
        use_table = case % 3 == 0
        hl, step = ri(2, 40), ri(1, max_new + (2 if case % 8 == 7 else 0))
        fin = int(case % 10 == 9)
        hist = torch.zeros(cap, dtype=torch.int32)
        hist[:hl] = torch.randint(3, 3 + ri(2, 5), (hl,), generator=g).to(torch.int32)      # few distinct ids: n-grams repeat
        nd = ri(0, k + 1)
        cur = torch.zeros(T, dtype=torch.int32)
        cur[0] = hist[hl - 1]
        cur[1:1 + nd] = torch.randint(3, 8, (nd,), generator=g).to(torch.int32)
        agree = ri(0, T + 1)                                 # rows 0 .. agree - 1 answer the draft (row k has none: a small id)
        for i in range(T):
            top = int(cur[1 + i]) if i < agree and i < nd else ri(3, 8)
            if case % 4 == 1 and i == ri(0, T):
                top = EOS
            logits[i, top] = 9.0
            if case % 7 == 3:
                logits[i, EOS] = 9.0                         # a tie with EOS: the lower index wins unless suppressed
        drafts = torch.randint(3, 8, (max_new, k), generator=g).to(torch.int32) if use_table else None
        st = torch.tensor([step, fin, nd, hl, ri(0, 9), ri(0, 30), 0, 0], dtype=torch.int32)
        pos0, slot0, ctx = ri(5, 50), ri(50, 90), ri(90, 99)
        out_ids = torch.full((max_new,), -5, dtype=torch.int32)
        want = _spec_select(logits.float(), cur, st, pos0, slot0, ctx, out_ids, hist, k, max_ngram, max_new, min_len, stop, drafts)
        dev = [t.cuda() for t in (cur, st, torch.tensor([pos0], dtype=torch.int32), torch.tensor([slot0], dtype=torch.int32),
                                  torch.tensor([ctx], dtype=torch.int32), out_ids, hist)]
        for rep in range(2):                                 # a second call goes on from the first one's state
            amax = ops.lookup_select(logits.cuda(), *dev, max_ngram, max_new, min_len, EOS, stop,
                                     drafts=None if drafts is None else drafts.cuda())
            torch.cuda.synchronize()
            got = [t.cpu() for t in dev]
            names = ("cur", "st", "pos0", "slot0", "ctx", "out_ids", "hist")
            for name, gt, wt in zip(names, got, want):
                wt = wt if isinstance(wt, torch.Tensor) else torch.tensor([wt], dtype=torch.int32)
                assert torch.equal(gt, wt), (T, case, rep, name, gt.tolist(), wt.tolist())
            if rep == 0 and step < max_new and not fin:
                assert amax.cpu().tolist() == speculate.row_argmax(logits.float(), step, min_len, EOS)
            want = _spec_select(logits.float(), want[0], want[1], *want[2:5], want[5], want[6], k, max_ngram, max_new, min_len, stop,
                                drafts)
            n_cases += 1
    assert n_cases == 80


# ------------------------------------------------------------------------------------------------ 3. the loop
@functools.lru_cache(maxsize=None)
def _fixture_cpu():
    import os
    z = tiny.load(os.path.join(os.path.dirname(__file__), "golden"), "generate_margin_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    return z, l, vocab, W, tiny.oracle_cfg(v, l, vocab)


@functools.lru_cache(maxsize=None)
def _screen(name, b, min_len, eos, fp8=False, max_new=MAX_NEW):
    """(greedy ids on the CPU, smallest top-2 margin) of row b of the fixture's prompts ``name``, computed once."""
    from oracle import emu2_ref as R
    z, l, vocab, W, cfg = _fixture_cpu()
    if fp8:
        from tests.test_gpu_fp8 import fake_quant
        W = R.bf16_round(W)
        W = {k: fake_quant(t) if k.startswith("decoder.lm.") and t.dim() == 2 and "embed_tokens" not in k else t for k, t in W.items()}
    ids, mask = _t(z[name + "_ids"])[b:b + 1], _t(z[name + "_mask"])[b:b + 1]
    x = R.embed_tokens(ids, W)
    if name == "b5":
        e = R.encode_image(_t(z["image"]), W, cfg)
        x = R.scatter_image_embeds(x, ids, torch.nn.functional.linear(e.reshape(-1, e.shape[-1]), W["project_up.weight"]))
    return lc.cpu_greedy(l, vocab, W, cfg.llama, x, mask, max_new, min_len, eos)


def _kept_rows(name, min_len, eos=None, fp8=False, max_new=MAX_NEW):
    """The rows of ``name`` whose whole greedy path keeps the margin; asserted non-empty."""
    from oracle import emu2_ref as R
    z = _fixture_cpu()[0]
    rows = []
    for b in range(z[name + "_ids"].shape[0]):
        e = R.EOS_ID if eos is None else eos(b)
        _, margin = _screen(name, b, min_len, e, fp8, max_new)
        print(f"{name} row {b} min_len {min_len} eos {e}: smallest top-2 margin on the CPU {margin:.3f}")
        if margin >= lc.MARGIN:
            rows.append(b)
    assert rows, f"no row of {name} keeps a top-2 margin of {lc.MARGIN} along its greedy path"
    return rows


def _prompt(model, name, b):
    """(embeds [1, S, H] on the device, mask, ids) of row b, as EmuModel.generate_ids prepares them."""
    m, _, _, z, *_ = model
    ids, mask = _t(z[name + "_ids"])[b:b + 1], _t(z[name + "_mask"])[b:b + 1]
    img = _t(z["image"]).cuda() if name == "b5" else None
    x = m._prompt_embeds(ids, img, m.n_query)
    return x.view(1, ids.shape[1], -1), mask, ids


def _lookup(lm, x, mask, ids, k, min_len, eos, graph, drafts=None, max_ngram=2, max_new=MAX_NEW):
    stats = {}
    out = lm.lookup_generate(x, mask, ids, max_new, k, max_ngram=max_ngram, min_len=min_len, eos_id=eos, use_graph=graph, drafts=drafts,
                             stats=stats)
    return out.cpu().tolist(), stats


@pytest.mark.parametrize("min_len", [1, 3])
@pytest.mark.parametrize("k", [1, 4, 7])
def test_forced_acceptance_equals_greedy_search(model, k, min_len):
    """Drafts that are right for their first j entries and wrong from there on, j = 0 (none accepted) .. k (all accepted): the ids
    are greedy_generate's, ``steps_run`` is what the specification predicts from those ids, the captured graph gives what the eager
    steps give, and a second call under the same signature replays the graph the first one captured."""
    from oracle import emu2_ref as R
    m, _, _, z, l, vocab = model
    lm = m.decoder.lm
    for b in _kept_rows("pen", min_len):
        x, mask, ids = _prompt(model, "pen", b)
        want = lm.greedy_generate(x, mask, MAX_NEW, min_len, eos_id=R.EOS_ID).cpu().tolist()
        g = want[0]
        assert g == _screen("pen", b, min_len, R.EOS_ID)[0], "the engine's greedy ids are the CPU screen's"
        prompt = ids[0][mask[0].bool()].tolist()
        for j in range(k + 1):
            drafts = lc.forced_drafts(g, k, MAX_NEW, j, vocab)
            sim, steps = speculate.simulate(lc.greedy_rows(g), g[0], prompt, k, 2, MAX_NEW, min_len, R.EOS_ID, drafts=drafts)
            assert sim == g
            got, stats = _lookup(lm, x, mask, ids, k, min_len, R.EOS_ID, False, drafts)
            assert got == want, (b, j, got, want)
            assert stats == dict(steps_run=steps, tokens_emitted=len(g) - 1), (b, j, stats, steps)
            got_g, stats_g = _lookup(lm, x, mask, ids, k, min_len, R.EOS_ID, True, drafts)
            captured = lm._loop_states["lookup"][1]["captured"]
            graph = captured.graph
            assert graph is not None
            again, stats_a = _lookup(lm, x, mask, ids, k, min_len, R.EOS_ID, True, drafts)
            assert lm._loop_states["lookup"][1]["captured"] is captured and captured.graph is graph, "the second call captured anew"
            assert got_g == again == want and stats_g == stats_a == stats, (b, j, got_g, again, stats_g, stats_a)
        if j == k and k >= 1:
            assert stats["steps_run"] == -(-(MAX_NEW - 1) // (k + 1))          # all accepted: k + 1 ids per step


def test_real_lookup_drafts_on_a_repeating_output(model):
    """The b5 prompt's greedy output repeats an id, so the lookup finds drafts that are accepted: more ids than steps; ids, step
    count and graph replay as above.  MAX_NEW_B5 new ids (see there)."""
    from oracle import emu2_ref as R
    m, *_ = model
    lm = m.decoder.lm
    n = MAX_NEW_B5
    assert _kept_rows("b5", 1, max_new=n) == [0]
    x, mask, ids = _prompt(model, "b5", 0)
    want = lm.greedy_generate(x, mask, n, 1, eos_id=R.EOS_ID).cpu().tolist()
    g = want[0]
    assert g == _screen("b5", 0, 1, R.EOS_ID, max_new=n)[0]
    assert len(set(g)) < len(g), "the fixture's greedy output repeats"
    prompt = ids[0][mask[0].bool()].tolist()
    for k in (1, 4, 7):
        sim, steps = speculate.simulate(lc.greedy_rows(g), g[0], prompt, k, 2, n, 1, R.EOS_ID)
        assert sim == g
        got, stats = _lookup(lm, x, mask, ids, k, 1, R.EOS_ID, False, max_new=n)
        got_g, stats_g = _lookup(lm, x, mask, ids, k, 1, R.EOS_ID, True, max_new=n)
        print(f"b5, k = {k}: {stats}")
        assert got == got_g == want, (k, got, got_g, want)
        assert stats == stats_g == dict(steps_run=steps, tokens_emitted=len(g) - 1)
        assert stats["tokens_emitted"] > stats["steps_run"]


@pytest.mark.parametrize("min_len", [1, 3])
def test_eos_ends_the_loop_and_replays_change_nothing(model, min_len):
    """The third greedy id declared EOS (with min_len = 3 it is emitted at index 2 < min_len, where it is suppressed, so the path
    is screened anew): output and padding equal greedy_generate's; the steps the loop replays between the EOS and the host's next
    look (every LOOKUP_POLL steps) change no state -- the counters and the ids behind the EOS."""
    from oracle import emu2_ref as R
    m, _, _, z, l, vocab = model
    lm = m.decoder.lm
    third = lambda b: _screen("pen", b, min_len, R.EOS_ID)[0][2]
    for b in _kept_rows("pen", min_len, eos=third):
        eos = third(b)
        x, mask, ids = _prompt(model, "pen", b)
        want = lm.greedy_generate(x, mask, MAX_NEW, min_len, eos_id=eos).cpu().tolist()
        g = _screen("pen", b, min_len, eos)[0]
        assert want[0] == g and (g[-1] == eos or len(g) == MAX_NEW)
        prompt = ids[0][mask[0].bool()].tolist()
        for k, right in ((1, 0), (4, 4), (7, 2)):
            drafts = lc.forced_drafts(g, k, MAX_NEW, right, vocab)
            _, steps = speculate.simulate(lc.greedy_rows(g), g[0], prompt, k, 2, MAX_NEW, min_len, eos, drafts=drafts)
            for graph in (False, True):
                got, stats = _lookup(lm, x, mask, ids, k, min_len, eos, graph, drafts)
                assert got == want, (b, k, graph, got, want)
                assert stats == dict(steps_run=steps, tokens_emitted=len(g) - 1), (b, k, graph, stats, steps)
                raw = lm._loop_states["lookup"][1]["out_ids"].cpu().tolist()
                assert raw[:len(g)] == g and all(t == 32000 for t in raw[len(g):]), raw


def test_under_the_wide_fp8_stream(model):
    """``use_fp8(True, wide=True)``: the chunk step streams the fp8 set through the few-row kernel; compared with that mode's own
    greedy ids, screened on the fp8-dequantised weights."""
    from oracle import emu2_ref as R
    m, _, _, z, l, vocab = model
    lm = m.decoder.lm
    rows = _kept_rows("pen", 1, fp8=True)
    try:
        lm.use_fp8(True, wide=True)
        for b in rows:
            x, mask, ids = _prompt(model, "pen", b)
            want = lm.greedy_generate(x, mask, MAX_NEW, 1, eos_id=R.EOS_ID).cpu().tolist()
            g = want[0]
            for k, right in ((4, 4), (4, 1)):
                drafts = lc.forced_drafts(g, k, MAX_NEW, right, vocab)
                for graph in (False, True):
                    got, stats = _lookup(lm, x, mask, ids, k, 1, R.EOS_ID, graph, drafts)
                    assert got == want, (b, k, right, graph, got, want)
            print(f"fp8 wide, row {b}: {stats}")
    finally:
        lm.use_fp8(False)
