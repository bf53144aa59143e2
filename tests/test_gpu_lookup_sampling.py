"""GPU: prompt-lookup speculation together with sampling or a repetition penalty -- the selection kernel (csrc/sample.hip:
lookup_sample_kernel) against the one-row sampler it shares its body with, bit for bit, and against the specification
(``speculate.row_select``); the device loop (``LlamaEngine.lookup_generate(do_sample=..., repetition_penalty=...)``) against the
specification on the logits it chose from (``trace``), and against the one-row device loop
(``sample_generate(device_sampler=True)``) with the same uniforms.

The comparisons with the one-row loop carry PRECONDITIONS, asserted on the CPU through tests/fake_engine.py the way
``lookup_cases.cpu_greedy`` screens (the chunk step runs the few-row weight streams, the one-row step does not: a score difference
may move by up to ``lookup_cases.MARGIN`` between them).  A prompt row that fails its screen is not compared, no step of a compared
row is skipped, and at least one row must remain:

* penalised greedy (penalty 1.3): every step's top-2 margin of the PENALISED scores is at least MARGIN * 1.3 (a penalised negative
  score is the logit times the penalty, so a rounding difference of the logit grows by that factor).  On the CPU stand-in, at
  1.3: row 1 of the two ``pen`` rows keeps 0.123 >= 0.104 (row 0: 0.038); on the fp8-dequantised weights row 0 keeps 0.113 (row 1:
  0.092).  The penalty did not have to be lowered.
* sampling (temperature 1, top_k 2): at every step the kept pair is separated from the third score by at least MARGIN, and the
  screen builds the table of uniforms itself: every u is at least d = MARGIN / (4 * temperature) + DRAW_TOL away from the boundary
  between the two kept ids' intervals.  (The boundary is a logistic function of the score difference, whose slope is at most 1/4,
  and MARGIN bounds how far a score difference moves between the streams.)"""
import functools

import numpy as np
import pytest
import torch

from emu_amd import llama, sampling, speculate
from tests import lookup_cases as lc
from tests import tiny
from tests.test_gpu_lookup import _fixture_cpu, _prompt, _t
from tests.test_gpu_sampler import DRAW_TOL

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
MAX_NEW = 8
EOS, PAD = 2, 32000
DEMO = dict(do_sample=True, temperature=0.7, top_p=0.9)


@pytest.fixture(scope="module")
def model(golden_dir):
    """emu_amd.EmuModel (HIP) on the margin fixture, as tests/test_gpu_lookup.py makes it."""
    from emu_amd import EmuModel, TextDecoderCfg
    z = tiny.load(golden_dir, "generate_margin_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    m = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda")
    m.load_state_dict(W, strict=True)
    return m, W, tiny.oracle_cfg(v, l, vocab), z, l, vocab


# ------------------------------------------------------------------------------------------------ 4. the kernel
def _params(o, min_len):
    return llama.sample_params(o.get("do_sample", False), o.get("temperature"), o.get("top_k"), o.get("top_p"),
                               o.get("repetition_penalty", 1.0), EOS, min_len, EOS, PAD)


def _spec_select(picked, cur, st, pos0, slot0, ctx, out_ids, hist, k, max_ngram, max_new, min_len, stop_on_eos, drafts):
    """One call of the selection on CPU copies of the state by emu_amd/speculate.py, the rows' picked ids given."""
    cur, st, out_ids, hist = cur.clone(), st.clone(), out_ids.clone(), hist.clone()
    step, fin, nd, hl = (int(t) for t in st[:4])
    if step >= max_new or fin:
        return cur, st, pos0, slot0, ctx, out_ids, hist
    a = picked
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


def _one_row_picks(logits_dev, out_ids, cur, step, nd, params, uni_dev):
    """What ``ops.sample`` (emu_sample_bf16) returns for each chunk row i <= nd as ONE row with the materialised history of
    length step + i, step_dev = step + i and the same table of uniforms."""
    from emu_amd import ops
    picks = []
    for i in range(nd + 1):
        h = out_ids[:step].tolist() + cur[1:1 + i].tolist()
        hist = torch.tensor(h + [0], dtype=torch.int32).view(-1, 1).cuda()          # (one spare row: an empty history has a pointer)
        step_dev = torch.tensor([step + i], dtype=torch.int32, device="cuda")
        picks.append(int(ops.sample(logits_dev[i:i + 1], step_dev, params, hist=hist[:len(h) + 1], uniforms=uni_dev)[0]))
    return picks


KERNEL_OPTIONS = (dict(repetition_penalty=1.3), dict(DEMO), dict(do_sample=True, temperature=0.8, top_k=6, top_p=0.85, repetition_penalty=1.2))


@pytest.mark.parametrize("V", [37, 32274])
@pytest.mark.parametrize("T", [2, 5, 8])
def test_kernel_equals_the_one_row_sampler_and_the_specification(T, V):
    """Random bf16 logits [T, V]; ``step`` 0 .. 20 (the history all draft, mixed, mostly generated); few distinct ids, so draft and
    generated ids collide; the draft padded with id 0; an id >= V planted in the history; n_draft 0 .. k; min_len around step; greedy
    with a penalty, the demo's sampling, and sampling with top_k + top_p + penalty.  amax[i] for i <= n_draft is bit for bit the
    one-row sampler's id; the entries behind are not written; every word of the state equals the specification's; a second call
    goes on from the first; calls at / past the end and after ``finished`` change nothing."""
    from emu_amd import ops
    k, max_new, cap = T - 1, 24, 96
    g = torch.Generator().manual_seed(4100 + 10 * T + (V > 100))
    ri = lambda lo, hi: int(torch.randint(lo, hi, (1,), generator=g))
    n_live = n_sampled = n_outside = 0
    for case in range(18):
        o = KERNEL_OPTIONS[case % 3]
        logits = (torch.randn(T, V, generator=g) * 2.5).to(BF16)
        step = ri(0, 21) if case % 9 != 8 else max_new + ri(0, 2)
        fin = int(case % 9 == 7)
        min_len, stop, max_ngram = max(0, step + ri(-2, 4)), case % 5 != 0, ri(1, 4)
        use_table = case % 2 == 0
        hl = step + ri(1, 30)                                   # prompt ids, then the `step` generated ones
        out_ids = torch.full((max_new,), -5, dtype=torch.int32)
        n_gen = min(step, max_new)
        out_ids[:n_gen] = torch.randint(3, 8, (n_gen,), generator=g).to(torch.int32)
        if n_gen > 2:
            out_ids[ri(0, n_gen)] = V + 5                       # outside the vocabulary: ignored by the penalty
        hist = torch.zeros(cap, dtype=torch.int32)
        hist[:hl] = torch.randint(3, 7, (hl,), generator=g).to(torch.int32)
        hist[hl - n_gen:hl] = out_ids[:n_gen]
        nd = ri(0, k + 1)
        cur = torch.zeros(T, dtype=torch.int32)
        cur[0] = hist[hl - 1]
        cur[1:1 + nd] = torch.randint(3, 8, (nd,), generator=g).to(torch.int32)
        for i in range(min(nd, ri(0, T + 1))):                  # lift the draft id of the leading rows: some drafts are accepted
            logits[i, int(cur[1 + i])] = 12.0
        if case % 4 == 1:
            logits[ri(0, T), EOS] = 14.0
        drafts = torch.randint(0, 8, (max_new, k), generator=g).to(torch.int32) if use_table else None
        st = torch.tensor([step, fin, nd, hl, ri(0, 9), ri(0, 30), 0, 0], dtype=torch.int32)
        pos0, slot0, ctx = ri(5, 50), ri(50, 90), ri(90, 99)
        uni = torch.rand(max_new, generator=g, dtype=torch.float32)
        params = _params(o, min_len)
        spec_params = dict(o, suppress_id=EOS, min_len=min_len)
        lg_dev, uni_dev = logits.cuda(), uni.cuda().view(max_new, 1)
        state = (cur, st, pos0, slot0, ctx, out_ids, hist)
        dev = [t.cuda() for t in (cur, st, torch.tensor([pos0], dtype=torch.int32), torch.tensor([slot0], dtype=torch.int32),
                                  torch.tensor([ctx], dtype=torch.int32), out_ids, hist)]
        for rep in range(2):                                    # a second call goes on from the first one's state
            c_cur, c_st, _, _, _, c_out, _ = state
            s_now, f_now, nd_now = int(c_st[0]), int(c_st[1]), int(c_st[2])
            live = s_now < max_new and not f_now
            amax = torch.full((T,), -7, dtype=torch.int32, device="cuda")
            picks = _one_row_picks(lg_dev, c_out, c_cur, s_now, nd_now, params, uni_dev) if live else []
            ops.lookup_sample(lg_dev, *dev, max_ngram, max_new, min_len, EOS, params, uniforms=uni_dev if o.get("do_sample") else None,
                              stop_on_eos=stop, drafts=None if drafts is None else drafts.cuda(), amax=amax)
            torch.cuda.synchronize()
            got_amax = amax.cpu().tolist()
            if live:
                assert got_amax[:nd_now + 1] == picks, (T, V, case, rep, got_amax, picks)
                assert all(t == -7 for t in got_amax[nd_now + 1:]), (T, V, case, rep, got_amax)
                spec = speculate.row_select(logits.float(), c_out.tolist(), c_cur.tolist(), s_now, spec_params, uni)
                n_live += 1
                for i in range(nd_now + 1):
                    if not o.get("do_sample"):
                        assert picks[i] == spec[i], (T, V, case, rep, i, picks, spec)           # fp32 scores: the kernel's bit for bit
                        continue
                    # the fp32 specification's draw may differ only within the draw's tolerance of a boundary: the criterion is the
                    # fp64 interval of the picked id (tests/test_gpu_sampler.py)
                    h = [c_out[:s_now].tolist() + c_cur[1:1 + i].tolist()]
                    q = sampling.reference_probs(logits[i:i + 1], h, o.get("repetition_penalty", 1.0), EOS if s_now + i < min_len else None,
                                                 True, o.get("temperature"), o.get("top_k"), o.get("top_p"), dtype=torch.float64)
                    lo, hi = sampling.reference_intervals(q)
                    u = float(uni[min(s_now + i, max_new - 1)])
                    assert float(q[0, picks[i]]) > 0 and float(lo[0, picks[i]]) - DRAW_TOL <= u <= float(hi[0, picks[i]]) + DRAW_TOL
                    n_sampled += 1
                    n_outside += picks[i] != spec[i]
                picked = picks + [0] * (k - nd_now)
            else:
                assert got_amax == [-7] * T, "a call past the end or after finished writes nothing"
                picked = None
            state = _spec_select(picked, *state, k, max_ngram, max_new, min_len, stop, drafts)
            got = [t.cpu() for t in dev]
            for name, gt, wt in zip(("cur", "st", "pos0", "slot0", "ctx", "out_ids", "hist"), got, state):
                wt = wt if isinstance(wt, torch.Tensor) else torch.tensor([wt], dtype=torch.int32)
                assert torch.equal(gt, wt), (T, V, case, rep, name, gt.tolist(), wt.tolist())
    print(f"T={T} V={V}: {n_live} live calls, {n_sampled} sampled rows, {n_outside} where the fp32 specification draws a neighbour")
    assert n_live >= 16 and n_sampled >= 16


def test_kernel_refusals():
    from emu_amd import ops
    from emu_amd._lib import EmuHipError, SAMPLE_MAX_VOCAB
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda")
    state = lambda: (i32(3, 4), i32(1, 0, 1, 4, 0, 0, 0, 0), i32(5), i32(6), i32(7), torch.full((8,), -5, dtype=torch.int32, device="cuda"),
                     torch.zeros(16, dtype=torch.int32, device="cuda"))
    big = torch.zeros(2, SAMPLE_MAX_VOCAB + 1, dtype=BF16, device="cuda")
    for lg, o, uni in ((big, dict(repetition_penalty=1.3), None),
                       (torch.zeros(2, 40, dtype=BF16, device="cuda"), DEMO, None)):               # sampling without uniforms
        s = state()
        before = [t.clone() for t in s]
        with pytest.raises(EmuHipError, match="-22"):
            ops.lookup_sample(lg, *s, 2, 8, 1, EOS, _params(o, 1), uniforms=uni)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(s, before)), "refused: nothing launched"


# ------------------------------------------------------------------------------------------------ the CPU screens
@functools.lru_cache(maxsize=None)
def _cpu_walk(name, b, max_new, min_len, mode, fp8=False, penalty=1.3, seed=0):
    """The CPU stand-in's path of row b of the fixture's prompts ``name``.  mode "pen": penalised greedy search -> (ids, the
    smallest top-2 margin of the penalised scores, None, None).  mode "top2": temperature 1, top_k 2 -> (ids, the smallest gap
    between the kept pair and the third score, the table of uniforms the screen built, (coin steps, coins that picked the less
    probable id)); every u is at least d from the boundary between the two kept ids."""
    from oracle import emu2_ref as R
    from tests.fake_engine import FakeEngine
    z, l, vocab, W, cfg = _fixture_cpu()
    if fp8:
        from tests.test_gpu_fp8 import fake_quant
        W = R.bf16_round(W)
        W = {k: fake_quant(t) if k.startswith("decoder.lm.") and t.dim() == 2 and "embed_tokens" not in k else t for k, t in W.items()}
    ids, mask = _t(z[name + "_ids"])[b:b + 1], _t(z[name + "_mask"])[b:b + 1]
    x = R.embed_tokens(ids, W)
    eng = FakeEngine(l, vocab, W, cfg.llama)
    h, kstart, pos = eng.prefill(x.float(), mask, 64 + x.shape[1])
    S = x.shape[1]
    row, out, margin = h[:, -1, :], [], float("inf")
    d = lc.MARGIN / 4.0 + DRAW_TOL
    coin = torch.Generator().manual_seed(seed)
    uni, coins, minority = torch.full((max_new,), 0.5), 0, 0
    for i in range(max_new):
        lg = eng.logits(row)[:1].float()
        sup = R.EOS_ID if i < min_len else None
        if mode == "pen":
            s = sampling.reference_scores(lg, [out], penalty, sup)[0]
            t2 = s.topk(2)
            margin = min(margin, float(t2.values[0] - t2.values[1]))
            tok = int(t2.indices[0])
        else:
            s = sampling.reference_scores(lg, None, 1.0, sup)[0]
            t3 = s.topk(3)
            margin = min(margin, float(t3.values[1] - t3.values[2]))
            lo_id, hi_id = sorted(int(t) for t in t3.indices[:2])
            bnd = float(torch.softmax(s[[lo_id, hi_id]].double(), dim=0)[0])        # the lower id's interval is [0, bnd)
            if 2 * d <= bnd <= 1 - 2 * d:
                tok = (lo_id, hi_id)[int(torch.randint(0, 2, (1,), generator=coin))]
                coins += 1
                minority += (bnd < 0.5) == (tok == lo_id)
            else:
                tok = lo_id if bnd >= 0.5 else hi_id
            uni[i] = bnd / 2 if tok == lo_id else (1 + bnd) / 2
        out.append(tok)
        if tok == R.EOS_ID or i + 1 == max_new:
            break
        e = R.embed_tokens(torch.tensor([[tok]]), W)[:, 0].float().clone()
        row = eng.forward(e, 1, 1, pos + i, torch.tensor([S + i]), kstart, S + i + 1)
    return out, margin, (uni if mode == "top2" else None), (coins, minority)


def _rows_kept(mode, need, min_len=1, fp8=False, **kw):
    z = _fixture_cpu()[0]
    rows = []
    for b in range(z["pen_ids"].shape[0]):
        ids, margin, _, coins = _cpu_walk("pen", b, MAX_NEW, min_len, mode, fp8, **kw)
        print(f"pen row {b} ({mode}, fp8 {fp8}): CPU path {ids}, smallest margin {margin:.3f} (needs {need:.3f}), coins {coins}")
        if margin >= need:
            rows.append(b)
    assert rows, f"no row of the pen prompts keeps the margin {need}"
    return rows


def _sampled_lookup(lm, x, mask, ids, k, graph, drafts=None, trace=None, min_len=1, max_new=MAX_NEW, **opts):
    stats = {}
    out = lm.lookup_generate(x, mask, ids, max_new, k, min_len=min_len, eos_id=EOS, use_graph=graph, drafts=drafts, stats=stats,
                             trace=trace, **opts)
    return out.cpu().tolist(), stats


# ------------------------------------------------------------------------------------------------ 5. the loop on its own logits
@pytest.mark.parametrize("k", [1, 4, 7])
def test_loop_follows_the_specification_on_its_own_logits(model, k):
    """Sampling at temperature 0.7 / top_p 0.9 / penalty 1.2, eager, traced; forced draft tables from a first free run, right for
    j in {0, 2, k} entries.  For every traced step and every emitted row: the id has positive probability and its fp64 interval
    (the row's history = the generated ids, then the draft ids before the row) contains the row's uniform within DRAW_TOL; the
    number emitted is ``speculate.accept``'s; ``stats`` equals the sums over the trace.  Graph replay: the same ids and stats; a
    second call replays the graph the first captured."""
    m, _, _, z, l, vocab = model
    lm = m.decoder.lm
    opts = dict(DEMO, repetition_penalty=1.2)
    uni = torch.rand(MAX_NEW, generator=torch.Generator().manual_seed(50 + k), dtype=torch.float32)
    x, mask, ids = _prompt(model, "pen", 0)
    free, _ = _sampled_lookup(lm, x, mask, ids, k, False, uniforms=uni, **opts)
    g = free[0]
    assert len(g) == MAX_NEW or g[-1] == EOS
    for j in sorted({0, min(2, k), k}):
        drafts = lc.forced_drafts(g, k, MAX_NEW, j, vocab)
        trace = []
        got, stats = _sampled_lookup(lm, x, mask, ids, k, False, drafts, trace, uniforms=uni, **opts)
        out = got[0]
        assert stats == dict(steps_run=len(trace), tokens_emitted=sum(r["n_emit"] for r in trace)), (j, stats)
        assert 1 + stats["tokens_emitted"] == len(out)
        at = 1
        for r in trace:
            step, nd, cur, n_emit = r["step"], r["n_draft"], r["cur"], r["n_emit"]
            assert step == at and cur[0] == out[step - 1] and cur[1:1 + nd] == drafts[step][:nd].tolist() and r["logits"].shape == (k + 1, vocab)
            emitted = out[step:step + n_emit]
            for i, tok in enumerate(emitted):
                q = sampling.reference_probs(r["logits"][i:i + 1], [out[:step] + cur[1:1 + i]], 1.2, EOS if step + i < 1 else None, True,
                                             0.7, None, 0.9, dtype=torch.float64)
                lo, hi = sampling.reference_intervals(q)
                u = float(uni[min(step + i, MAX_NEW - 1)])
                print(f"k={k} j={j} step {step} row {i}: id {tok}, u {u:.6f}, interval {float(lo[0, tok]):.6f} .. {float(hi[0, tok]):.6f}")
                assert float(q[0, tok]) > 0, (j, step, i)
                assert float(lo[0, tok]) - DRAW_TOL <= u <= float(hi[0, tok]) + DRAW_TOL, (j, step, i)
            want_emit, _ = speculate.accept(cur[1:], nd, emitted + [-1] * (k + 1), step, MAX_NEW, 1, EOS)
            assert n_emit == want_emit, (j, step, n_emit, want_emit)
            at += n_emit
        assert at == len(out)
        got_g, stats_g = _sampled_lookup(lm, x, mask, ids, k, True, drafts, uniforms=uni, **opts)
        captured = lm._loop_states["lookup_sample"][1]["captured"]
        graph = captured.graph
        assert graph is not None
        again, stats_a = _sampled_lookup(lm, x, mask, ids, k, True, drafts, uniforms=uni, **opts)
        assert lm._loop_states["lookup_sample"][1]["captured"] is captured and captured.graph is graph, "the second call captured anew"
        assert got_g == again == got and stats_g == stats_a == stats, (j, got_g, again, got, stats_g, stats_a, stats)
    assert "lookup" not in lm._loop_states or lm._loop_states["lookup"][1] is not lm._loop_states["lookup_sample"][1]


# ------------------------------------------------------------------------------------------------ 6. penalised greedy
PENALTY = 1.3


def _penalised_rows(fp8=False):
    return _rows_kept("pen", lc.MARGIN * PENALTY, fp8=fp8, penalty=PENALTY)


@pytest.mark.parametrize("k", [1, 4, 7])
def test_penalised_greedy_equals_the_one_row_device_loop(model, k):
    """``lookup_generate(do_sample=False, repetition_penalty=1.3)`` with forced drafts (j = 0 .. k) and with the real lookup's
    drafts gives the ids of ``sample_generate(do_sample=False, repetition_penalty=1.3, device_sampler=True)``, on the rows whose
    penalised top-2 margin is at least MARGIN * 1.3 at every step of the CPU path."""
    m, _, _, z, l, vocab = model
    lm = m.decoder.lm
    for b in _penalised_rows():
        x, mask, ids = _prompt(model, "pen", b)
        want = lm.sample_generate(x, mask, MAX_NEW, 1, do_sample=False, repetition_penalty=PENALTY, eos_id=EOS, device_sampler=True).cpu().tolist()
        g = want[0]
        assert g == _cpu_walk("pen", b, MAX_NEW, 1, "pen", penalty=PENALTY)[0], "the one-row device loop's ids are the CPU screen's"
        for j in range(k + 1):
            drafts = lc.forced_drafts(g, k, MAX_NEW, j, vocab)
            for graph in (False, True):
                got, stats = _sampled_lookup(lm, x, mask, ids, k, graph, drafts, repetition_penalty=PENALTY)
                assert got == want, (b, j, graph, got, want)
        assert stats["steps_run"] == -(-(len(g) - 1) // (k + 1))                   # j = k: all accepted, k + 1 ids per step
        got, stats = _sampled_lookup(lm, x, mask, ids, k, False, repetition_penalty=PENALTY)
        print(f"row {b}, k = {k}, the real lookup's drafts: {stats}")
        assert got == want, (b, got, want)


# ------------------------------------------------------------------------------------------------ 7. same uniforms, same sample
TOP2_SEED = 9                  # the coin's seed: the path it walks on row 0 keeps the kept pair 0.097 above the third score


def test_same_uniforms_same_sample_as_the_one_row_device_sampler(model):
    """Temperature 1, top_k 2: with the table of uniforms the CPU screen built, ``lookup_generate`` with forced drafts (j = 0, 2, k;
    k = 4), eager and replayed, emits the ids of ``sample_generate(device_sampler=True)`` with the same table."""
    m, _, _, z, l, vocab = model
    lm = m.decoder.lm
    k, opts = 4, dict(do_sample=True, temperature=1.0, top_k=2)
    compared = 0
    for b in _rows_kept("top2", lc.MARGIN, seed=TOP2_SEED):
        cpu_ids, _, uni, (coins, minority) = _cpu_walk("pen", b, MAX_NEW, 1, "top2", seed=TOP2_SEED)
        if coins < 2 or minority < 1:
            print(f"row {b}: {coins} coin steps, {minority} for the less probable id: not a sampled path, not compared")
            continue
        x, mask, ids = _prompt(model, "pen", b)
        want = lm.sample_generate(x, mask, MAX_NEW, 1, eos_id=EOS, device_sampler=True, uniforms=uni.view(-1, 1), **opts).cpu().tolist()
        assert want[0] == cpu_ids, "the one-row device sampler follows the CPU screen's path"
        for j in (0, 2, k):
            drafts = lc.forced_drafts(want[0], k, MAX_NEW, j, vocab)
            for graph in (False, True):
                got, _ = _sampled_lookup(lm, x, mask, ids, k, graph, drafts, uniforms=uni, **opts)
                assert got == want, (b, j, graph, got, want)
        compared += 1
    assert compared >= 1, "no screened row took the coin at two steps and the less probable id at one: it did not sample"


# ------------------------------------------------------------------------------------------------ 8. the wide fp8 stream
def test_penalised_greedy_under_the_wide_fp8_stream(model):
    """``use_fp8(True, wide=True)``: case 6 (k = 4, j in {1, 4}) against that mode's own one-row ids, screened on the
    fp8-dequantised weights."""
    m, _, _, z, l, vocab = model
    lm = m.decoder.lm
    rows = _penalised_rows(fp8=True)
    try:
        lm.use_fp8(True, wide=True)
        for b in rows:
            x, mask, ids = _prompt(model, "pen", b)
            want = lm.sample_generate(x, mask, MAX_NEW, 1, do_sample=False, repetition_penalty=PENALTY, eos_id=EOS,
                                      device_sampler=True).cpu().tolist()
            for j in (1, 4):
                drafts = lc.forced_drafts(want[0], 4, MAX_NEW, j, vocab)
                for graph in (False, True):
                    got, stats = _sampled_lookup(lm, x, mask, ids, 4, graph, drafts, repetition_penalty=PENALTY)
                    assert got == want, (b, j, graph, got, want)
    finally:
        lm.use_fp8(False)


# ------------------------------------------------------------------------------------------------ 9. model level
def test_model_option_reaches_the_device_loop(model, monkeypatch):
    """``EmuModel(device_sampler=True).generate_ids(do_sample=True, temperature=0.7, top_p=0.9, prompt_lookup_num_tokens=4)`` runs
    ``lookup_generate``'s sampled loop on one ``torch.rand`` table; with an id of the free run declared EOS the result is the free
    run cut behind it; with the flag off the call is refused as before."""
    m, _, _, z, l, vocab = model
    ids, mask = _t(z["pen_ids"])[:1], _t(z["pen_mask"])[:1]
    # min_len = 0: no id is suppressed in either run, so declaring another id EOS leaves every draw in front of it as it was
    kw = dict(max_new_tokens=MAX_NEW, min_len=0, prompt_lookup_num_tokens=4, **DEMO)
    with pytest.raises(ValueError, match="sampling"):
        m.generate_ids(ids, mask, None, **kw)
    monkeypatch.setattr(m, "device_sampler", True)
    table = torch.rand(MAX_NEW, generator=torch.Generator().manual_seed(8), dtype=torch.float32)
    real_rand, made = torch.rand, []

    def fixed(*shape, **k):
        if tuple(shape) == (MAX_NEW,) and k.get("dtype") == torch.float32:
            made.append(1)
            return table.to(k.get("device", "cpu"))
        return real_rand(*shape, **k)

    monkeypatch.setattr(torch, "rand", fixed)
    calls = []
    real = llama.LlamaEngine.lookup_generate
    monkeypatch.setattr(llama.LlamaEngine, "lookup_generate", lambda self, *a, **k: calls.append(k) or real(self, *a, **k))
    free = m.generate_ids(ids, mask, None, stop_on_eos=False, **kw).cpu()
    assert free.shape == (1, MAX_NEW) and len(calls) == 1 and len(made) == 1
    assert calls[0]["do_sample"] is True and calls[0]["temperature"] == 0.7 and calls[0]["top_p"] == 0.9 and calls[0]["num_tokens"] == 4
    assert "lookup_sample" in m.decoder.lm._loop_states
    x, pm, pids = _prompt(model, "pen", 0)
    direct = m.decoder.lm.lookup_generate(x, pm, pids, MAX_NEW, 4, min_len=0, stop_on_eos=False, uniforms=table, **DEMO).cpu()
    assert torch.equal(free, direct), "the model's call is the engine's with the table torch.rand handed out"
    g = free[0].tolist()
    at = next(i for i in range(1, MAX_NEW) if g[i] not in g[:i])                 # an id first drawn behind index 0
    got = m.generate_ids(ids, mask, None, eos_token_id=g[at], **kw).cpu()
    assert got.tolist() == [g[:at + 1]], (got.tolist(), g, at)
    raw = m.decoder.lm._loop_states["lookup_sample"][1]["out_ids"].cpu().tolist()
    assert raw[:at + 1] == g[:at + 1] and all(t == PAD for t in raw[at + 1:]), raw
