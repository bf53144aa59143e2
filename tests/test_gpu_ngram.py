"""GPU: the no-repeat n-gram ban on the device -- ``emu_sample_ngram_bf16``, ``emu_beam_step_ngram_bf16`` and
``emu_beam_sample_step_ngram_bf16`` against the specification (emu_amd/sampling.py with ``banned`` = ``banned_ngram_mask``) and the
torch pipeline of the host loop, and the device loops under ``device_ngram_ban`` against the host loops on the same engine."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from emu_amd import llama, sampling
from tests import beam_sampler_cases as bc
from tests import constrain_cases as cc
from tests import ngram_cases as nc
from tests import tiny
from tests.beam_step_common import BeamBuffers, assert_beam_state, logit_strides
from tests.test_gpu_beam_sampler import Step
from tests.test_gpu_sampler import DRAW_TOL

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
EOS, PAD = nc.EOS, nc.PAD
NEG_INF = -float("inf")
PAD_ID, NO_EOS = 1, -1                                 # of the bare kernel calls (tests/test_gpu_sampler.py's)
SAMPLE_SHAPES = [(97, 3), (1000, 2), (32274, 2), (40000, 1)]
NS = (1, 2, 3, 5)
SCALE = {97: 3.0, 1000: 4.0, 32274: 16.0, 40000: 16.0}        # tests/sampler_cases.py: the top-p threshold in the sparse upper tail
MARGIN = 1e-4                                          # ... and its screen: no fp32 summation order flips a top-p decision


# ------------------------------------------------------------------------------------------------ the sample kernel
def _params(o, do_sample, suppress=None, min_len=1 << 30):
    from emu_amd.llama import sample_params
    return sample_params(do_sample, o.get("temperature"), o.get("top_k"), o.get("top_p"), o.get("repetition_penalty", 1.0), suppress,
                         min_len, NO_EOS, PAD_ID, 1)


def _hist_dev(hist, rows):
    """int64 [rows, nh] -> the kernel's int32 [max(nh, 1), rows]."""
    h = torch.full((max(hist.shape[1], 1), rows), PAD, dtype=torch.int32, device="cuda")
    if hist.shape[1]:
        h[:hist.shape[1]] = hist.t().to(torch.int32).cuda()
    return h


def _run(x, hist, step, ngram, do_sample=False, o={}, uniforms=None, probs=False, suppress=None):
    """One launch: (ids, probabilities or None).  ``ngram`` None = the parent entry point.  ``probs``: rows V + 5 apart, the 5
    columns between the rows must stay as they were."""
    from emu_amd import ops
    R, V = x.shape
    step_dev = torch.tensor([step], dtype=torch.int32, device="cuda")
    if do_sample and uniforms is None:
        uniforms = torch.full((step + 1, R), 0.5, dtype=torch.float32, device="cuda")
    pr = torch.full((R, V + 5), -1.0, dtype=torch.float32, device="cuda") if probs else None
    out = ops.sample(x.cuda(), step_dev, _params(o, do_sample, suppress), hist=_hist_dev(hist, R), uniforms=uniforms,
                     probs_out=None if pr is None else pr[:, :V], ngram=ngram)
    torch.cuda.synchronize()
    if probs:
        assert bool((pr[:, V:] == -1.0).all())
    return out.cpu().long(), (pr[:, :V].cpu() if probs else None)


@pytest.mark.parametrize("V,rows", SAMPLE_SHAPES)
def test_sample_greedy_with_planted_repetitions(V, rows):
    """n in {1, 2, 3, 5} x step in {0, n - 1, n, 17} x the three planted targets (id 0, id V - 1, the first id of the last thread's
    chunk): the ids equal ``reference_greedy(banned=mask)`` exactly, plain and under a penalty with a suppressed id; on every planted
    row the unbanned arg-max IS the planted id and the kernel's id is another."""
    fired = 0
    for n in NS:
        for step in sorted({0, n - 1, n, 17}):
            for k in range(3):
                x, hist, targets, planted = nc.planted_case(V, rows, n, step, k)
                mask = sampling.banned_ngram_mask(hist, n, V)
                what = (n, step, k)
                got, _ = _run(x, hist, step, n)
                assert got.tolist() == sampling.reference_greedy(x, hist, banned=mask).tolist(), what
                free = sampling.reference_greedy(x).tolist()
                assert free == targets, what
                for r in range(rows):
                    assert bool(mask[r, targets[r]]) == planted[r] and (int(got[r]) != targets[r]) == planted[r], (what, r)
                fired += sum(planted)
                sup = int(got[0])                           # row 0's choice is suppressed on top: it has to move again
                got, _ = _run(x, hist, step, n, o=dict(repetition_penalty=1.3), suppress=sup)
                assert got.tolist() == sampling.reference_greedy(x, hist, 1.3, sup, banned=mask).tolist(), what
                assert int(got[0]) != sup, what
    assert fired >= 3 * rows * len(NS) * 2                  # at step n and at step 17 every row is planted


@functools.lru_cache(maxsize=None)
def _sampling_case(V, rows, n, step, name):
    """A planted case whose top-p decisions are at least ``MARGIN`` of mass from their bound (the first seed of 0, 1, ... to pass):
    (x, hist, mask, options of ``reference_probs``)."""
    opts = dict(nc.CHAT if name == "chat" else nc.PEN)
    for seed in range(64):
        x, hist, targets, planted = nc.planted_case(V, rows, n, step, 0, seed=seed)
        x = (x.float() * (SCALE[V] / 3.0)).to(BF16)
        mask = sampling.banned_ngram_mask(hist, n, V)
        o = dict(opts, history=hist, suppress_id=EOS, banned=mask)
        if float(sampling.top_p_threshold_group(x, **o)[1].min()) >= MARGIN:
            return x, hist, mask, o
    raise AssertionError("no seed passes the screen")


@pytest.mark.parametrize("V,rows", SAMPLE_SHAPES)
def test_sample_kept_set_probabilities_and_draw(V, rows):
    """Sampling at the chat options and under penalty + top-k + top-p, a suppressed id beside the ban: ``probs_out > 0`` is exactly
    the spec's kept set, no banned id is in it, the values agree with the fp64 form within the 1e-5 of tests/test_gpu_sampler.py; 64
    rows of one logit row under 64 uniforms (0 and 1 - 2^-24 among them) draw inside the fp64 interval, that file's rule and
    tolerance."""
    for n in NS:
        for step in (n, 17):
            for name in ("chat", "pen"):
                x, hist, mask, o = _sampling_case(V, rows, n, step, name)
                kw = dict(temperature=o.get("temperature"), top_k=o.get("top_k"), top_p=o.get("top_p"),
                          repetition_penalty=o.get("repetition_penalty", 1.0))
                tok, pr = _run(x, hist, step, n, True, kw, probs=True, suppress=EOS)
                q32, q64 = sampling.reference_probs(x, **o), sampling.reference_probs(x, dtype=torch.float64, **o)
                what = (n, step, name)
                assert bool(mask.any()) and torch.equal(pr > 0, q32 > 0) and not bool((pr > 0)[mask].any()), what
                err = float((pr.double() - q64).abs().max())
                print(f"V={V} {what}: kept {int((pr[0] > 0).sum())}, banned {int(mask[0].sum())}, max |q - spec| {err:.2e}")
                assert err <= 1e-5, (what, err)
                assert bool((q32.gather(1, tok[:, None]) > 0).all()), what
    x, hist, mask, o = _sampling_case(V, rows, 2, 17, "chat")
    R = 64
    u = torch.rand(R, generator=torch.Generator().manual_seed(V), dtype=torch.float32)
    u[0], u[1] = 0.0, 1 - 2.0 ** -24
    uni = torch.zeros(18, R)
    uni[17] = u
    tok, _ = _run(x[:1].expand(R, V).contiguous(), hist[:1].expand(R, -1), 17, 2, True, nc.CHAT, uniforms=uni.cuda(), suppress=EOS)
    q64 = sampling.reference_probs(x[:1], dtype=torch.float64, **dict(o, history=hist[:1], banned=mask[:1]))
    lo, hi = sampling.reference_intervals(q64)
    lo_t, hi_t, ud = lo[0, tok], hi[0, tok], u.double()
    assert bool((q64[0, tok] > 0).all()) and not bool(mask[0, tok].any())
    assert bool(((ud >= lo_t - DRAW_TOL) & (ud <= hi_t + DRAW_TOL)).all()), float(torch.maximum(lo_t - ud, ud - hi_t).max())
    assert int(tok[0]) == int((q64[0] > 0).nonzero()[0])    # u = 0: the lowest kept id


def test_sample_long_history_and_the_clamp():
    """step = 1500 at V = 97 (the position loop strides more than once; ids repeat everywhere) and step = 20 over a history buffer of
    8 rows (the kernel reads min(step, hist_rows) of them)."""
    V, rows, n = 97, 3, 2
    g = torch.Generator().manual_seed(5)
    hist = torch.randint(3, V, (rows, 1500), generator=g)
    x = (torch.randn(rows, V, generator=g) * 3.0).to(BF16)
    for r, f in enumerate(nc.planted_targets(V)):
        hist[r, 1200], hist[r, 1201] = hist[r, -1], f       # behind the first 1024 positions
        x[r, f] = x[r].float().max() + 1.0
    mask = sampling.banned_ngram_mask(hist, n, V)
    got, _ = _run(x, hist, 1500, n)
    assert got.tolist() == sampling.reference_greedy(x, hist, banned=mask).tolist()
    assert all(int(got[r]) != f and bool(mask[r, f]) for r, f in enumerate(nc.planted_targets(V)))
    assert sampling.reference_greedy(x).tolist() == nc.planted_targets(V)
    for k in range(3):
        x, hist, targets, planted = nc.planted_case(1000, 2, 2, 20, k, hist_rows=8)
        assert hist.shape == (2, 8) and all(planted)
        got, _ = _run(x, hist, 20, 2)                       # the buffer has 8 rows, the step index says 20
        assert got.tolist() == sampling.reference_greedy(x, hist, banned=sampling.banned_ngram_mask(hist, 2, 1000)).tolist()
        assert all(int(got[r]) != targets[r] for r in range(2))


@pytest.mark.parametrize("V", [97, 1000, 32274])
def test_sample_pad_in_the_banned_position_is_ignored(V):
    """Row 0's history repeats its last id followed by an id outside the vocabulary (PAD 32000; V + 3 where PAD is a real id): nothing
    is banned there and nothing is written outside the row (the columns between the rows of ``probs_out`` are checked by ``_run``);
    row 1's planted ban holds."""
    g = torch.Generator().manual_seed(V)
    x = (torch.randn(2, V, generator=g) * 3.0).to(BF16)
    outside = PAD if V <= PAD else V + 3
    hist = torch.tensor([[7, outside, 9, 10, 7], [7, 0, 9, 10, 7]])
    x[1, 0] = x[1].float().max() + 1.0
    mask = sampling.banned_ngram_mask(hist, 2, V)
    assert mask.nonzero().tolist() == [[1, 0]]
    got, _ = _run(x, hist, 5, 2)
    assert got.tolist() == sampling.reference_greedy(x, hist, banned=mask).tolist() and int(got[0]) == int(sampling.reference_greedy(x)[0])
    tok, pr = _run(x, hist, 5, 2, True, dict(top_k=50), probs=True)
    q64 = sampling.reference_probs(x, hist, top_k=50, dtype=torch.float64, banned=mask)
    assert torch.equal(pr > 0, q64 > 0) and float((pr.double() - q64).abs().max()) <= 1e-5 and float(pr[1, 0]) == 0.0


@pytest.mark.parametrize("V,rows", SAMPLE_SHAPES)
def test_sample_without_a_ban_equals_the_parent_bit_for_bit(V, rows):
    """``ngram = 0``, and n = 3 over a history of distinct ids: ``out`` and ``probs_out`` are ``emu_sample_bf16``'s bits, greedy and
    sampling; two identical calls give identical bits; ``ngram = -1`` is refused with nothing written."""
    from emu_amd import ops
    from emu_amd._lib import lib
    x, hist, _, _ = nc.planted_case(V, rows, 3, 2, 0)       # step 2 < n: two distinct ids per row, no ban possible
    g = torch.Generator().manual_seed(V)
    distinct = torch.stack([torch.randperm(V - 3, generator=g)[:17] + 3 for _ in range(rows)])
    assert not bool(sampling.banned_ngram_mask(distinct, 3, V).any())
    for o, do_sample in ((dict(repetition_penalty=1.3), False), (dict(nc.PEN), True), (dict(nc.CHAT), True)):
        a, pa = _run(x, distinct, 17, None, do_sample, o, probs=do_sample, suppress=EOS)
        for ngram in (0, 3):
            b, pb = _run(x, distinct, 17, ngram, do_sample, o, probs=do_sample, suppress=EOS)
            assert torch.equal(a, b) and (pa is None or torch.equal(pa.view(torch.int32), pb.view(torch.int32))), (o, ngram)
    x, hist, _, _ = nc.planted_case(V, rows, 2, 17, 1)
    runs = [_run(x, hist, 17, 2, True, dict(nc.PEN), probs=True, suppress=EOS) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    lg, out = x.cuda(), torch.full((rows,), -7, dtype=torch.int32, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    p = _params({}, False)
    assert lib().emu_sample_ngram_bf16(lg.data_ptr(), V, rows, V, None, 0, 0, step.data_ptr(), None, 0, 0, C.byref(p), None, out.data_ptr(),
                                       None, 0, -1, ops.stream(lg.device)) == -22
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [-7] * rows


# ------------------------------------------------------------------------------------------------ the beam kernels, step by step
class _DetState(BeamBuffers):
    """Device state of ``emu_beam_step_bf16`` at the start of a search, and one call of it (``ngram`` None = the parent)."""

    def __init__(self, B, nb, V, L):
        from emu_amd._lib import lib
        super().__init__(sampling.beam_start_state(B, nb, L, PAD))
        self.V = V
        self.ws = torch.empty(lib().emu_beam_step_workspace_bytes(B, nb, V), dtype=torch.uint8, device="cuda")

    def call(self, lg, cur, v431, ngram, counter):
        from emu_amd import ops
        from emu_amd._lib import lib
        args = self.step_args(lg.data_ptr(), *logit_strides(lg, self.B, self.nb), self.V, cur, nc.BEAM_MIN_LEN, EOS, nc.BEAM_LP, v431,
                              self.ws, counter)
        rc = lib().emu_beam_step_bf16(*args, ops.stream(lg.device)) if ngram is None else \
            lib().emu_beam_step_ngram_bf16(*args, ngram, ops.stream(lg.device))
        torch.cuda.synchronize()
        return rc


@pytest.mark.parametrize("v431", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("B,nb,V,L", nc.BEAM_SHAPES)
def test_beam_step_ngram_equals_the_torch_pipeline(B, nb, V, L, n, v431):
    """tests/test_gpu_beam.py::test_beam_step_kernel_equals_the_torch_pipeline with the ban: after every step the state and the outputs
    of ``emu_beam_step_ngram_bf16`` equal the torch pipeline's (``process_logits(..., no_repeat_ngram_size=n)`` on the log-probabilities,
    tests/ngram_cases.py), ids exactly, scores to that test's 1e-4.  Under v431 the step index comes from the device counter.  From
    step n on some beam row has a non-empty banned set, and the kept sequences differ from the same logits' search with
    ``ngram = 0`` -- which in turn is ``emu_beam_step_bf16``'s bit for bit.  A call with ``cur >= L`` changes nothing."""
    steps = nc.beam_scenario(B, nb, V, L, n, v431)
    assert all(s["banned_rows"] > 0 for s in steps[n:]), [s["banned_rows"] for s in steps]
    st, zero, parent = _DetState(B, nb, V, L), _DetState(B, nb, V, L), _DetState(B, nb, V, L)
    for cur, s in enumerate(steps):
        lg = s["lg"].cuda()
        assert st.call(lg, cur, v431, n, counter=v431) == 0 and zero.call(lg, cur, v431, 0, counter=v431) == 0
        assert parent.call(lg, cur, v431, None, counter=v431) == 0
        what = f"step {cur}"
        assert_beam_state(st, s["state"], s["toks"], s["flat"], what)
        for a_, b_ in zip(zero.state(), parent.state()):
            assert torch.equal(a_.view(torch.uint8), b_.view(torch.uint8)), what
    assert st.seq.cpu().tolist() != zero.seq.cpu().tolist()
    assert not any(nc.has_repeated_ngram(r, n) for r in st.seq.cpu().view(-1, L).tolist())
    assert any(nc.has_repeated_ngram(r, n) for r in zero.seq.cpu().view(-1, L).tolist())
    snap = [t.clone() for t in st.state()]
    assert st.call(lg, L, v431, n, counter=True) == 0
    assert all(torch.equal(a_, b_) for a_, b_ in zip(snap, st.state()))
    assert st.call(lg, 0, v431, -1, counter=False) == -22
    assert all(torch.equal(a_, b_) for a_, b_ in zip(snap, st.state()))


class _NgramStep(Step):
    """tests/test_gpu_beam_sampler.py's Step calling ``emu_beam_sample_step_ngram_bf16`` (``ngram`` None: the parent)."""

    def call(self, o, cur, want=0, ngram=None, **kw):
        from emu_amd import ops
        from emu_amd._lib import lib
        args = self.args(o, cur, **kw)
        rc = lib().emu_beam_sample_step_bf16(*args, ops.stream(self.lg.device)) if ngram is None else \
            lib().emu_beam_sample_step_ngram_bf16(*args, ngram, ops.stream(self.lg.device))
        assert rc == want, rc
        torch.cuda.synchronize()


@pytest.mark.parametrize("sample", [True, False])
@pytest.mark.parametrize("v431", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("B,nb,V,L", nc.BEAM_SHAPES)
def test_beam_sample_step_ngram_equals_the_specification(B, nb, V, L, n, v431, sample):
    """tests/test_gpu_beam_sampler.py::test_bookkeeping_equals_the_torch_pipeline with the ban: after every step the kernel's state
    and outputs equal a torch step whose scores are the spec's (``beam_reference_rows(banned=mask)`` from the torch state's own
    histories and running scores) and whose candidates are the kernel's own ``draws_out`` (sorted by the spec's scores under "4.31");
    scores to that file's 1e-4.  No banned id keeps a score in ``acc_out`` or is drawn.  Without sampling (penalised beam search)
    ``acc_out`` is finite exactly where the spec is and the candidates must BE the stable top-2N of the spec's scores.  Bans fire (the counts are asserted), the kept sequences differ from the ``ngram = 0`` run of the same
    logits and uniforms, which is the parent's bit for bit, and a call at ``cur = L`` changes nothing."""
    from tests.test_beam_sampling_host import spec_acc
    order = "4.31" if v431 else "5.x"
    # (under "4.31" the running score IS the warped row: a temperature of 0.7 would divide it, and every rounding in it, by 0.7 once per
    # step -- 5000-fold over 24 steps, beyond any absolute bound on the scores; that order is run at temperature 1)
    o = dict(temperature=1.0 if v431 else 0.7, top_k=3, top_p=0.9, repetition_penalty=1.2) if sample else dict(repetition_penalty=1.3)
    s, zero, parent = (_NgramStep(B, nb, V, L, order, sample) for _ in range(3))
    ref = sampling.beam_start_state(B, nb, L, 32000, equal_start=sample and v431)
    g = torch.Generator().manual_seed(B * 1000 + nb * 10 + L + n)
    fired = 0
    for cur, x in enumerate(nc.beam_logits(B, nb, V, L)):
        for t in (s, zero, parent):
            t.set_logits(x, shared=cur == 0)
        rows = x.repeat_interleave(nb, 0) if cur == 0 else x
        u = torch.rand(1, B, 2 * nb, generator=g).cuda()
        hist = ref["running_seq"][:, :, :cur].reshape(B * nb, cur)
        mask = sampling.banned_ngram_mask(hist, n, V)
        fired += int(mask.any(dim=1).sum())
        accr = sampling.beam_reference_rows(rows, ref["running_scores"], hist if cur else None, o["repetition_penalty"], bc.EOS,
                                            cur < nc.BEAM_MIN_LEN, do_sample=sample, temperature=o.get("temperature"),
                                            top_k=o.get("top_k"), top_p=o.get("top_p"), order=order, banned=mask)
        kw = dict(min_len=nc.BEAM_MIN_LEN, lp=1.0, hf431=int(v431), u=u, device_counter=v431)
        s.call(o, cur, ngram=n, **kw); zero.call(o, cur, ngram=0, **kw); parent.call(o, cur, ngram=None, **kw)
        what = f"step {cur}"
        got = s.acc[:, :V].cpu()
        assert not bool((got > NEG_INF)[mask].any()), what                       # no banned id keeps a score
        top_idx = s.draws.long().cpu()
        acc = accr.view(B, nb * V)
        if not sample:
            assert torch.equal(got > NEG_INF, accr > NEG_INF), what
            assert float((got[accr > NEG_INF] - accr[accr > NEG_INF]).abs().max()) <= 1e-4, what
            assert top_idx.tolist() == sampling.beam_reference_select(accr.view(B, nb, V), nb, None, False)[1].tolist(), what
        top_lp = acc.gather(1, top_idx)
        assert bool((top_lp > NEG_INF).all()) and all(len(set(r)) == 2 * nb for r in top_idx.tolist()), what
        assert not bool(mask.view(B, nb * V).gather(1, top_idx).any()), what
        if sample and v431:
            top_lp, srt = torch.sort(top_lp, descending=True, dim=1, stable=True)
            top_idx = top_idx.gather(1, srt)
        toks, flat = sampling.beam_scorer_step(ref, top_lp, top_idx, V, cur, L, 1.0, bc.EOS, v431)[:2]
        assert_beam_state(s, ref, toks, flat, what)
        for a_, b_ in zip(zero.outputs(), parent.outputs()):
            assert torch.equal(a_.view(torch.uint8), b_.view(torch.uint8)), what
    print(f"{(B, nb, V, L)} n={n} {order} sample={sample}: banned rows over the search {fired}")
    assert fired >= L - n
    assert s.seq.cpu().tolist() != zero.seq.cpu().tolist()
    assert not any(nc.has_repeated_ngram(r, n) for r in s.run.cpu().view(-1, L).tolist())
    snap = [t_.clone() for t_ in s.outputs()]
    s.call(o, L, ngram=n, **dict(kw, device_counter=True))
    assert all(torch.equal(a_, b_) for a_, b_ in zip(snap, s.outputs()))
    s.call(o, 0, ngram=-1, want=-22, **dict(kw, device_counter=False))
    assert all(torch.equal(a_, b_) for a_, b_ in zip(snap, s.outputs()))


# ------------------------------------------------------------------------------------------------ the loops on the tiny LLaMA
N_NEW = 40
LOOP_SEED = 2                                          # picked on the GPU among 1..12: see the fixture (host margins 0.005 / 0.008 nat)
LOOP_MARGIN = 10 * bc.MARGIN


@pytest.fixture(scope="module")
def tiny_engine():
    """tests/constrain_cases.py::tiny_llama at the engine's smallest shape (vocabulary 64, two layers, two heads of 128) on the
    device, and two left-padded prompts.  40 new tokens with min_len = 40: no row finishes early.  ``LOOP_SEED`` is one at which the
    unbanned outputs do repeat n-grams and the host beam loop's margin is above ``LOOP_MARGIN``; the tests assert both."""
    from emu_amd.llama import EmuHipContext, LlamaEngine
    hf, W, l, r = cc.tiny_llama(LOOP_SEED, vocab=64, hidden=256, heads=2, layers=2, ffn=512)
    eng = LlamaEngine(l, 64, EmuHipContext(torch.device("cuda", 0)))
    eng.load_weights(W.items())
    ids = torch.randint(3, 64, (2, 6), generator=torch.Generator().manual_seed(LOOP_SEED))
    mask = torch.ones(2, 6, dtype=torch.long)
    mask[1, :2] = 0
    return eng, eng.embed_tokens(ids).contiguous(), mask


def _one(eng, x, mask, **kw):
    return eng.sample_generate(x, mask, N_NEW, min_len=N_NEW, pad_id=PAD, **kw).cpu()


@pytest.mark.parametrize("n", [1, 2, 3])
def test_one_beam_loop_equals_the_host_loop(tiny_engine, n):
    """Greedy with the ban on the device, eager and replayed, returns the host loop's ids; sampling under one table of uniforms draws
    every id inside the fp64 interval of the spec with ``banned`` on that step's logits (the extent to which
    tests/test_gpu_device_sampler.py compares the loops), the same eager and replayed.  No output row repeats an n-gram; the
    unbanned output of the same prompts does."""
    from tests.test_gpu_device_sampler import _step_logits
    eng, x, mask = tiny_engine
    host = _one(eng, x, mask, do_sample=False, no_repeat_ngram_size=n)
    assert host.shape == (2, N_NEW) and not any(nc.has_repeated_ngram(r, n) for r in host.tolist())
    for graph in (False, True):
        got = _one(eng, x, mask, do_sample=False, no_repeat_ngram_size=n, device_sampler=True, device_ngram_ban=True, use_graph=graph)
        assert got.tolist() == host.tolist(), graph
    free = _one(eng, x, mask, do_sample=False, device_sampler=True, use_graph=True)
    assert any(nc.has_repeated_ngram(r, n) for r in free.tolist())
    uni = torch.rand(N_NEW, 2, generator=torch.Generator().manual_seed(7), dtype=torch.float32).cuda()
    o = dict(temperature=0.9, top_k=50)
    ids = _one(eng, x, mask, do_sample=True, no_repeat_ngram_size=n, device_sampler=True, device_ngram_ban=True, uniforms=uni, **o)
    assert ids.shape == (2, N_NEW) and not any(nc.has_repeated_ngram(r, n) for r in ids.tolist())
    u = uni.cpu().double()
    for step, lg in enumerate(_step_logits(eng, x, mask, ids)):
        q = sampling.reference_probs(lg, suppress_id=EOS, dtype=torch.float64, banned=sampling.banned_ngram_mask(ids[:, :step], n, 64), **o)
        lo, hi = sampling.reference_intervals(q)
        t = ids[:, step, None]
        lo_t, hi_t = lo.gather(1, t)[:, 0], hi.gather(1, t)[:, 0]
        assert bool((q.gather(1, t) > 0).all()), step
        assert bool(((u[step] >= lo_t - DRAW_TOL) & (u[step] <= hi_t + DRAW_TOL)).all()), step
    again = _one(eng, x, mask, do_sample=True, no_repeat_ngram_size=n, device_sampler=True, device_ngram_ban=True, uniforms=uni,
                 use_graph=True, **o)
    assert again.tolist() == ids.tolist()
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):             # without the flag: the refusal of before
        _one(eng, x, mask, do_sample=False, no_repeat_ngram_size=n, device_sampler=True)


def test_beam_loops_equal_the_host_loop(tiny_engine, monkeypatch):
    """3 beams, bigram ban: the deterministic device loop (``emu_beam_step_ngram_bf16``), eager and replayed, returns the host
    loop's ids, as tests/test_gpu_constrain.py compares them (the host's margin is the precondition); so does penalised beam search
    through ``emu_beam_sample_step_ngram_bf16``.  No row repeats a bigram; the unbanned search does."""
    eng, x, mask = tiny_engine
    every = list(range(64))
    # the host loop with the kernels' tie rule (ties to the lower index; its margins leave exact ties out): what a constraint makes
    # of it -- here one that allows every id.  bf16 logits tie exactly all the time, and torch.topk leaves such ties open
    stable = dict(constraint=lambda batch_id, ids: every)
    beam = lambda **k: eng.beam_search_generate(x, mask, 3, N_NEW, min_len=N_NEW, length_penalty=0.0, pad_id=PAD, hf_semantics="5.x",
                                                **k).cpu()
    calls = _count_calls(monkeypatch)
    for extra, entry in ((dict(), "emu_beam_step_ngram_bf16"),
                         (dict(repetition_penalty=1.2, device_beam_sampler=True), "emu_beam_sample_step_ngram_bf16")):
        tr = {}
        host = beam(no_repeat_ngram_size=2, trace=tr, **stable, **{k: v for k, v in extra.items() if k != "device_beam_sampler"})
        print(f"{entry}: host margin {tr['margin']:.4f}")
        assert tr["margin"] > LOOP_MARGIN, tr
        assert not calls and not any(nc.has_repeated_ngram(r, 2) for r in host.tolist())
        for graph in (False, True):
            monkeypatch.setattr(eng, "beam_graph", graph, raising=False)
            calls.clear()
            got = beam(no_repeat_ngram_size=2, device_ngram_ban=True, **extra)
            assert got.tolist() == host.tolist(), (entry, graph)
            assert set(calls) == {entry}, calls
        calls.clear()
    free = beam()
    assert any(nc.has_repeated_ngram(r, 2) for r in free.tolist()) and set(calls) == {"emu_beam_step_bf16"}
    calls.clear()
    assert beam(no_repeat_ngram_size=2).shape == (2, N_NEW) and not calls       # without the flag: the host loop, as before
    uni = torch.rand(N_NEW, 2, 6, generator=torch.Generator().manual_seed(3), dtype=torch.float32)
    runs = []
    for graph in (False, True):
        monkeypatch.setattr(eng, "beam_graph", graph, raising=False)
        runs.append(beam(no_repeat_ngram_size=2, device_ngram_ban=True, device_beam_sampler=True, do_sample=True, temperature=0.7, top_k=3,
                         top_p=0.9, uniforms=uni))
        assert not any(nc.has_repeated_ngram(r, 2) for r in runs[-1].tolist())
    assert runs[0].tolist() == runs[1].tolist()


def _count_calls(monkeypatch):
    """Spy on the C entry points ``emu_amd.llama`` calls: the names of the selection steps, in order."""
    from emu_amd import _lib
    real, calls = _lib.lib(), []
    watched = ("emu_beam_step_ngram_bf16", "emu_beam_sample_step_ngram_bf16", "emu_llama_sample_step_ngram", "emu_beam_step_bf16",
               "emu_beam_sample_step_bf16", "emu_llama_sample_step")

    class Counting:
        def __getattr__(self, name):
            f = getattr(real, name)
            if name in watched:
                return lambda *a: (calls.append(name), f(*a))[1]
            return f
    monkeypatch.setattr(llama, "lib", lambda: Counting())
    return calls


def test_emu_model_reaches_the_device_loops(golden_dir, monkeypatch):
    from emu_amd import EmuModel, TextDecoderCfg
    z = tiny.load(golden_dir, "generate_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    m = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda", device_sampler=True, device_beam_sampler=True,
                 device_ngram_ban=False)
    m.load_state_dict(W, strict=True)
    ids2, mask = torch.from_numpy(np.asarray(z["ids2"])), torch.from_numpy(np.asarray(z["mask2"]))
    calls = _count_calls(monkeypatch)
    one = lambda: m.generate_ids(ids2, mask, max_new_tokens=8, min_len=8, num_beams=1, no_repeat_ngram_size=1, hf_semantics="4.31").cpu()
    beams = lambda: m.generate_ids(ids2, mask, max_new_tokens=8, min_len=8, num_beams=3, no_repeat_ngram_size=1, hf_semantics="4.31").cpu()
    host1, hostb = one(), beams()
    assert not calls                                                             # the option off: the host loops
    monkeypatch.setattr(m, "device_ngram_ban", True)
    got1 = one()
    assert set(calls) == {"emu_llama_sample_step_ngram"} and got1.tolist() == host1.tolist()
    calls.clear()
    gotb = beams()
    assert set(calls) == {"emu_beam_step_ngram_bf16"} and gotb.tolist() == hostb.tolist()
    for row in got1.tolist() + gotb.tolist():
        assert not nc.has_repeated_ngram(row, 1), row


def test_emu1_reaches_the_device_loop(golden_dir, monkeypatch):
    """Emu1's caption call with its own options (5 beams, bigram ban, length_penalty 0; tests/golden/emu1_generate_tiny.npz)."""
    from emu_amd.emu1 import Emu
    z = tiny.load(golden_dir, "emu1_generate_tiny.npz")
    v, t5, l, vocab, W, ocfg = tiny.emu1_generate_from(z)
    m = Emu(v, l, t5, vocab=vocab, device="cuda")
    m.load_state_dict(W, strict=True)
    ids, mask, img = torch.from_numpy(z["ids"]), torch.from_numpy(z["mask"]), torch.from_numpy(z["image"])
    calls = _count_calls(monkeypatch)
    run = lambda: m.generate_ids(ids, mask, img.cuda(), num_beams=5, max_new_tokens=8, length_penalty=0.0, no_repeat_ngram_size=2).cpu()
    host = run()
    assert not calls and not any(nc.has_repeated_ngram(r, 2) for r in host.tolist())
    monkeypatch.setattr(m, "device_ngram_ban", True, raising=False)
    got = run()
    assert set(calls) == {"emu_beam_step_ngram_bf16"} and got.tolist() == host.tolist()
