"""GPU tests of beam-search sampling and penalised beam search on the device (csrc/beam_sample.hip, emu_beam_sample_step_bf16, and
the loop of LlamaEngine.beam_search_generate(device_beam_sampler=True)) against the specification in emu_amd/sampling.py and against
the host loop drawing from the same table of uniforms.  Run on an MI355X with `-m gpu`."""
import os

import numpy as np
import pytest
import torch

from emu_amd import sampling
from tests import beam_sampler_cases as bc
from tests import tiny
from tests.beam_step_common import BeamBuffers, assert_beam_state
from tests.test_beam_sampling_host import spec_acc

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
NEG_INF = -float("inf")
DEV = torch.device("cuda", 0)
_t = lambda a: torch.from_numpy(np.asarray(a))

# the draws' tolerance: derived in test_every_draw_lies_in_its_reference_interval's docstring
BEAM_DRAW_TOL = (58 + 59 + 1) * 2.0 ** -24 + 2 * (2 * 2.0 ** -22 + 2.0 ** -24 * 12.7)


class Step(BeamBuffers):
    """State and buffers of emu_beam_sample_step_bf16 for B prompts x nb beams, and one call of it."""

    def __init__(self, B, nb, V, L, order="5.x", sample=True, ld=None, ld_acc=None):
        from emu_amd._lib import lib
        super().__init__(sampling.beam_start_state(B, nb, L, 32000, equal_start=sample and order == "4.31"), DEV, fill=-1)
        self.V, self.order, self.sample = V, order, sample
        self.ws = torch.empty(lib().emu_beam_sample_workspace_bytes(B, nb, V), dtype=torch.uint8, device=DEV)
        self.draws = torch.full((B, 2 * nb), -1, dtype=torch.int32, device=DEV)
        self.ld = ld or V
        self.ld_acc = ld_acc or V
        self.lg = torch.zeros(B * nb * self.ld + 1, dtype=BF16, device=DEV)          # rows start at element 1: an odd base offset
        self.acc = torch.full((B * nb, self.ld_acc), 7.0, device=DEV)

    def outputs(self):
        return self.state() + (self.draws, self.acc)

    def set_logits(self, x, shared=False):
        """x [B * nb, V] (or [B, V] with ``shared``: step 0, every beam continues the prompt)."""
        rows = x.shape[0]
        view = self.lg[1:1 + rows * self.ld].view(rows, self.ld)
        view[:, :self.V] = x.to(DEV)
        self.ldp, self.ldb = (self.ld, 0) if shared else (self.nb * self.ld, self.ld)

    def args(self, o, cur, min_len=0, lp=1.0, hf431=0, u=None, eos=bc.EOS, device_counter=False, **override):
        """The arguments of emu_beam_sample_step_bf16 ahead of the stream: the beam step's common list, then the sampler's."""
        from emu_amd.llama import sample_params
        params = sample_params(self.sample, o.get("temperature"), o.get("top_k"), o.get("top_p"), o.get("repetition_penalty", 1.0),
                               eos, min_len, eos, 32000, min_keep=1)                    # (the call forces min_keep to 2)
        uni = override.pop("uni") if "uni" in override else (None if u is None else u.data_ptr())
        return (*self.step_args(self.lg.data_ptr() + 2, self.ldp, self.ldb, override.pop("V", self.V), cur, min_len, eos, lp, hf431,
                                self.ws, device_counter, override),
                params, int(self.sample and self.order == "4.31"), uni, 1, self.draws.data_ptr(), self.acc.data_ptr(), self.ld_acc)

    def call(self, o, cur, want=0, **kw):
        from emu_amd import ops
        from emu_amd._lib import lib
        rc = lib().emu_beam_sample_step_bf16(*self.args(o, cur, **kw), ops.stream(DEV))
        assert rc == want, rc
        torch.cuda.synchronize()


def _loaded(B, nb, V, name, order, sample=True, pad=0):
    """A Step at cur = 6 holding a screened case: its logits, histories (as the beams' running sequences) and running scores."""
    x, rs, o = bc.case(B, nb, V, name, order)
    s = Step(B, nb, V, 8, order, sample, ld=V + pad, ld_acc=V + pad)
    s.set_logits(x)
    s.rs.copy_(rs)
    s.run[:, :, :6] = bc.history(B * nb, V).view(B, nb, 6).to(torch.int32)
    if "history" not in o:
        o["history"] = None
    return s, x, rs, o


# ------------------------------------------------------------------------------------------------ 5. rows
@pytest.mark.parametrize("order", bc.ORDERS)
@pytest.mark.parametrize("B,nb,V", bc.GPU_SHAPES)
def test_rows_equal_the_spec(B, nb, V, order):
    """acc_out > -inf is exactly the spec's kept set; finite values agree with the fp32 spec to 1e-4 (tests/test_gpu_beam.py's bound
    for the re-ordered log-sum-exp).  Row strides V and V + 3 behind an odd base offset, do_sample on and off, every option set."""
    for name in bc.CASES:
        for sample in (True, False):
            for pad in (0, 3):
                s, x, rs, o = _loaded(B, nb, V, name, order, sample, pad)
                u = torch.full((1, B, 2 * nb), 0.5, device=DEV)
                s.call(o, 6, min_len=7 if o["suppress_eos"] else 0, u=u)
                got = s.acc[:, :V].cpu()
                want = spec_acc(x, rs, o, order, do_sample=sample)
                what = (name, sample, pad)
                assert torch.equal(got > NEG_INF, want > NEG_INF), what
                live = want > NEG_INF
                err = float((got[live] - want[live]).abs().max())
                print(f"{(B, nb, V)} {order} {what}: kept {int(live.sum())}, max |acc - spec| {err:.2e}")
                assert err <= 1e-4, (what, err)
                assert bool((s.acc[:, V:] == 7.0).all())                 # nothing written between the rows
                d = s.draws.long().cpu()
                assert bool((want.view(B, -1).gather(1, d) > NEG_INF).all()), what      # every draw is a kept entry


# ------------------------------------------------------------------------------------------------ 6. draws
def _judge(acc, nb, draws, u):
    """Every draw of ``draws`` [T, 2 nb] (T tables ``u`` [T, 2 nb], one prompt with kernel scores ``acc`` [nb, V]) against the fp64
    intervals with the kernel's own earlier draws removed.  Returns the worst distance outside an interval."""
    p = sampling.beam_reference_probs(acc, nb, torch.float64)[0]
    T, n2 = draws.shape
    rem = p.repeat(T, 1)
    free = (acc.reshape(-1) > NEG_INF).repeat(T, 1)
    worst = 0.0
    for k in range(n2):
        d = draws[:, k:k + 1]
        assert bool(free.gather(1, d).all()), f"draw {k}: a removed entry, or one drawn before"
        R = rem.sum(dim=1, keepdim=True)
        hi = rem.cumsum(dim=1).gather(1, d)
        mass = rem.gather(1, d)
        t = u[:, k:k + 1].double() * R
        out = torch.maximum((hi - mass) - t, t - hi)
        ok = (out <= BEAM_DRAW_TOL) & ((mass > 0) | (R <= BEAM_DRAW_TOL))
        lowest_free = free.int().argmax(dim=1, keepdim=True)
        ok = torch.where(R == 0, d == lowest_free, ok)                   # no mass left: the lowest not-yet-drawn finite entry
        assert bool(ok.all()), (k, float(out.max()))
        worst = max(worst, float(out[R > 0].max()) if bool((R > 0).any()) else 0.0)
        rem.scatter_(1, d, 0.0)
        free.scatter_(1, d, False)
    return worst


@pytest.mark.parametrize("order", bc.ORDERS)
@pytest.mark.parametrize("B,nb,V", bc.GPU_SHAPES)
def test_every_draw_lies_in_its_reference_interval(B, nb, V, order):
    """64 tables per shape and option set, u = 0 and u = 1 - 2^-24 among them.  Draw k passes iff u_k * R_k lies within
    [lo - tol, hi + tol] of the fp64 interval of the drawn entry, computed from the scores the kernel itself reports (acc_out, judged
    by test_rows_equal_the_spec) with the kernel's own draws 0..k-1 removed; in units of the initial total mass.  Every draw is
    judged; no index repeats, no removed index appears; where no mass is left the draw must be the lowest finite entry.

    tol = BEAM_DRAW_TOL, from the kernels' summation shape (beam_sample.hip).  A term of a cumulative value passes at most 40
    sequential adds inside its thread's chunk, 6 + 4 levels of the block scan, the add of the wave and lane prefixes, the add of the
    chunk's own prefix, the multiplication by the row's scale, and the add of the masses of up to 7 earlier rows one by one: at
    most 40 + 10 + 2 + 1 + 1 = 54 roundings for the drawn row and 40 + 10 + 1 + 7 = 58 for an earlier one, each at most 2^-24
    relative; a term of the remaining mass R at most 40 + 10 + 1 + 8 = 59; u * R rounds once more.  The terms themselves are
    exp(acc - row max) * exp(row max - common max) in fp32: the two subtractions are off by at most 2^-24 (|d1| + |d2|) =
    2^-24 |acc - common max| absolutely, which is that much relatively in the product, and each expf by at most 2 ulp = 2^-22;
    summed with the weights q_i that is at most 2 * 2^-22 + 2^-24 sum q_i |d_i| <= 2 * 2^-22 + 2^-24 ln(nb V) (the entropy bound),
    in the cumulative value and again in R.  With nb V <= 8 * 40 000: (58 + 59 + 1) * 2^-24 + 2 * (2 * 2^-22 + 2^-24 * 12.7) =
    7.03e-6 + 2.47e-6 = 9.5e-6 < 1e-5.  A drawn entry's mass is set to zero and its chunk sum rebuilt, so nothing drifts from draw to
    draw."""
    assert BEAM_DRAW_TOL < 1e-5
    T = 64
    for name in ("demo", "p09", "plain"):
        s, x, rs, o = _loaded(B, nb, V, name, order)
        U = torch.rand(T, B, 2 * nb, generator=torch.Generator().manual_seed(V + nb), dtype=torch.float32)
        U[0], U[1] = 0.0, 1 - 2.0 ** -24
        U = U.to(DEV)
        snap = [t_.clone() for t_ in s.state()]
        draws = torch.empty(T, B, 2 * nb, dtype=torch.int64, device=DEV)
        for i in range(T):
            for t_, c in zip(s.state(), snap):
                t_.copy_(c)
            s.call(o, 6, u=U[i:i + 1])
            draws[i] = s.draws.long()
        acc = s.acc[:, :V].view(B, nb, V)
        worst = max(_judge(acc[b], nb, draws[:, b], U[:, b]) for b in range(B))
        print(f"{(B, nb, V)} {order} {name}: worst distance outside an interval {worst:.2e} (tol {BEAM_DRAW_TOL:.2e})")
        p0 = sampling.beam_reference_probs(acc[0], nb, torch.float64)[0]
        assert int(draws[0, 0, 0]) == int((p0 > 0).nonzero()[0])         # u = 0: the lowest entry of positive mass


def test_zero_mass_fallback_on_the_device():
    """nb = 5, top_k = 3, the "5.x" start (step 0: every beam continues the prompt, beams 1..4 carry -1e9): the first draws are beam
    0's kept ids, the rest follow ascending flat index among the finite entries."""
    B, nb, V = 2, 5, 32274
    x = bc.rows(B, 1, V, 4)
    s = Step(B, nb, V, 8)
    s.set_logits(x, shared=True)
    o = dict(temperature=0.7, top_k=3, top_p=0.9)
    u = torch.rand(1, B, 2 * nb, generator=torch.Generator().manual_seed(1)).to(DEV)
    s.call(o, 0, u=u)
    acc = s.acc.view(B, nb * V).cpu()
    want = spec_acc(x.repeat_interleave(nb, 0), s_rs0(B, nb), dict(o, eos_id=bc.EOS, suppress_eos=False), "5.x").view(B, nb * V)
    assert torch.equal(acc > NEG_INF, want > NEG_INF)
    for b in range(B):
        finite = (acc[b] > NEG_INF).nonzero().flatten().tolist()
        n0 = sum(i < V for i in finite)
        d = s.draws[b].tolist()
        assert 2 <= n0 <= 3 and sorted(d[:n0]) == finite[:n0] and d[n0:] == finite[n0:2 * nb], (b, d, finite[:12])


def s_rs0(B, nb):
    return sampling.beam_start_state(B, nb, 1, 32000)["running_scores"]


# ------------------------------------------------------------------------------------------------ 7. bookkeeping
@pytest.mark.parametrize("sample", [True, False])
@pytest.mark.parametrize("v431", [False, True])
@pytest.mark.parametrize("B,nb,V,max_len,min_len,lp,eos_boost", [
    (2, 5, 32274, 8, 1, 1.0, 7.0),             # the demo's call: five beams, length_penalty 1, EOS often drawn
    (3, 3, 1000, 6, 3, -1.0, 8.0),             # min_length masks EOS for three steps
    (1, 2, 64, 5, 1, 0.0, 3.0),                # tiny vocabulary
])
def test_bookkeeping_equals_the_torch_pipeline(B, nb, V, max_len, min_len, lp, eos_boost, v431, sample):
    """Multi-step scenarios in the manner of test_beam_step_kernel_equals_the_torch_pipeline: random bf16 logits with the EOS logit
    raised, so that hypotheses finish and the heuristic closes.  After every step the kernel's state and outputs equal a step of the
    host loop's own bookkeeping (``sampling.beam_scorer_step``) whose scores are the spec's (from the torch state's own histories and
    running scores) and whose candidates are the kernel's own draws_out (sorted by the spec's scores under "4.31"); scores to 1e-4.  Without sampling (penalised beam search) the kernel's
    candidates must BE the stable top-2N of the spec's scores.  Under v431 the step index comes from a device counter, and a call
    at cur = L leaves everything untouched."""
    order = "4.31" if v431 else "5.x"
    o = dict(temperature=0.7, top_k=3, top_p=0.9, repetition_penalty=1.2) if sample else dict(repetition_penalty=1.3)
    s = Step(B, nb, V, max_len, order, sample)
    ref = sampling.beam_start_state(B, nb, max_len, 32000, equal_start=sample and v431)
    g = torch.Generator().manual_seed(B * 1000 + nb * 10 + max_len)
    for cur in range(max_len):
        x = (torch.randn(B if cur == 0 else B * nb, V, generator=g) * 3.0).to(BF16)
        x[:, bc.EOS] += eos_boost
        s.set_logits(x, shared=cur == 0)
        rows = x.repeat_interleave(nb, 0) if cur == 0 else x
        u = torch.rand(1, B, 2 * nb, generator=g).to(DEV)
        acc = spec_acc(rows, ref["running_scores"], dict(o, eos_id=bc.EOS, suppress_eos=cur < min_len,
                                                         history=ref["running_seq"][:, :, :cur].reshape(B * nb, cur) if cur else None),
                       order, do_sample=sample).view(B, nb * V)
        s.call(o, cur, min_len=min_len, lp=lp, hf431=int(v431), u=u, device_counter=v431)
        top_idx = s.draws.long().cpu()
        what = f"step {cur}"
        if not sample:
            assert top_idx.tolist() == sampling.beam_reference_select(acc.view(B, nb, V), nb, None, False)[1].tolist(), what
        top_lp = acc.gather(1, top_idx)
        assert bool((top_lp > NEG_INF).all()) and all(len(set(r)) == 2 * nb for r in top_idx.tolist()), what
        if sample and v431:
            top_lp, srt = torch.sort(top_lp, descending=True, dim=1, stable=True)
            top_idx = top_idx.gather(1, srt)
        toks, flat = sampling.beam_scorer_step(ref, top_lp, top_idx, V, cur, max_len, lp, bc.EOS, v431)[:2]
        assert_beam_state(s, ref, toks, flat, what)
    assert bool(ref["finished"].any())                                       # the scenario did finish hypotheses
    snap = [t_.clone() for t_ in s.outputs()]
    s.call(o, max_len, min_len=min_len, lp=lp, hf431=int(v431), u=u, device_counter=True)
    assert all(torch.equal(a_, b_) for a_, b_ in zip(snap, s.outputs()))     # a replay at the length limit is a no-op


# ------------------------------------------------------------------------------------------------ 8. rejections
def test_rejections_leave_every_output_unwritten():
    B, nb, V = 1, 2, 64
    s = Step(B, nb, V, 8)
    s.set_logits(bc.rows(B, nb, V, 1))
    u = torch.full((1, B, 2 * nb), 0.5, device=DEV)
    o = dict(top_p=0.9)
    snap = [t_.clone() for t_ in s.outputs()]
    from emu_amd._lib import SAMPLE_MAX_VOCAB
    for bad in (dict(V=SAMPLE_MAX_VOCAB + 1), dict(V=3), dict(nb=9), dict(L=257), dict(ws=None), dict(ws_bytes=s.ws.numel() - 4),
                dict(run=None), dict(uni=None)):
        s.call(o, 0, u=u, want=-22, **bad)
        assert all(torch.equal(a_, b_) for a_, b_ in zip(snap, s.outputs())), bad
    s.call(o, 0, u=u)                                                        # and the same call within the range runs
    assert int(s.draws.min()) >= 0 and bool((s.acc != 7.0).all())


# ------------------------------------------------------------------------------------------------ 9. the loop on the tiny model
@pytest.fixture(scope="module")
def tiny_model(golden_dir):
    from emu_amd import EmuModel, TextDecoderCfg
    z = tiny.load(golden_dir, "generate_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    m = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda", device_sampler=False, device_beam_sampler=False)
    m.load_state_dict(W, strict=True)
    return m, z


@pytest.fixture(scope="module")
def prompts(tiny_model):
    """B -> (embeds [B, S, hidden], mask): one prompt with an image, two ragged left-padded text prompts."""
    m, z = tiny_model
    ids1, ids2 = _t(z["ids1"]), _t(z["ids2"])
    x1 = m._prompt_embeds(ids1, _t(z["image"]).cuda(), m.n_query).view(1, ids1.shape[1], -1)
    x2 = m._prompt_embeds(ids2, None, m.n_query).view(2, ids2.shape[1], -1)
    return {1: (x1, _t(z["mask1"])), 2: (x2, _t(z["mask2"]))}


NB, N_NEW, MIN_LEN = 3, 8, 3
DEMO = dict(do_sample=True, temperature=0.7, top_k=3, top_p=0.9, length_penalty=1.0)


def table(seed, B, n_new=N_NEW, nb=NB):
    return torch.rand(n_new, B, 2 * nb, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


# (order, B, repetition penalty) -> the first seed of table() under which every draw of the HOST loop keeps 5e-4 of mass between
# u * R and the nearest boundary and every pruning decision 1e-3 of score; screened on the host path alone, the device loop unseen:
# for seed in range(60): beam_search_generate(uniforms=table(seed, B), trace=tr) -> tr["draw_margin"], tr["margin"]
LOOP_SEEDS = {('5.x', 1, 1.0): 0, ('5.x', 1, 1.2): 2, ('5.x', 2, 1.0): 1, ('5.x', 2, 1.2): 0,
              ('4.31', 1, 1.0): 2, ('4.31', 1, 1.2): 0, ('4.31', 2, 1.0): 0, ('4.31', 2, 1.2): 6}
EOS_SEEDS = {'5.x': (1, 22258), '4.31': (0, 10724)}           # order -> (seed, eos id): a run whose stand-in EOS ends a hypothesis early


def _host(lm, x, mask, seed, B, **kw):
    tr = {}
    out = lm.beam_search_generate(x, mask, NB, N_NEW, min_len=MIN_LEN, uniforms=table(seed, B), trace=tr, **kw)
    return out.cpu().tolist(), tr


@pytest.mark.parametrize("pen", [1.0, 1.2])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("order", bc.ORDERS)
def test_device_loop_returns_the_host_loops_ids(tiny_model, prompts, order, B, pen):
    """beam_search_generate(device_beam_sampler=True, uniforms=U) returns the ids of beam_search_generate(uniforms=U): eagerly
    launched and replayed from the captured graph.  The host run's trace must show that no draw sat within 1e-4 of a boundary."""
    lm = tiny_model[0].decoder.lm
    x, mask = prompts[B]
    kw = dict(DEMO, repetition_penalty=pen, hf_semantics=order)
    seed = LOOP_SEEDS[(order, B, pen)]
    want, tr = _host(lm, x, mask, seed, B, **kw)
    print(f"{order} B={B} pen={pen}: draw margin {tr['draw_margin']:.2e}, pruning margin {tr['margin']:.2e}")
    assert tr["draw_margin"] >= 1e-4 and tr["margin"] >= 1e-4
    for graph in (False, True):
        lm.beam_graph = graph
        got = lm.beam_search_generate(x, mask, NB, N_NEW, min_len=MIN_LEN, uniforms=table(seed, B).cuda(), device_beam_sampler=True,
                                      **kw)
        lm.beam_graph = True
        assert got.cpu().tolist() == want, (graph, got.cpu().tolist(), want)


@pytest.mark.parametrize("order", bc.ORDERS)
def test_device_loop_with_an_early_end_and_a_reused_graph(tiny_model, prompts, order, monkeypatch):
    """A token the search does produce plays EOS, so a hypothesis ends early and the graph is replayed beyond the end of the
    search: same ids as the host loop.  A second call with another table replays the graph captured by the first."""
    lm = tiny_model[0].decoder.lm
    x, mask = prompts[1]
    seed, eos = EOS_SEEDS[order]
    kw = dict(DEMO, hf_semantics=order, eos_id=eos)
    want, tr = _host(lm, x, mask, seed, 1, **kw)
    assert tr["draw_margin"] >= 1e-4 and tr["margin"] >= 1e-4
    captures = []
    real = torch.cuda.graph
    monkeypatch.setattr(torch.cuda, "graph", lambda g, *a, **k: (captures.append(g), real(g, *a, **k))[1])
    lm._drop_loop_states()
    run = lambda s: lm.beam_search_generate(x, mask, NB, N_NEW, min_len=MIN_LEN, uniforms=table(s, 1), device_beam_sampler=True,
                                            **kw).cpu().tolist()
    assert run(seed) == want
    st = lm._loop_states["beam"][1]
    assert len(captures) == 1 and bool(st["finished"].any()) and len(want[0]) < N_NEW and want[0][-1] == eos
    assert len(run(seed + 1)) == 1                                           # another table ...
    assert run(seed) == want and len(captures) == 1                          # ... and the first again: one capture served all three


@pytest.mark.parametrize("order", bc.ORDERS)
def test_penalised_beam_search_on_the_device(tiny_model, prompts, order):
    lm = tiny_model[0].decoder.lm
    for B in (1, 2):
        x, mask = prompts[B]
        kw = dict(repetition_penalty=1.3, hf_semantics=order, length_penalty=1.0, min_len=MIN_LEN)
        tr = {}
        want = lm.beam_search_generate(x, mask, NB, N_NEW, trace=tr, **kw).cpu().tolist()
        print(f"{order} B={B}: pruning margin {tr['margin']:.2e}")
        assert tr["margin"] >= 1e-4
        for graph in (False, True):
            lm.beam_graph = graph
            got = lm.beam_search_generate(x, mask, NB, N_NEW, device_beam_sampler=True, **kw).cpu().tolist()
            lm.beam_graph = True
            assert got == want, (B, graph)


def test_default_table_is_seed_stable(tiny_model, prompts):
    lm = tiny_model[0].decoder.lm
    x, mask = prompts[2]
    outs = []
    for seed in (5, 5, 6):
        torch.manual_seed(seed)
        outs.append(lm.beam_search_generate(x, mask, NB, N_NEW, device_beam_sampler=True, **DEMO).cpu().tolist())
    assert outs[0] == outs[1]


# ------------------------------------------------------------------------------------------------ 10. unchanged paths
def test_with_the_option_off_beam_sampling_returns_what_it_returned_before(tiny_model, prompts, golden_dir):
    """The ids tests/golden/beam_sample_parent_ids_gpu.npz holds were returned on an MI355X by the commit before this option, for
    tests/beam_sampler_cases.py's PARENT_SETS under torch.manual_seed(PARENT_SEED) on the two text prompts."""
    lm = tiny_model[0].decoder.lm
    x, mask = prompts[2]
    z = np.load(os.path.join(golden_dir, "beam_sample_parent_ids_gpu.npz"))
    for name, o in bc.PARENT_SETS.items():
        o = dict(o)
        nb, n_new = o.pop("num_beams"), o.pop("max_new_tokens")
        torch.manual_seed(bc.PARENT_SEED)
        assert lm.beam_search_generate(x, mask, nb, n_new, **o).cpu().tolist() == z[name].tolist(), name


def test_unpenalised_deterministic_search_keeps_its_kernel(tiny_model, prompts, monkeypatch):
    from emu_amd import _lib
    lm = tiny_model[0].decoder.lm
    x, mask = prompts[1]
    L, calls = _lib.lib(), dict(step=0, sample=0)

    class Counting:
        def __getattr__(self, name):
            f = getattr(L, name)
            if name == "emu_beam_step_bf16":
                return lambda *a: (calls.__setitem__("step", calls["step"] + 1), f(*a))[1]
            if name == "emu_beam_sample_step_bf16":
                return lambda *a: (calls.__setitem__("sample", calls["sample"] + 1), f(*a))[1]
            return f
    import emu_amd.llama as LL
    monkeypatch.setattr(LL, "lib", lambda: Counting())
    lm.beam_graph = False
    try:
        a = lm.beam_search_generate(x, mask, NB, 4, device_beam_sampler=True).cpu().tolist()
        assert calls["step"] >= 1 and calls["sample"] == 0
        b = lm.beam_search_generate(x, mask, NB, 4, device_beam_sampler=True, repetition_penalty=1.2).cpu().tolist()
        assert calls["sample"] >= 1
    finally:
        lm.beam_graph = True
    assert a == lm.beam_search_generate(x, mask, NB, 4).cpu().tolist() and len(b) == 1


def test_refusals_on_the_real_engine_come_before_any_device_work(tiny_model, prompts, monkeypatch):
    lm = tiny_model[0].decoder.lm
    x, mask = prompts[1]
    monkeypatch.setattr(lm, "prefill", lambda *a, **k: pytest.fail("device work before the refusal"))
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        lm.beam_search_generate(x, mask, NB, 4, do_sample=True, device_beam_sampler=True, no_repeat_ngram_size=2)
    monkeypatch.setattr(lm.ctx, "tp_size", 2)
    with pytest.raises(ValueError, match="tensor parallelism"):
        lm.beam_search_generate(x, mask, NB, 4, do_sample=True, device_beam_sampler=True)
    with pytest.raises(ValueError, match="uniforms"):
        lm.beam_search_generate(x, mask, NB, 4, do_sample=True, uniforms=torch.zeros(4, 2, 6))
