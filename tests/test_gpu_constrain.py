"""GPU: constrained decoding on the device -- ``emu_beam_step_trie_bf16`` and ``emu_sample_trie_bf16`` against the specification
(emu_amd/sampling.py with ``allowed``, ``sampling.trie_nodes``), and the constrained device loops on the tiny model of
tests/golden/generate_tiny.npz against the host loops on the same engine (forced by ``constraint=trie.as_callable()``)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from emu_amd import llama, sampling
from emu_amd.constrain import TokenTrie
from tests import beam_sampler_cases as bc
from tests import constrain_cases as cc
from tests import tiny
from tests.beam_step_common import BeamBuffers, assert_beam_state, logit_strides
from tests.test_gpu_sampler import DRAW_TOL

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
EOS, PAD = cc.EOS, cc.PAD
BEAM_SHAPES = [(1, 2, 64), (3, 3, 1000), (2, 8, 4099), (2, 5, 32274)]
assert all(s in bc.GPU_SHAPES for s in BEAM_SHAPES)


def _beam_cases(V, nb):
    """name -> (trie, nodes of the B * nb rows as a function of the row index)."""
    out = {name: (trie, (lambda r, n=node: n)) for name, (trie, node) in cc.node_shape_tries(V, nb).items()}
    mixed = TokenTrie([[3, 4], [3, 5, 6], [8], [9, 10]], EOS, V)             # the beams of one prompt at different nodes
    at = [0, mixed.walk([3]), mixed.walk([3, 5]), -1, mixed.walk([9])]
    out["mixed"] = (mixed, lambda r: at[r % len(at)])
    return out


class _BeamState:
    """The state of a search under way at step ``cur`` (CPU reference ``ref`` and device copy ``dev``), for both conventions."""

    def __init__(self, B, nb, V, L, cur, seed):
        g = torch.Generator().manual_seed(seed)
        self.ref = sampling.beam_start_state(B, nb, L, PAD)
        if cur:
            self.ref["running_scores"] = bc.running_scores(B, nb, "5.x")
        self.ref["running_seq"][:, :, :cur] = torch.randint(3, V, (B, nb, cur), generator=g)
        if cur:                                                              # one kept result per prompt, to merge against
            self.ref["sequences"][:, 0, :2] = torch.tensor([5, EOS])
            self.ref["beam_scores"][:, 0] = -9.5
            self.ref["finished"][:, 0] = True
            self.ref["seq_len"][:, 0] = 2
        self.dev = BeamBuffers(self.ref)


def _beam_call(lg, V, cur, counter, min_len, lp, v431, bufs, ws, trie=None, node=None, **override):
    from emu_amd import ops
    from emu_amd._lib import lib
    args = bufs.step_args(lg.data_ptr(), *logit_strides(lg, bufs.B, bufs.nb), V, cur, min_len, EOS, lp, v431, ws, counter, override)
    if trie is None:
        return lib().emu_beam_step_bf16(*args, ops.stream(lg.device))
    return lib().emu_beam_step_trie_bf16(*args, C.byref(trie), node.data_ptr(), ops.stream(lg.device))


@pytest.mark.parametrize("v431", [False, True])
@pytest.mark.parametrize("B,nb,V", BEAM_SHAPES)
def test_beam_step_trie_equals_the_specification(B, nb, V, v431):
    """One step of ``emu_beam_step_trie_bf16`` per node shape, at ``cur = 0`` (the beams share the prompt's row) and at ``cur = 6``
    (a search under way, one kept result to merge against), with the step index from the host and from a device counter: the
    state, ``next_tok``, ``beam_flat`` and the new nodes equal the specification -- ``sampling.beam_reference_rows(allowed=...)``,
    the stable selection, the scorer's bookkeeping, ``child(node[beam it continues], token)``.  Scores to 1e-4, the bound
    tests/test_gpu_beam.py uses for the re-ordered log-sum-exp; -inf is compared as such.  With every id a child the outputs are
    ``emu_beam_step_bf16``'s bit for bit."""
    from emu_amd import ops
    from emu_amd._lib import lib
    L_, lp = 10, -1.0 if not v431 else 1.0
    ws = torch.empty(lib().emu_beam_step_workspace_bytes(B, nb, V), dtype=torch.uint8, device="cuda")
    for cur in (0, 6):
        g = torch.Generator().manual_seed(B * 1000 + nb * 10 + cur)
        x = (torch.randn(B if cur == 0 else B * nb, V, generator=g) * 3.0).to(BF16)
        x[:, EOS] += 6.0                                                     # where EOS is allowed, hypotheses end
        lg = x.cuda()
        rows = x[:, None, :].expand(B, nb, V).reshape(B * nb, V) if cur == 0 else x
        for name, (trie, node_of) in _beam_cases(V, nb).items():
            min_len = 0 if name in ("exhausted", "mixed") else 1             # (EOS alone under the suppress is refused on the host)
            node0 = torch.tensor([node_of(r) for r in range(B * nb)], dtype=torch.int32)
            allowed = torch.zeros(B * nb, V, dtype=torch.bool)
            for r in range(B * nb):
                allowed[r, trie.allowed_at(int(node0[r]))] = True
            for counter in ("host", "device"):
                what = (name, cur, counter)
                st = _BeamState(B, nb, V, L_, cur, seed=7)
                acc = sampling.beam_reference_rows(rows, st.ref["running_scores"], eos_id=EOS, suppress_eos=cur < min_len,
                                                   do_sample=False, allowed=allowed).view(B, nb, V)
                if name in ("fan1", "fan2", "fan2N-1", "exhausted"):             # fewer candidates than 2N outside the -1e9 / -inf tail
                    assert int((acc > -1.0e8).view(B, -1).sum(1).min()) < 2 * nb, what
                top_lp, top_idx = sampling.beam_reference_select(acc, nb, None, False)
                toks, flat, beam_idx = sampling.beam_scorer_step(st.ref, top_lp, top_idx, V, cur, L_, lp, EOS, v431)[:3]
                want_node = [trie.child(int(node0[b * nb + int(beam_idx[b, j])]), int(toks[b * nb + j])) for b in range(B) for j in range(nb)]
                node = node0.cuda()
                tt = ops.trie_tables(trie.tables("cuda"))
                rc = _beam_call(lg, V, cur, counter == "device", min_len, lp, v431, st.dev, ws, tt, node)
                torch.cuda.synchronize()
                assert rc == 0, what
                assert node.cpu().tolist() == want_node, what
                assert_beam_state(st.dev, st.ref, toks, flat, what)
                if name == "all":                                            # nothing is masked: the unconstrained kernel's bits
                    base = _BeamState(B, nb, V, L_, cur, seed=7)
                    assert _beam_call(lg, V, cur, counter == "device", min_len, lp, v431, base.dev, ws) == 0
                    torch.cuda.synchronize()
                    for a_, b_ in zip(st.dev.state(), base.dev.state()):
                        assert torch.equal(a_.view(torch.uint8), b_.view(torch.uint8)), what
    # a replay at the length limit changes nothing, the nodes included
    snap = [t.clone() for t in st.dev.state()] + [node.clone()]
    assert _beam_call(lg, V, L_, True, 0, lp, v431, st.dev, ws, tt, node) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a_, b_) for a_, b_ in zip(snap, list(st.dev.state()) + [node]))


def test_trie_entry_points_refuse_bad_tables_before_any_launch():
    from emu_amd import ops
    from emu_amd._lib import TokenTrieC, lib
    from emu_amd.llama import sample_params
    V = 64
    trie = TokenTrie([[5]], EOS, V)
    first, tok, child = trie.tables("cuda")
    good = ops.trie_tables((first, tok, child))
    st = _BeamState(1, 2, V, 8, 0, seed=1)
    snap = [t.clone() for t in st.dev.state()]
    lg = torch.zeros(1, V, dtype=BF16, device="cuda")
    ws = torch.empty(lib().emu_beam_step_workspace_bytes(1, 2, V), dtype=torch.uint8, device="cuda")
    node = torch.zeros(2, dtype=torch.int32, device="cuda")
    bad = [TokenTrieC(None, tok.data_ptr(), child.data_ptr(), 1, 2), TokenTrieC(first.data_ptr(), None, child.data_ptr(), 1, 2),
           TokenTrieC(first.data_ptr(), tok.data_ptr(), None, 1, 2), TokenTrieC(first.data_ptr(), tok.data_ptr(), child.data_ptr(), 0, 2),
           TokenTrieC(first.data_ptr(), tok.data_ptr(), child.data_ptr(), 1, -1)]
    out = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    p = sample_params(False, None, None, None, 1.0, None, 0, EOS, PAD)
    sample = lambda t, n: lib().emu_sample_trie_bf16(lg.data_ptr(), V, 1, V, None, 0, 0, step.data_ptr(), None, 0, 0, C.byref(p), None,
                                                     out.data_ptr(), None, 0, t, n, ops.stream(lg.device))
    for t in bad:
        assert _beam_call(lg, V, 0, False, 0, 1.0, False, st.dev, ws, t, node) == -22
        assert sample(C.byref(t), node.data_ptr()) == -22
    assert sample(None, node.data_ptr()) == -22 and sample(C.byref(good), None) == -22
    assert _beam_call(lg, V, 0, False, 0, 1.0, False, st.dev, ws, good, node, nb=9) == -22                # the base entry point's bounds
    torch.cuda.synchronize()
    assert all(torch.equal(a_, b_) for a_, b_ in zip(snap, st.dev.state())) and out.cpu().tolist() == [-7] and node.cpu().tolist() == [0, 0]
    # a node outside [-1, nodes) at entry is the exhausted node, not an address
    node = torch.tensor([7, -5], dtype=torch.int32, device="cuda")
    lg2 = torch.zeros(2, V, dtype=BF16, device="cuda")
    out2 = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    assert lib().emu_sample_trie_bf16(lg2.data_ptr(), V, 2, V, None, 0, 0, step.data_ptr(), None, 0, 0, C.byref(p), None, out2.data_ptr(),
                                      None, 0, C.byref(good), node.data_ptr(), ops.stream(lg.device)) == 0
    torch.cuda.synchronize()
    assert out2.cpu().tolist() == [EOS, EOS] and node.cpu().tolist() == [-1, -1]


# ---- emu_sample_trie_bf16
SAMPLE_VOCABS = (64, 1000, 4099, 32274, 40000)
SAMPLE_OPTS = dict(temperature=0.7, top_k=50)


@functools.lru_cache(maxsize=None)
def _sample_rows(V):
    return (torch.randn(5, V, generator=torch.Generator().manual_seed(V)) * 3.0).to(BF16)


def _sample(x, trie, node, do_sample, step=0, uniforms=None, unfinished=None, probs=False, hist=None, penalty=1.0, constrained=True):
    from emu_amd import ops
    from emu_amd.llama import sample_params
    R, V = x.shape
    step_dev = torch.tensor([step], dtype=torch.int32, device="cuda")
    pr = torch.full((R, V), -1.0, dtype=torch.float32, device="cuda") if probs else None
    p = sample_params(do_sample, SAMPLE_OPTS["temperature"], SAMPLE_OPTS["top_k"], None, penalty, EOS, 0, EOS, PAD)
    kw = dict(trie=ops.trie_tables(trie.tables("cuda")), node=node) if constrained else {}
    out = ops.sample(x.cuda(), step_dev, p, hist=hist, uniforms=uniforms, unfinished=unfinished, probs_out=pr, **kw)
    torch.cuda.synchronize()
    return out.cpu().long(), (pr.cpu() if probs else None)


@pytest.mark.parametrize("V", SAMPLE_VOCABS)
def test_sample_trie_follows_the_specification(V):
    """Per node shape, 5 rows: the greedy ids are the spec's exactly (under a repetition penalty over a history too); ``probs_out``
    is positive exactly on the spec's kept set; the nodes advance by ``child(node, id)``; 64 rows of one logit row under 64
    uniforms draw inside the fp64 interval of the constrained spec (tests/test_gpu_sampler.py's rule and tolerance); with every
    id a child the outputs are ``emu_sample_bf16``'s bit for bit.  V = 40 000 is the bound at which the row fills the LDS."""
    x = _sample_rows(V)
    hist_ids = torch.tensor([[5, 5, 17], [0, 1, 1], [V + 3] * 3, [7, 7, 7], [3, 9, 27]], dtype=torch.int64)
    hist = hist_ids.t().to(torch.int32).contiguous().cuda()
    u64 = torch.rand(64, generator=torch.Generator().manual_seed(V + 1), dtype=torch.float32)
    u64[0], u64[1] = 0.0, 1 - 2.0 ** -24
    for name, (trie, n0) in cc.node_shape_tries(V, 5).items():
        allowed = torch.zeros(5, V, dtype=torch.bool)
        allowed[:, trie.allowed_at(n0)] = True
        node = torch.full((5,), n0, dtype=torch.int32, device="cuda")
        got, _ = _sample(x, trie, node, False)
        want = sampling.reference_greedy(x, allowed=allowed)
        assert got.tolist() == want.tolist(), name
        assert node.cpu().tolist() == [trie.child(n0, int(t)) for t in got], name
        node.fill_(n0)
        got, _ = _sample(x, trie, node, False, step=3, hist=hist, penalty=1.3)
        assert got.tolist() == sampling.reference_greedy(x, hist_ids, 1.3, allowed=allowed).tolist(), name
        # sampling: the kept set, then the draws
        node.fill_(n0)
        uni = torch.full((1, 5), 0.5, device="cuda")
        tok, pr = _sample(x, trie, node, True, uniforms=uni, probs=True)
        q64 = sampling.reference_probs(x, dtype=torch.float64, allowed=allowed, **SAMPLE_OPTS)
        assert torch.equal(pr > 0, q64 > 0) and float((pr.double() - q64).abs().max()) <= 1e-5, name
        assert bool(allowed.gather(1, tok[:, None]).all()) and node.cpu().tolist() == [trie.child(n0, int(t)) for t in tok], name
        node64 = torch.full((64,), n0, dtype=torch.int32, device="cuda")
        tok, _ = _sample(x[:1].expand(64, V).contiguous(), trie, node64, True, uniforms=u64[None].cuda())
        lo, hi = sampling.reference_intervals(q64[:1])
        lo_t, hi_t, ud = lo[0, tok], hi[0, tok], u64.double()
        assert bool((q64[0, tok] > 0).all()), name
        assert bool(((ud >= lo_t - DRAW_TOL) & (ud <= hi_t + DRAW_TOL)).all()), (name, float(torch.maximum(lo_t - ud, ud - hi_t).max()))
        assert int(tok[0]) == int((q64[0] > 0).nonzero()[0])                 # u = 0: the lowest kept id
        if name == "all":
            node.fill_(n0)
            for do_sample in (False, True):
                a, pa = _sample(x, trie, node, do_sample, uniforms=uni, probs=do_sample)
                b, pb = _sample(x, trie, None, do_sample, uniforms=uni, probs=do_sample, constrained=False)
                assert torch.equal(a, b) and (pa is None or torch.equal(pa.view(torch.int32), pb.view(torch.int32)))
                node.fill_(n0)


def test_sample_trie_finished_row_keeps_its_node():
    V = 1000
    x = _sample_rows(V)
    trie, n0 = cc.node_shape_tries(V, 5)["fan2N+3"]
    for do_sample in (False, True):
        node = torch.tensor([0, 0, 0, -1, 0], dtype=torch.int32, device="cuda")
        flags = torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32, device="cuda")
        tok, _ = _sample(x, trie, node, do_sample, uniforms=torch.full((1, 5), 0.3, device="cuda"), unfinished=flags)
        assert tok[1] == PAD and tok[4] == PAD and int(tok[3]) == EOS        # row 3 is exhausted: EOS, and that finishes it
        assert flags.cpu().tolist() == [1, 0, 1, 0, 0]
        assert node.cpu().tolist() == [trie.child(0, int(tok[0])), 0, trie.child(0, int(tok[2])), -1, 0]


# ---- the loops on the tiny model
@pytest.fixture(scope="module")
def tiny_model(golden_dir):
    from emu_amd import EmuModel, TextDecoderCfg
    z = tiny.load(golden_dir, "generate_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    m = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda", device_sampler=False)
    m.load_state_dict(W, strict=True)
    ids2 = torch.from_numpy(np.asarray(z["ids2"]))
    x = m._prompt_embeds(ids2, None, m.n_query).view(2, ids2.shape[1], -1)
    return m, z, x, torch.from_numpy(np.asarray(z["mask2"])), vocab


# (sequences, seed): screened on the CPU stand-in (tests/fake_engine.py, fp32): the host loop's margin on the two text prompts of the
# fixture is 10.8 / 2.8 nat for the small tries with 5 beams and 0.20 / 0.16 nat for the big ones (5 beams, lp -1 / 3 beams, lp 0)
LOOP_TRIES = {"small5": (4, 3, 5), "small3": (4, 3, 3), "big13": (300, 4, 13), "big11": (300, 4, 11)}
LOOP_MARGIN = 10 * bc.MARGIN


def _loop_trie(name, vocab):
    n, length, seed = LOOP_TRIES[name]
    return TokenTrie(cc.random_sequences(n, length, vocab, seed), EOS, vocab)


def _members(trie_seqs, ids):
    for row in ids.tolist():
        assert EOS in row and tuple(row[:row.index(EOS)]) in trie_seqs, row
        assert all(t == PAD for t in row[row.index(EOS) + 1:]), row


def test_constrained_beam_loop_equals_the_host_loop(tiny_model, monkeypatch):
    """The constrained device beam loop, eager and replayed, returns the ids of the host loop on the same engine; with ``BEAM_POLL``
    above the answer's length the replays past the end change nothing.  Two tries of different sizes in a row, then an
    unconstrained call: the key, the re-capture and the state left behind."""
    m, z, x, mask, vocab = tiny_model
    lm = m.decoder.lm
    monkeypatch.setattr(llama.LlamaEngine, "BEAM_POLL", 7)
    free = lm.beam_search_generate(x, mask, 5, 8, hf_semantics="5.x").cpu().tolist()
    for name, nb, lp in (("small5", 5, -1.0), ("big13", 5, -1.0), ("big11", 3, 0.0), ("small3", 5, -1.0)):
        trie = _loop_trie(name, vocab)
        seqs = {tuple(s) for s in cc.random_sequences(*LOOP_TRIES[name][:2], vocab, LOOP_TRIES[name][2])}
        tr = {}
        host = lm.beam_search_generate(x, mask, nb, 8, length_penalty=lp, hf_semantics="5.x", constraint=trie.as_callable(), trace=tr).cpu()
        print(f"{name} {nb} beams: host margin {tr['margin']:.4f}")
        assert tr["margin"] > LOOP_MARGIN, (name, tr)                        # the precondition: chosen so on the CPU stand-in
        _members(seqs, host)
        for graph in (False, True):
            monkeypatch.setattr(lm, "beam_graph", graph, raising=False)
            got = lm.beam_search_generate(x, mask, nb, 8, length_penalty=lp, hf_semantics="5.x", constraint=trie).cpu()
            assert got.tolist() == host.tolist(), (name, graph)
        ret = lm.beam_search_generate(x, mask, nb, 8, length_penalty=lp, hf_semantics="5.x", constraint=trie, num_return_sequences=2).cpu()
        assert ret[0::2].tolist() == [r + [PAD] * (ret.shape[1] - len(r)) for r in host.tolist()], name       # the best of two
        _members(seqs, ret)
    assert lm.beam_search_generate(x, mask, 5, 8, hf_semantics="5.x").cpu().tolist() == free      # the unconstrained call after them


def test_constrained_one_beam_loop(tiny_model):
    """Constrained greedy on the device, eager and replayed, equals the host loop on the same engine; with injected uniforms every
    id lies in the fp64 interval of the constrained spec on that step's logits, the same uniforms give the same ids eager and
    replayed, and every answer is a member of the trie."""
    from tests.test_gpu_device_sampler import _step_logits
    m, z, x, mask, vocab = tiny_model
    lm = m.decoder.lm
    for name in ("small5", "big13"):
        trie = _loop_trie(name, vocab)
        seqs = {tuple(s) for s in cc.random_sequences(*LOOP_TRIES[name][:2], vocab, LOOP_TRIES[name][2])}
        host = lm.sample_generate(x, mask, 8, do_sample=False, pad_id=PAD, constraint=trie.as_callable()).cpu()
        _members(seqs, host)
        for graph in (False, True):
            got = lm.sample_generate(x, mask, 8, do_sample=False, pad_id=PAD, device_sampler=True, use_graph=graph, constraint=trie).cpu()
            assert got.tolist() == host.tolist(), (name, graph)
        uni = torch.rand(8, 2, generator=torch.Generator().manual_seed(5), dtype=torch.float32).cuda()
        o = dict(temperature=1.5, top_k=50)
        ids = lm.sample_generate(x, mask, 8, do_sample=True, pad_id=PAD, device_sampler=True, uniforms=uni, constraint=trie, **o).cpu()
        _members(seqs, ids)
        u = uni.cpu().double()
        done = torch.zeros(2, dtype=torch.bool)
        for step, lg in enumerate(_step_logits(lm, x, mask, ids.clamp(max=vocab - 1))):
            allowed = sampling.constraint_allowed(trie, ids[:, :step])
            q = sampling.reference_probs(lg, suppress_id=EOS if step < 1 else None, allowed=allowed, dtype=torch.float64, **o)
            lo, hi = sampling.reference_intervals(q)
            for r in range(2):
                if not done[r]:
                    t = int(ids[r, step])
                    assert float(q[r, t]) > 0 and lo[r, t] - DRAW_TOL <= u[step, r] <= hi[r, t] + DRAW_TOL, (name, step, r)
            done |= ids[:, step] == EOS
        again = lm.sample_generate(x, mask, 8, do_sample=True, pad_id=PAD, device_sampler=True, uniforms=uni, use_graph=True,
                                   constraint=trie, **o).cpu()
        assert again.tolist() == ids.tolist(), name


def _count_calls(monkeypatch):
    """Spy on the C entry points ``emu_amd.llama`` calls: the names, in order."""
    from emu_amd import _lib
    real, calls = _lib.lib(), []

    class Counting:
        def __getattr__(self, name):
            f = getattr(real, name)
            if name in ("emu_beam_step_trie_bf16", "emu_llama_sample_step_trie", "emu_beam_step_bf16", "emu_llama_sample_step"):
                return lambda *a: (calls.append(name), f(*a))[1]
            return f
    monkeypatch.setattr(llama, "lib", lambda: Counting())
    return calls


def test_models_reach_the_constrained_device_loop(tiny_model, monkeypatch):
    m, z, x, mask, vocab = tiny_model
    trie = _loop_trie("small5", vocab)
    seqs = {tuple(s) for s in cc.random_sequences(*LOOP_TRIES["small5"][:2], vocab, 5)}
    ids2 = torch.from_numpy(np.asarray(z["ids2"]))
    calls = _count_calls(monkeypatch)
    out = m.generate_ids(ids2, mask, max_new_tokens=8, num_beams=5, hf_semantics="5.x", constraint=trie).cpu()
    assert "emu_beam_step_trie_bf16" in calls and "emu_beam_step_bf16" not in calls
    _members(seqs, out)
    calls.clear()
    monkeypatch.setattr(m, "device_sampler", True)
    out = m.generate_ids(ids2, mask, max_new_tokens=8, num_beams=1, hf_semantics="5.x", constraint=trie).cpu()
    assert "emu_llama_sample_step_trie" in calls and "emu_llama_sample_step" not in calls
    _members(seqs, out)
    calls.clear()
    m.generate_ids(ids2, mask, max_new_tokens=4, num_beams=5, hf_semantics="5.x", constraint=trie.as_callable())    # a callable: the host loop
    assert not calls


def test_emu1_reaches_the_constrained_device_loop(golden_dir, monkeypatch):
    from emu_amd.emu1 import Emu
    z = tiny.load(golden_dir, "emu1_generate_tiny.npz")
    v, t5, l, vocab, W, ocfg = tiny.emu1_generate_from(z)
    m = Emu(v, l, t5, vocab=vocab, device="cuda")
    m.load_state_dict(W, strict=True)
    ids, mask, img = torch.from_numpy(z["ids"]), torch.from_numpy(z["mask"]), torch.from_numpy(z["image"])
    seq = cc.random_sequences(4, 3, vocab, 5)
    trie = TokenTrie(seq, EOS, vocab)
    calls = _count_calls(monkeypatch)
    out = m.generate_ids(ids, mask, img.cuda(), num_beams=5, max_new_tokens=8, constraint=trie).cpu()
    assert "emu_beam_step_trie_bf16" in calls and "emu_beam_step_bf16" not in calls
    for row in out.tolist():
        assert tuple(row[:row.index(EOS)]) in {tuple(s) for s in seq}, row
