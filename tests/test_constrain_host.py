"""CPU: constrained decoding on the host -- ``emu_amd.constrain.TokenTrie``, its place in the specification (emu_amd/sampling.py) and in
``process_logits``, the host loops against the installed library's ``generate(prefix_allowed_tokens_fn=...)`` through the CPU
stand-in engine, and where a constrained call is routed or refused."""
import itertools
import types
import warnings

import pytest
import torch

from emu_amd import sampling
from emu_amd.constrain import TokenTrie
from tests import beam_sampler_cases as bc
from tests import constrain_cases as cc

EOS = cc.EOS


def _brute_allowed(seqs, eos, prefix):
    """The definition: the next ids of the stored sequences (each with its EOS) that start with ``prefix``; none -> {eos}."""
    full = [tuple(s) + (() if s[-1] == eos else (eos,)) for s in seqs]
    nxt = sorted({s[len(prefix)] for s in full if len(s) > len(prefix) and s[:len(prefix)] == tuple(prefix)})
    return nxt or [eos]


@pytest.mark.parametrize("seed", range(6))
def test_allowed_agrees_with_a_brute_force_prefix_scan(seed):
    """Random sets over a small alphabet (so that prefixes are shared, sequences repeat and one is a prefix of another): every
    prefix of every sequence, each of them with one wrong id appended, and complete sequences with ids after their EOS."""
    g = torch.Generator().manual_seed(seed)
    V = 9
    seqs = [[int(t) for t in torch.randint(3, V, (int(torch.randint(1, 5, (1,), generator=g)),), generator=g)] for _ in range(12)]
    trie = TokenTrie(seqs, EOS, V)
    fn = trie.as_callable()
    prefixes = {tuple(s[:n]) for s in seqs for n in range(len(s) + 1)}
    prefixes |= {p + (t,) for p in list(prefixes) for t in (0, 1, 8)} | {tuple(s) + (EOS,) for s in seqs} | {tuple(s) + (EOS, 0) for s in seqs}
    for p in sorted(prefixes):
        want = _brute_allowed(seqs, EOS, p)
        assert trie.allowed(list(p)) == want, p
        assert fn(0, torch.tensor(p, dtype=torch.long)) == want, p
    assert trie.count == len({tuple(s) for s in seqs}) and trie.min_depth == min(len(s) for s in seqs)


def test_shared_prefixes_duplicates_and_validation():
    trie = TokenTrie(cc.LIB_SEQS + [[20], [10, 11, EOS]], EOS, 64)           # a duplicate, and one given with its EOS
    assert trie.count == 5 and trie.min_depth == 1
    assert trie.allowed([]) == [10, 20, 21]
    assert trie.allowed([10]) == [11, 12]
    assert trie.allowed([10, 11]) == [EOS, 30]                               # [10, 11] is complete AND a prefix of [10, 11, 30]
    assert trie.allowed([10, 11, EOS]) == [EOS] and trie.allowed([10, 11, 30, EOS, EOS]) == [EOS]     # past the EOS
    assert trie.allowed([11]) == [EOS] and trie.allowed([10, 13, 5]) == [EOS]                         # off the trie
    for bad, what in (([[3, 64]], "vocab"), ([[-1]], "vocab"), ([[]], "empty"), ([[EOS]], "empty"), ([[3, EOS, 4]], "inside"), ([], "least")):
        with pytest.raises(ValueError, match=what):
            TokenTrie(bad, EOS, 64)
    with pytest.raises(ValueError):
        TokenTrie([[3]], 64, 64)
    with pytest.raises(AttributeError):
        trie.eos_id = 3                                                      # immutable


def test_tables_round_trip_and_trie_nodes_equal_the_stateless_walk():
    for seqs, V in ((cc.LIB_SEQS, 64), (cc.random_sequences(200, 6, 50, 3), 50), ([[t] for t in range(40) if t != EOS], 40)):
        trie = TokenTrie(seqs, EOS, V)
        first, tok, child = trie.tables()
        assert all(t.dtype == torch.int32 for t in (first, tok, child)) and trie.tables()[0] is first      # made once
        assert first.numel() == trie.nodes + 1 and tok.numel() == child.numel() == trie.edges and int(first[0]) == 0
        for n in range(trie.nodes):
            ids = tok[int(first[n]):int(first[n + 1])].tolist()
            assert ids == sorted(set(ids)) and ids                           # ascending within a node, no empty node
        assert int(child.min()) >= -1 and int(child.max()) < trie.nodes
        assert TokenTrie.sequences_of(first, tok, child) == sorted({tuple(s) + (EOS,) for s in seqs})
        # the state the kernels keep: node' = child(node, id), from the root; against the walk of the ids from scratch
        hist = [list(s) + [EOS, 0] for s in seqs[:20]] + [[V - 1, 3], []]
        for ids in hist:
            node = 0
            for n in range(len(ids) + 1):
                assert int(sampling.trie_nodes(trie, [ids[:n]])[0]) == node == trie.walk(ids[:n]), (ids, n)
                assert sampling.constraint_allowed(trie, [ids[:n]])[0].nonzero().flatten().tolist() == _brute_allowed(seqs, EOS, ids[:n])
                if n < len(ids):
                    node = trie.child(node, ids[n])


def test_specification_takes_the_mask_after_the_suppress():
    """``allowed=None`` is the old result bit for bit; with a mask the arg-max, the kept set and the probabilities live on the
    allowed ids, and the beam rows keep the log-sum-exp of the WHOLE row."""
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(3, 64, generator=g) * 3).to(torch.bfloat16)
    trie = TokenTrie(cc.LIB_SEQS, EOS, 64)
    allowed = sampling.constraint_allowed(trie, [[], [10], [10, 11]])
    o = dict(temperature=0.7, top_k=5, top_p=0.9)
    assert torch.equal(sampling.reference_probs(x, **o), sampling.reference_probs(x, allowed=None, **o))
    q = sampling.reference_probs(x, allowed=allowed, **o)
    assert bool(((q > 0) <= allowed).all()) and torch.allclose(q.sum(-1), torch.ones(3))
    gr = sampling.reference_greedy(x, suppress_id=EOS, allowed=allowed)
    assert gr.tolist() == [int(x[r].float().masked_fill(~allowed[r], -1e30).argmax()) for r in (0, 1)] + [30]    # row 2: EOS suppressed
    rs = torch.tensor([0.0, -1.0, -2.0])
    free = sampling.beam_reference_rows(x, rs, do_sample=False)
    acc = sampling.beam_reference_rows(x, rs, do_sample=False, allowed=allowed)
    assert torch.equal(acc[allowed], free[allowed]) and bool(torch.isinf(acc[~allowed]).all())


def test_process_logits_equals_the_library_processor():
    """``process_logits(allowed=...)`` against transformers' PrefixConstrainedLogitsProcessor in the library's order -- penalty,
    min length, constraint, warpers -- element for element."""
    lp = pytest.importorskip("transformers.generation.logits_process")
    from emu_amd.llama import allowed_mask, process_logits
    g = torch.Generator().manual_seed(7)
    V, nb = 64, 2
    trie = TokenTrie(cc.LIB_SEQS, EOS, V)
    fn = trie.as_callable()
    for gen, rp, min_len, sample in (([[], [], [], []], 1.0, 0, False), ([[10], [20], [21], [5]], 1.3, 3, False),
                                     ([[10, 11], [10, 12], [21, 22], [20, EOS]], 1.2, 1, True), ([[10, 11], [10, 12], [21, 22], [20, EOS]], 1.0, 5, False)):
        ids = torch.tensor(gen, dtype=torch.long).reshape(4, -1)
        scores = torch.randn(4, V, generator=g) * 3
        want = scores.clone()
        if rp != 1.0 and ids.shape[1]:
            want = lp.RepetitionPenaltyLogitsProcessor(rp)(ids, want)
        want = lp.MinLengthLogitsProcessor(min_len, EOS)(ids, want)
        want = lp.PrefixConstrainedLogitsProcessor(fn, nb)(ids, want)
        if sample:
            want = lp.TopKLogitsWarper(3)(ids, lp.TemperatureLogitsWarper(0.7)(ids, want))
        got = process_logits(scores.clone(), ids, ids.shape[1] < min_len, EOS, sample, 0.7, 3, None, rp,
                             allowed=allowed_mask(fn, ids, nb, V))
        assert torch.equal(torch.isinf(got), torch.isinf(want))
        assert torch.equal(got[~torch.isinf(want)], want[~torch.isinf(want)])
        assert torch.equal(process_logits(scores.clone(), ids, False, EOS, False), scores)          # no constraint: untouched
    with pytest.raises(ValueError, match="empty list"):
        allowed_mask(lambda b, ids: [], torch.zeros(1, 0, dtype=torch.long), 1, V)


# ---- the host loops against the installed library
LIB_PAD = 1        # inside the tiny vocabulary (the library embeds nothing with it, but checks it), and not 0: the library's beam search
                   # fills its outputs with `pad_token_id or eos_token_id`
LIB_MODES = {"greedy": dict(num_beams=1), "beam5": dict(num_beams=5, length_penalty=0.0),
             "beam3_ret3": dict(num_beams=3, length_penalty=-1.0, num_return_sequences=3)}
LIB_SEEDS = (1, 2, 3)      # screened: the host loop's margins on these lie between 2.8 and 68 nat (the bound is bc.MARGIN = 1e-4)


def _stand_in(monkeypatch):
    from emu_amd import llama as L, ops
    monkeypatch.setattr(L, "BF16", torch.float32)
    monkeypatch.setattr(ops, "embed_gather", lambda ids, table, out=None: out.copy_(table[ids.long()]))
    return L


@pytest.mark.parametrize("mode,seed", list(itertools.product(LIB_MODES, LIB_SEEDS)))
def test_host_loops_return_the_ids_of_the_installed_library(monkeypatch, mode, seed):
    """A tiny random LlamaForCausalLM under ``generate(inputs_embeds=..., prefix_allowed_tokens_fn=trie.as_callable())`` and the
    product's host loops on the same weights (tests/fake_engine.py, hf_semantics="5.x"), a ragged batch of two prompts: equal ids.
    The trie leaves fewer finite candidates than 2N at every step, so dead beams, -inf candidates and the EOS-on-exhaustion rule
    are all in play."""
    pytest.importorskip("transformers")
    L = _stand_in(monkeypatch)
    from tests.fake_engine import FakeEngine
    hf, W, l, r = cc.tiny_llama(seed)
    trie = TokenTrie(cc.LIB_SEQS, EOS, 64)
    x = torch.randn(2, 5, 32, generator=torch.Generator().manual_seed(seed))
    mask = torch.ones(2, 5, dtype=torch.long)
    mask[1, :2] = 0
    kw = dict(LIB_MODES[mode])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = hf.generate(inputs_embeds=x, attention_mask=mask, max_new_tokens=8, do_sample=False, min_length=0, early_stopping=False,
                           prefix_allowed_tokens_fn=trie.as_callable(), pad_token_id=LIB_PAD, eos_token_id=EOS, **kw)
    nb = kw.pop("num_beams")
    eng = FakeEngine(l, 64, W, r)
    if nb == 1:
        got = L.LlamaEngine.sample_generate(eng, x, mask, 8, min_len=0, do_sample=False, eos_id=EOS, pad_id=LIB_PAD, constraint=trie)
    else:
        tr = {}
        got = L.LlamaEngine.beam_search_generate(eng, x, mask, nb, 8, min_len=0, eos_id=EOS, pad_id=LIB_PAD, hf_semantics="5.x",
                                                 trace=tr, constraint=trie, **kw)
        print(f"{mode} seed {seed}: margin {tr['margin']:.3f}")
        assert tr["margin"] > bc.MARGIN, tr
        # the callable form gives the same answer as the trie itself
        again = L.LlamaEngine.beam_search_generate(FakeEngine(l, 64, W, r), x, mask, nb, 8, min_len=0, eos_id=EOS, pad_id=LIB_PAD,
                                                   hf_semantics="5.x", constraint=trie.as_callable(), **kw)
        assert again.tolist() == got.tolist()
    assert got.tolist() == want.tolist()
    seqs = {tuple(s) + (EOS,) for s in cc.LIB_SEQS}
    for row in got.tolist():
        assert tuple(row[:row.index(EOS) + 1]) in seqs, row


# ---- routing and refusals
class _Spy(Exception):
    pass


def _engine(monkeypatch, seed=1):
    """The stand-in dressed as the device engine (it has a ``handle``), its device loops replaced by a spy."""
    from tests.fake_engine import FakeEngine
    L = _stand_in(monkeypatch)
    hf, W, l, r = cc.tiny_llama(seed)
    eng = FakeEngine(l, 64, W, r)
    eng.handle, eng.ctx.tp_size, eng.calls = 1, 1, []

    def spy(name):
        def f(*a, **k):
            eng.calls.append((name, k.get("trie", a[-1] if name == "sample" else None)))
            raise _Spy(name)
        return f
    eng._beam_search_device, eng._sample_device = spy("beam"), spy("sample")
    x = torch.randn(1, 4, 32, generator=torch.Generator().manual_seed(seed))
    return L, eng, x, torch.ones(1, 4, dtype=torch.long)


def test_engine_routing(monkeypatch):
    L, eng, x, mask = _engine(monkeypatch)
    trie = TokenTrie(cc.LIB_SEQS, EOS, 64)
    beam = lambda **k: L.LlamaEngine.beam_search_generate(eng, x, mask, 3, 6, min_len=0, eos_id=EOS, pad_id=LIB_PAD, hf_semantics="5.x", **k)
    one = lambda **k: L.LlamaEngine.sample_generate(eng, x, mask, 6, min_len=0, eos_id=EOS, pad_id=LIB_PAD, **k)
    with pytest.raises(_Spy):                                   # a trie, deterministic and unpenalised: the device loop, with the trie
        beam(constraint=trie)
    assert eng.calls[-1] == ("beam", trie)
    with pytest.raises(_Spy):                                   # no constraint: the path it took before, without a trie
        beam()
    assert eng.calls[-1] == ("beam", None)
    n = len(eng.calls)
    host = beam(constraint=trie.as_callable())                  # a callable keeps the host loop
    assert len(eng.calls) == n and host.shape[0] == 1
    tr = {}
    assert beam(constraint=trie, trace=tr).tolist() == host.tolist() and "margin" in tr and len(eng.calls) == n     # a trace: host, no warning
    assert beam(constraint=trie, no_repeat_ngram_size=3).tolist() == host.tolist() and len(eng.calls) == n
    L.LlamaEngine._warned_beam_constraint = False
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        beam(constraint=trie, repetition_penalty=1.2, device_beam_sampler=True)
        beam(constraint=trie, repetition_penalty=1.2, device_beam_sampler=True)
        beam(constraint=trie, trace={})
    assert sum("constraint" in str(m.message) for m in w) == 1 and len(w) == 1 and len(eng.calls) == n       # one warning, host loop
    # one beam
    with pytest.raises(_Spy):
        one(do_sample=False, device_sampler=True, constraint=trie)          # constrained greedy on the device
    assert eng.calls[-1] == ("sample", trie)
    with pytest.raises(_Spy):
        one(do_sample=True, device_sampler=True, constraint=trie)
    assert eng.calls[-1] == ("sample", trie)
    n = len(eng.calls)
    a = one(do_sample=False, device_sampler=False, constraint=trie)
    b = one(do_sample=False, device_sampler=True, constraint=trie.as_callable())
    assert a.tolist() == b.tolist() and len(eng.calls) == n


def test_constraint_is_checked_before_any_device_work(monkeypatch):
    L, eng, x, mask = _engine(monkeypatch)
    eng.prefill = lambda *a, **k: pytest.fail("device work before the check")
    trie = TokenTrie(cc.LIB_SEQS, EOS, 64)
    for kw, what in ((dict(min_len=2), "min_len"), (dict(num_return_sequences=6), "num_return_sequences"), (dict(eos_id=3), "EOS")):
        with pytest.raises(ValueError, match=what):
            L.LlamaEngine.beam_search_generate(eng, x, mask, 8, 6, **{**dict(min_len=1, eos_id=EOS), **kw}, constraint=trie)
        with pytest.raises(ValueError, match=what):
            L.LlamaEngine.sample_generate(eng, x, mask, 6, **{**dict(min_len=1, eos_id=EOS, do_sample=True), **kw}, constraint=trie)
    with pytest.raises(ValueError, match="vocabulary"):
        L.LlamaEngine.beam_search_generate(eng, x, mask, 3, 6, eos_id=EOS, constraint=TokenTrie([[5]], EOS, 65))
    with pytest.raises(TypeError):
        L.LlamaEngine.beam_search_generate(eng, x, mask, 3, 6, eos_id=EOS, constraint=[[5]])


class _LM:
    def __init__(self):
        self.calls = []

    def _rec(name):
        def f(self, x, mask, *a, **kw):
            self.calls.append((name, kw.get("constraint", "absent"), kw.get("device_sampler")))
            return torch.zeros(x.shape[0], 1, dtype=torch.long)
        return f
    greedy_generate, sample_generate, beam_search_generate, contrastive_generate = _rec("greedy"), _rec("sample"), _rec("beam"), _rec("contrastive")


def test_models_hand_the_constraint_to_the_right_loop():
    from emu_amd.emu import EmuModel
    from emu_amd.emu1 import Emu
    trie = TokenTrie(cc.LIB_SEQS, EOS, 64)
    fn = trie.as_callable()
    ids, mask = torch.ones(1, 5, dtype=torch.long), torch.ones(1, 5, dtype=torch.long)
    EmuModel._warned_431 = True

    class Tok:
        padding_side = "right"

        def __call__(self, text, **k):
            return types.SimpleNamespace(input_ids=ids, attention_mask=mask)

        def batch_decode(self, out, **k):
            return ["x"] * out.shape[0]

    for model in ("emu2", "emu1"):
        lm = _LM()
        if model == "emu2":
            me = types.SimpleNamespace(hf_semantics="5.x", n_query=4, v_query=4, use_graph=False, device_sampler=True, image_placeholder="[i]",
                                       video_placeholder="[v]", decoder=types.SimpleNamespace(lm=lm, tokenizer=Tok()),
                                       _prompt_embeds=lambda i, image, nq, tok, embeds=None: torch.zeros(i.numel(), 8))
            gen_ids = lambda **k: EmuModel.generate_ids(me, ids, mask, **{**dict(min_len=0), **k})
            me.generate_ids = lambda *a, **k: EmuModel.generate_ids(me, *a, **k)
            gen = lambda **k: EmuModel.generate(me, ["q"], **k)
        else:
            me = types.SimpleNamespace(hf_semantics="5.x", device_sampler=True, lm=lm, tokenizer=Tok(),
                                       _prompt_embeds=lambda i, image: torch.zeros(1, i.numel(), 8))
            gen_ids = lambda **k: Emu.generate_ids(me, ids, mask, **{**dict(num_beams=1), **k})
            me.generate_ids = lambda *a, **k: Emu.generate_ids(me, *a, **k)
            gen = lambda **k: Emu.generate(me, {"prompt": ["q"]}, **k)
        gen_ids(num_beams=1)
        gen_ids(num_beams=5)
        assert lm.calls == [("greedy", "absent", None), ("beam", "absent", None)]            # no constraint: the old calls, unchanged
        gen_ids(num_beams=1, constraint=trie)                                                   # one beam: sample_generate, not greedy_generate
        gen_ids(num_beams=5, constraint=trie)
        gen_ids(num_beams=1, do_sample=True, constraint=fn)
        assert lm.calls[2:] == [("sample", trie, True), ("beam", trie, None), ("sample", fn, True)]
        with pytest.raises(NotImplementedError, match="constraint"):
            gen_ids(num_beams=1, penalty_alpha=0.6, top_k=4, constraint=trie)
        gen(num_beams=5, prefix_allowed_tokens_fn=fn)                                           # generate pops both spellings
        gen(num_beams=5, constraint=trie)
        assert lm.calls[-2:] == [("beam", fn, None), ("beam", trie, None)]
        with pytest.raises(ValueError, match="either"):
            gen(constraint=trie, prefix_allowed_tokens_fn=fn)
        with pytest.raises(TypeError, match="unsupported generation options"):
            gen(prefix_allowed_tokens=fn)
