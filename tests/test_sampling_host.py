"""CPU: the device sampler's specification (emu_amd/sampling.py) against the library-pinned host pipeline
(emu_amd.llama.process_logits), its tie rule, its draw, and the refusals / routing of the ``device_sampler`` option."""
import types

import pytest
import torch

from emu_amd import sampling
from emu_amd.llama import LlamaEngine, process_logits
from tests import sampler_cases as sc

HOST_VOCABS = (97, 1000, 32274)


def _host_probs(x, o):
    """softmax(process_logits(...)) with the options of a sampler case; the history holds in-range ids only there (the host gather
    has no bounds check: transformers never sees an id outside the vocabulary)."""
    B, V = x.shape
    h = o.get("history")
    gen = torch.zeros(B, 0, dtype=torch.int64) if h is None else h.clamp(max=V - 1)
    sup = o.get("suppress_id")
    s = process_logits(x.float(), gen, sup is not None, -1 if sup is None else sup, True, o.get("temperature"), o.get("top_k"),
                       o.get("top_p"), o.get("repetition_penalty", 1.0), o.get("min_keep", 1))
    return torch.softmax(s, dim=-1)


@pytest.mark.parametrize("V", HOST_VOCABS)
@pytest.mark.parametrize("name", list(sc.CASES))
def test_spec_equals_host_pipeline(V, name):
    """Same kept set, probabilities within 1e-6, on seeds whose top-p threshold group has one member (asserted by ``sc.case``)."""
    x, o = sc.case(V, name)
    if "history" in o:                                      # an id >= V is ignored by the spec and cannot be given to the host path
        o = dict(o, history=o["history"].clamp(max=V - 1))
        assert sc.check_screen(x, o)
    got = sampling.reference_probs(x, **o)
    want = _host_probs(x, o)
    assert torch.equal(got > 0, want > 0)
    assert float((got - want).abs().max()) <= 1e-6
    g64 = sampling.reference_probs(x, dtype=torch.float64, **o)
    assert torch.equal(g64 > 0, got > 0) and float((g64 - got.double()).abs().max()) <= 1e-6
    assert float((g64.sum(-1) - 1).abs().max()) < 1e-12


def test_history_ids_outside_the_vocabulary_are_ignored_and_duplicates_count_once():
    V = 97
    x = sc.rows(V, 11)
    h = sc.history(V)
    a = sampling.reference_scores(x, h, 1.3)
    dedup = [sorted({i for i in r if i < V}) for r in h.tolist()]
    b = sampling.reference_scores(x, dedup, 1.3)
    assert torch.equal(a, b)
    assert torch.equal(a[2], x[2].float())                  # row 2's history holds only ids >= V
    xf = x.float()
    assert a[0, 5] == (xf[0, 5] * torch.tensor(1.3) if xf[0, 5] < 0 else xf[0, 5] / torch.tensor(1.3))     # once, not three times


def test_tie_at_the_top_p_threshold_keeps_the_whole_group():
    """Constructed: probabilities (0.5, 0.2, 0.1, 0.1, 0.1) with top_p = 0.85 put the bound 0.15 inside the group of three equal
    scores.  The library's sort removes one member of the group (whichever it placed first); the spec keeps all three.  The spec's
    set is a superset, and the two differ only inside the tied group."""
    p = torch.tensor([[0.1, 0.5, 0.1, 0.2, 0.1]])
    x = p.log().to(torch.bfloat16)
    assert int((x[0] == x[0, 0]).sum()) == 3
    kept_spec = sampling.reference_probs(x, top_p=0.85) > 0
    kept_host = _host_probs(x, dict(top_p=0.85)) > 0
    tied = x[0] == x[0, 0]
    assert kept_spec.all() and int(kept_host.sum()) == 4
    assert bool((kept_spec | ~kept_host).all())                                     # superset
    assert bool((tied | (kept_spec == kept_host))[0].all())                         # they differ only inside the group
    group, _ = sampling.top_p_threshold_group(x, top_p=0.85)
    assert int(group[0]) == 3


def test_reference_draw():
    x, o = sc.case(1000, "both")
    q = sampling.reference_probs(x, dtype=torch.float64, **o)
    lo, hi = sampling.reference_intervals(q)
    pos = torch.arange(q.shape[1])
    for r in range(q.shape[0]):
        kept = pos[q[r] > 0]
        for t in kept.tolist():                             # u inside a token's interval returns that token
            mid = (lo[r, t] + hi[r, t]) / 2
            assert int(sampling.reference_draw(q[r:r + 1], mid[None])) == t
        assert int(sampling.reference_draw(q[r:r + 1], torch.zeros(1, dtype=torch.float64))) == int(kept[0])
        assert int(sampling.reference_draw(q[r:r + 1], torch.tensor([1 - 2.0 ** -24], dtype=torch.float64))) in kept.tolist()
        assert int(sampling.reference_draw(q[r:r + 1], torch.tensor([1.0], dtype=torch.float64))) == int(kept[-1])
    q32 = sampling.reference_probs(x, **o)
    assert int(sampling.reference_draw(q32[:1], torch.tensor([1 - 2.0 ** -24]))) in pos[q32[0] > 0].tolist()


def test_greedy_is_the_first_index_of_the_maximum():
    x = torch.tensor([[1.0, 3.0, 3.0, -2.0], [0.5, 0.5, 0.25, 0.5]]).to(torch.bfloat16)
    assert sampling.reference_greedy(x).tolist() == [1, 0]
    assert sampling.reference_greedy(x, suppress_id=1).tolist() == [2, 0]
    assert sampling.reference_greedy(x, [[1, 2, 2], [0, 1, 3]], 4.0).tolist() == [0, 2]
    assert sampling.reference_probs(x, do_sample=False).tolist() == [[0, 1, 0, 0], [1, 0, 0, 0]]


# ------------------------------------------------------------------------------------------------ refusals and routing
def _stand_in_engine(tp_size=1, vocab=1000):
    """A LlamaEngine without a library: every refusal has to come before the first library call, which would fail on it."""
    e = LlamaEngine.__new__(LlamaEngine)
    e.ctx = types.SimpleNamespace(tp_size=tp_size)
    e.vocab = vocab
    return e


def test_refusals_come_before_any_library_call():
    x, mask = torch.zeros(1, 4, 8, dtype=torch.bfloat16), torch.ones(1, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        _stand_in_engine().sample_generate(x, mask, 4, device_sampler=True, no_repeat_ngram_size=2)
    with pytest.raises(ValueError, match="tensor parallelism"):
        _stand_in_engine(tp_size=2).sample_generate(x, mask, 4, device_sampler=True)
    with pytest.raises(AttributeError):                     # without the option the stand-in gets as far as its missing engine
        _stand_in_engine(tp_size=2).sample_generate(x, mask, 4)


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a, **k):
            self.calls.append((name, k))
            return torch.zeros(1, 1, dtype=torch.int64)
        return f


def _stand_in_model(model_cls, **attrs):
    m = model_cls.__new__(model_cls)
    rec = _Recorder()
    m.device_sampler, m.use_graph, m.hf_semantics = True, True, "5.x"
    m.n_query = m.v_query = 1
    for k, v in attrs.items():
        setattr(m, k, v)
    return m, rec


def test_generate_ids_routes_only_the_one_beam_sampling_branch_to_the_device_sampler():
    from emu_amd.emu import EmuModel
    m, rec = _stand_in_model(EmuModel)
    m.decoder = types.SimpleNamespace(lm=rec)
    m._prompt_embeds = lambda ids, *a, **k: torch.zeros(ids.shape[0] * ids.shape[1], 8)
    ids, mask = torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, 4, dtype=torch.int64)
    m.generate_ids(ids, mask, do_sample=True, top_p=0.9)
    m.generate_ids(ids, mask, repetition_penalty=1.5)
    m.generate_ids(ids, mask, do_sample=True, no_repeat_ngram_size=2)               # the n-gram ban keeps the host loop
    m.generate_ids(ids, mask, do_sample=True, num_beams=3)                          # beam sampling: its old path
    m.generate_ids(ids, mask, penalty_alpha=0.6, top_k=4)                           # contrastive search: its old path
    m.generate_ids(ids, mask)                                                       # plain greedy
    names = [c[0] for c in rec.calls]
    assert names == ["sample_generate", "sample_generate", "sample_generate", "beam_search_generate", "contrastive_generate",
                     "greedy_generate"]
    assert [c[1]["device_sampler"] for c in rec.calls[:3]] == [True, True, False]
    assert all(c[1]["use_graph"] is True for c in rec.calls[:3])
    assert all("device_sampler" not in c[1] for c in rec.calls[3:])
    m.device_sampler = False
    m.generate_ids(ids, mask, do_sample=True)
    assert rec.calls[-1][1]["device_sampler"] is False


def test_emu1_generate_ids_passes_the_option():
    from emu_amd.emu1 import Emu
    m, rec = _stand_in_model(Emu)
    rec.embed_tokens = lambda ids: torch.zeros(*ids.shape, 8)
    m.lm = rec
    ids, mask = torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, 4, dtype=torch.int64)
    m.generate_ids(ids, mask, num_beams=1, do_sample=True, top_p=0.9)
    m.generate_ids(ids, mask, num_beams=3, do_sample=True)
    assert rec.calls[0][0] == "sample_generate" and rec.calls[0][1]["device_sampler"] is True
    assert rec.calls[1][0] == "beam_search_generate" and "device_sampler" not in rec.calls[1][1]


def test_bound_constant_matches_the_header():
    import re
    from emu_amd import _lib
    txt = open(_lib.HEADER_PATH).read()
    assert int(re.search(r"#define EMU_SAMPLE_MAX_VOCAB (\d+)", txt).group(1)) == _lib.SAMPLE_MAX_VOCAB >= 40000
    for cite in ("emu.py:213-229", "chat.py:86-148"):
        assert cite in txt
