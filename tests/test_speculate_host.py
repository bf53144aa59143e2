"""CPU: prompt-lookup speculative decoding on the host side -- the specification (emu_amd/speculate.py) against the installed
library's PromptLookupCandidateGenerator and on hand-written tables, the routing (genroute.lookup_route) enumerated, and the public
entry points on models made with ``__new__`` around a stub engine (as tests/generation_route_cases.py makes them)."""
import itertools
import os
import random
import types

import pytest
import torch

from emu_amd import genroute, speculate
from tests import generation_route_cases as gc


# ------------------------------------------------------------------------------------------------ lookup_draft
def _library_candidates(history, k, max_ngram):
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    gen = PromptLookupCandidateGenerator(eos_token_id=None, num_output_tokens=k, max_matching_ngram_size=max_ngram,
                                         max_length=len(history) + k + 8)
    ids = torch.tensor([history], dtype=torch.long)
    out, _ = gen.get_candidates(ids)
    return out[0, len(history):].tolist()


def test_lookup_draft_restates_the_library():
    """Seeded random low-entropy strings: L 2..60, vocabulary 2..5, k 1..7, max_ngram 1..3 -- every draft equals the ids the
    installed library appends."""
    rng = random.Random(20260)
    seen_hit = seen_miss = seen_cut = 0
    for _ in range(1500):
        L, V, k, n = rng.randint(2, 60), rng.randint(2, 5), rng.randint(1, 7), rng.randint(1, 3)
        h = [rng.randrange(V) for _ in range(L)]
        got = speculate.lookup_draft(h, k, n)
        assert got == _library_candidates(h, k, n), (h, k, n, got)
        seen_hit += bool(got); seen_miss += not got; seen_cut += 0 < len(got) < k
    assert seen_hit > 100 and seen_miss > 10 and seen_cut > 10, (seen_hit, seen_miss, seen_cut)


def test_lookup_draft_by_hand():
    d = speculate.lookup_draft
    assert d([1, 2, 3, 9, 1, 2], 3, 2) == [3, 9, 1]                  # the 2-gram (1, 2) at 0: what followed it
    assert d([1, 2, 3, 9, 1, 2], 7, 2) == [3, 9, 1, 2]               # cut at the end of the history
    assert d([5, 2, 7, 1, 2], 2, 2) == [7, 1]                        # no earlier (1, 2): the 1-gram (2,) at 1
    assert d([1, 2, 3], 4, 3) == []                                  # nothing repeats
    assert d([4, 4], 3, 2) == [4]                                    # L - 1 bounds n; the first 4 is followed by one id
    assert d([7], 3, 2) == [] and d([], 3, 2) == []
    assert d([1, 2, 8, 1, 2, 9, 1, 2], 1, 2) == [8]                  # the FIRST window, left to right


# ------------------------------------------------------------------------------------------------ accept
EOS = 2


@pytest.mark.parametrize("draft, n_draft, a, step, max_new, min_len, want", [
    ([7, 8, 9], 3, [5, 6, 6, 6], 1, 20, 1, (1, False)),              # no match: row 0's arg-max alone
    ([7, 8, 9], 3, [7, 8, 9, 4], 1, 20, 1, (4, False)),              # all match: k + 1 ids
    ([7, 8, 9], 3, [6, 8, 9, 4], 1, 20, 1, (1, False)),              # mismatch at j = 0 (later matches do not count)
    ([7, 8, 9], 3, [7, 6, 9, 4], 1, 20, 1, (2, False)),              # ... at j = 1
    ([7, 8, 9], 3, [7, 8, 6, 4], 1, 20, 1, (3, False)),              # ... at j = 2
    ([7, EOS, 9], 3, [7, EOS, 9, 4], 1, 20, 1, (2, True)),           # EOS inside the accepted run: cut behind it, finished
    ([7, 8, 9], 3, [EOS, 8, 9, 4], 1, 20, 1, (1, True)),             # row 0 itself
    ([7, 8, 9], 3, [7, 8, 9, EOS], 1, 20, 1, (4, True)),             # the bonus id
    ([7, EOS, 9], 3, [7, EOS, 9, 4], 1, 20, 3, (4, False)),          # an EOS at index 2 < min_len ends nothing
    ([7, 8, EOS], 3, [7, 8, EOS, 4], 1, 20, 3, (3, True)),           # at index 3 = min_len it does
    ([7, 8, 9], 3, [7, 8, 9, 4], 18, 20, 1, (2, True)),              # the max_new cut: two ids fit
    ([7, 8, 9], 3, [6, 8, 9, 4], 19, 20, 1, (1, True)),              # the last id
    ([7, 8, 9], 3, [7, 8, 9, 4], 16, 20, 1, (4, True)),              # exactly full
    ([7, 0, 0], 1, [7, 0, 0, 4], 1, 20, 1, (2, False)),              # n_draft < k: the padding id 0 is never accepted
    ([0, 0, 0], 0, [0, 0, 0, 0], 1, 20, 1, (1, False)),              # no draft at all
])
def test_accept_tables(draft, n_draft, a, step, max_new, min_len, want):
    assert speculate.accept(draft, n_draft, a, step, max_new, min_len, EOS) == want


def test_row_argmax_suppresses_eos_below_min_len_and_takes_the_lowest_index():
    x = torch.zeros(4, 6)
    x[:, EOS] = 5.0
    x[:, 4] = 3.0
    x[3, 1] = 5.0                                                         # a tie with EOS: the lower index
    assert speculate.row_argmax(x, 1, 3, EOS) == [4, 4, EOS, 1]           # rows at indices 1, 2 are below min_len = 3
    assert speculate.row_argmax(x, 0, 0, EOS) == [EOS, EOS, EOS, 1]
    # a draft that guesses EOS below min_len meets a suppressed arg-max and is rejected
    assert speculate.accept([EOS, 4, 4], 3, speculate.row_argmax(x, 1, 3, EOS), 1, 20, 3, EOS) == (1, False)


def test_simulate_counts_steps():
    """A fixed greedy continuation 3, 4, 3, 4, ...: with real lookup drafts every step after the pattern is seen emits k + 1."""
    seq = [3, 4] * 8

    def rows(fed, step):                                                  # the model: whatever is fed, position p emits seq[p]
        return [seq[step + i] for i in range(len(fed))]

    out, steps = speculate.simulate(rows, seq[0], [9, 9], 3, 2, 12, 1, EOS)
    assert out == seq[:12]
    assert steps < 11                                                     # 11 one-token steps without speculation
    wrong = torch.full((12, 3), 8)
    out, steps = speculate.simulate(rows, seq[0], [9, 9], 3, 2, 12, 1, EOS, drafts=wrong)
    assert out == seq[:12] and steps == 11
    right = torch.tensor([[seq[s + j] if s + j < 16 else 0 for j in range(3)] for s in range(12)])
    out, steps = speculate.simulate(rows, seq[0], [9, 9], 3, 2, 12, 1, EOS, drafts=right)
    assert out == seq[:12] and steps == 3                                 # 1 + 4 + 4 + 3


# ------------------------------------------------------------------------------------------------ routing
def test_lookup_route_refusals_and_the_device_case():
    r = genroute.lookup_route
    assert r(0, 3, 8, num_beams=5, do_sample=True).device is False        # off: nothing is decided, nothing refused
    for k in range(1, 8):
        assert r(k, 1, 1).device is True
    for kw, word in ((dict(num_beams=3), "beam search"), (dict(do_sample=True), "sampling"),
                     (dict(repetition_penalty=1.2), "repetition penalty"), (dict(ngram=2), "n-gram ban"),
                     (dict(constraint=object()), "constraint"), (dict(penalty_alpha=0.6, top_k=4), "contrastive search"),
                     (dict(num_return_sequences=2), "num_return_sequences")):
        with pytest.raises(ValueError, match=word):
            r(3, 1, 1, **kw)
    for k in (-1, 8, 100):
        with pytest.raises(ValueError, match="1..7"):
            r(k, 1, 1)
    with pytest.raises(ValueError, match="batch_size = 1"):
        r(3, 2, 1)
    with pytest.raises(ValueError, match="tensor parallelism"):
        r(3, 1, 2)


def test_k0_keeps_every_recorded_model_route(golden_dir):
    """With the option given as 0 every model-level case of the recorded grid ends where the table says (the table itself is
    checked with the option absent by tests/test_generation_routes.py)."""
    table = gc.load(os.path.join(golden_dir, "generation_routes.json"))
    flags = dict.fromkeys(genroute.MODEL_FLAGS, True)
    for beams, sample, pen, ngram, nret, cons, alpha in itertools.product((1, 3), (False, True), (1.0, 1.2), (0, 2), (1, 2), (None, "c"),
                                                                         (None, 0.6)):
        a = (flags, beams, sample, 4 if alpha else None, alpha, pen, ngram, nret, cons)
        try:
            want = genroute.model_route(*a)
        except NotImplementedError as e:
            with pytest.raises(NotImplementedError, match=str(e)[:20]):
                genroute.model_route(*a, prompt_lookup_num_tokens=0, max_matching_ngram_size=3)
            continue
        assert genroute.model_route(*a, prompt_lookup_num_tokens=0, max_matching_ngram_size=3) == want
    n = 0
    for c, i in zip(gc.all_cases(), table["index"]):
        if c["level"] == "model" and n < 400:
            assert gc.run_case(c) == table["outcomes"][i], gc.case_id(c)
            n += 1
    assert genroute.model_route(flags, 1, False, None, None, 1.0, 0, 1, None, prompt_lookup_num_tokens=3) == \
        ("lookup_generate", dict(num_tokens=3, max_ngram=2, use_graph=True))


# ------------------------------------------------------------------------------------------------ the public entry points
class _StubLM:
    """Records the engine call the model makes."""

    def __init__(self, tp=1):
        self.calls, self.ctx = [], types.SimpleNamespace(tp_size=tp)

    def __getattr__(self, name):
        def f(*a, **k):
            self.calls.append((name, a, k))
            return torch.tensor([[5, 6, 7]])
        return f


class _StubTokenizer:
    def __call__(self, text, **k):
        return types.SimpleNamespace(input_ids=torch.tensor([[1, 4, 4, 9]] * len(text)), attention_mask=torch.ones(len(text), 4, dtype=torch.long))

    def batch_decode(self, ids, **k):
        return ["/".join(map(str, row.tolist())) for row in ids]


def _emu2(lm):
    from emu_amd.emu import EmuModel
    m = EmuModel.__new__(EmuModel)
    m.n_query = m.v_query = 1
    m.decoder = types.SimpleNamespace(lm=lm, tokenizer=_StubTokenizer())
    m.image_placeholder = m.video_placeholder = ""
    m.embeds = []
    m._prompt_embeds = lambda ids, *a, **k: (m.embeds.append(1), torch.zeros(ids.numel(), 8))[1]
    m.hf_semantics, m.use_graph = "5.x", False
    return m


def test_generate_takes_the_option_and_reaches_lookup_generate():
    """EmuModel.generate(..., prompt_lookup_num_tokens=3) was a TypeError ("unsupported generation options") before the option
    existed; now it reaches LlamaEngine.lookup_generate with the prompt's ids."""
    lm = _StubLM()
    m = _emu2(lm)
    out = m.generate(["a"], num_beams=1, max_new_tokens=6, prompt_lookup_num_tokens=3)
    assert out == ["5/6/7"]
    (name, a, k), = lm.calls
    assert name == "lookup_generate" and k["num_tokens"] == 3 and k["max_ngram"] == 2 and k["use_graph"] is False
    assert a[2].tolist() == [[1, 4, 4, 9]] and a[3] == 6 and k["min_len"] == 0       # ("5.x": min_len - S, floored)
    lm.calls.clear()
    m.generate(["a"], num_beams=1, max_new_tokens=6, prompt_lookup_num_tokens=2, max_matching_ngram_size=3)
    assert lm.calls[0][2]["max_ngram"] == 3
    lm.calls.clear()
    m.generate(["a"], num_beams=1, max_new_tokens=6)                                  # the option unused: plain greedy, as before
    assert lm.calls[0][0] == "greedy_generate" and "num_tokens" not in lm.calls[0][2]
    lm.calls.clear()
    m.generate(["a"], num_beams=1, max_new_tokens=6, prompt_lookup_num_tokens=0)
    assert lm.calls[0][0] == "greedy_generate"


def test_refusals_come_before_any_device_work():
    lm = _StubLM()
    m = _emu2(lm)
    ids, mask = torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, 4, dtype=torch.int64)
    for kw, word in ((dict(num_beams=5), "beam search"), (dict(do_sample=True), "sampling"), (dict(repetition_penalty=1.3), "penalty"),
                     (dict(no_repeat_ngram_size=2), "n-gram ban"), (dict(penalty_alpha=0.6, top_k=4), "contrastive"),
                     (dict(constraint=lambda b, i: [1]), "constraint"), (dict(prompt_lookup_num_tokens=8), "1..7")):
        with pytest.raises(ValueError, match=word):
            m.generate_ids(ids, mask, max_new_tokens=6, **{"prompt_lookup_num_tokens": 3, **kw})
    with pytest.raises(ValueError, match="batch_size = 1"):
        m.generate_ids(torch.zeros(2, 4, dtype=torch.int64), torch.ones(2, 4, dtype=torch.int64), max_new_tokens=6, prompt_lookup_num_tokens=3)
    m2 = _emu2(_StubLM(tp=2))
    with pytest.raises(ValueError, match="tensor parallelism"):
        m2.generate_ids(ids, mask, max_new_tokens=6, prompt_lookup_num_tokens=3)
    assert not lm.calls and not m.embeds and not m2.embeds


def test_emu1_takes_the_option():
    from emu_amd.emu1 import Emu
    lm = _StubLM()
    m = Emu.__new__(Emu)
    m.lm = lm
    m._prompt_embeds = lambda ids, *a, **k: torch.zeros(*ids.shape, 8)
    ids, mask = torch.tensor([[1, 4, 4, 9]]), torch.ones(1, 4, dtype=torch.int64)
    m.generate_ids(ids, mask, num_beams=1, max_new_tokens=6, prompt_lookup_num_tokens=4)
    (name, a, k), = lm.calls
    assert name == "lookup_generate" and k["num_tokens"] == 4 and a[2] is ids
    with pytest.raises(ValueError, match="beam search"):
        m.generate_ids(ids, mask, max_new_tokens=6, prompt_lookup_num_tokens=4)        # Emu's default is 5 beams


def test_engine_refuses_before_the_prefill():
    """LlamaEngine.lookup_generate on an engine made with ``__new__``: every refusal is raised before ``prefill`` is reached."""
    from emu_amd.llama import LlamaEngine
    e = LlamaEngine.__new__(LlamaEngine)
    e.ctx = types.SimpleNamespace(tp_size=1, check_p2p=lambda: None)
    e.cfg = types.SimpleNamespace(max_position_embeddings=64, hidden_size=8)
    e.vocab, e.device = 50, torch.device("cpu")
    e.prefill = lambda *a, **k: pytest.fail("device work")
    x, mask, ids = torch.zeros(1, 10, 8), torch.ones(1, 10, dtype=torch.long), torch.zeros(1, 10, dtype=torch.long)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        e.lookup_generate(x, mask, ids, 50, 5)                                        # 10 + 50 + 5 > 64
    with pytest.raises(ValueError, match="1..7"):
        e.lookup_generate(x, mask, ids, 8, 9)
    with pytest.raises(ValueError, match="batch_size = 1"):
        e.lookup_generate(torch.zeros(2, 10, 8), torch.ones(2, 10), torch.zeros(2, 10), 8, 3)
    with pytest.raises(ValueError, match="drafts"):
        e.lookup_generate(x, mask, ids, 8, 3, drafts=torch.zeros(8, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="prompt_ids"):
        e.lookup_generate(x, mask, ids[:, :5], 8, 3)
    e.decode_fused = 1
    with pytest.raises(ValueError, match="fused decode"):
        e.lookup_generate(x, mask, ids, 8, 3)
