"""CPU: prompt-lookup speculation together with sampling or a repetition penalty, on the host side -- the specification
(``speculate.row_select`` / ``simulate_select``) against the one-token-at-a-time loop of ``emu_amd/sampling.py`` with the same
uniforms, the routing (``genroute.lookup_route(device_sampler=True)``) and the refusals of ``LlamaEngine.lookup_generate``."""
import types

import pytest
import torch

from emu_amd import genroute, sampling, speculate
from tests.test_speculate_host import _StubLM, _emu2

V, EOS = 50, 2
SAMPLED = dict(do_sample=True, temperature=0.7, top_k=5, top_p=0.9)
PENALISED = dict(do_sample=False, repetition_penalty=1.3)


def toy_logits(prefix, seed):
    """bf16 logits [V] that are a seeded, deterministic function of the WHOLE prefix of generated ids; EOS is lifted into reach."""
    h = seed
    for t in prefix:
        h = (h * 1000003 + int(t) + 1) % (2 ** 31 - 1)
    g = torch.Generator().manual_seed(h)
    x = torch.randn(V, generator=g) * 2.0
    x[EOS] += 1.0
    return x.to(torch.bfloat16)


def sequential(seed, params, uniforms, max_new, min_len):
    """The non-speculative loop: ``sampling.reference_*`` per token, uniform ``uniforms[j]`` for output index j."""
    out = []
    for j in range(max_new):
        lg = toy_logits(out, seed)[None]
        sup = EOS if j < min_len else None
        pen = params.get("repetition_penalty", 1.0)
        if params["do_sample"]:
            p = sampling.reference_probs(lg, [out], pen, sup, True, params.get("temperature"), params.get("top_k"), params.get("top_p"))
            tok = int(sampling.reference_draw(p, uniforms[j].reshape(1))[0])
        else:
            tok = int(sampling.reference_greedy(lg, [out], pen, sup)[0])
        out.append(tok)
        if tok == EOS:
            break
    return out


def draft_table(g, k, max_new, right, gen):
    """[max_new, k]: row s is right (g[s + i]) for its first right[s] entries and a random other id from there on."""
    d = torch.zeros(max_new, k, dtype=torch.int32)
    for s in range(max_new):
        for i in range(k):
            gid = g[s + i] if s + i < len(g) else -1
            if i < right[s] and gid >= 0:
                d[s, i] = gid
            else:
                w = int(torch.randint(0, V, (1,), generator=gen))
                d[s, i] = w if w != gid else (w + 1) % V
    return d


def predicted_steps(g, drafts):
    """The step count from the accepted run lengths: a step at index s emits 1 + (the draft's leading matches with g[s:])."""
    s, steps = 1, 0
    while s < len(g) and g[s - 1] != EOS:
        n = 0
        while n < drafts.shape[1] and s + n < len(g) and int(drafts[s, n]) == g[s + n]:
            n += 1
        s += min(n + 1, len(g) - s)
        steps += 1
    return steps


@pytest.mark.parametrize("min_len", [0, 3])
@pytest.mark.parametrize("params", [PENALISED, SAMPLED], ids=["greedy_pen1.3", "sample_t0.7_k5_p0.9"])
@pytest.mark.parametrize("k", [1, 4, 7])
def test_speculation_does_not_change_the_sample(k, params, min_len):
    max_new, n_eos, longest = 14, 0, 0
    gen = torch.Generator().manual_seed(77 + k)
    for seed in range(1, 7):
        uniforms = torch.rand(max_new, generator=gen)
        g = sequential(seed, params, uniforms, max_new, min_len)
        n_eos += g[-1] == EOS
        longest = max(longest, len(g))
        spec_params = dict(params, suppress_id=EOS, min_len=min_len)

        def rows(fed, step, out):
            assert len(out) == step and fed[0] == out[-1]
            lg = torch.stack([toy_logits(out + fed[1:1 + i], seed) for i in range(len(fed))])
            return speculate.row_select(lg, out, fed, step, spec_params, uniforms)

        tables = [[j] * max_new for j in range(k + 1)] + [torch.randint(0, k + 1, (max_new,), generator=gen).tolist()]
        for right in tables:
            drafts = draft_table(g, k, max_new, right, gen)
            got, steps = speculate.simulate_select(rows, g[0], [], k, 2, max_new, min_len, EOS, drafts=drafts)
            assert got == g, (seed, right, got, g)
            assert steps == predicted_steps(g, drafts), (seed, right, steps)
        got, _ = speculate.simulate_select(rows, g[0], [7, 8, 7], k, 2, max_new, min_len, EOS)       # the real lookup's drafts
        assert got == g
    assert n_eos >= 1 and longest >= 8, "an EOS in reach, and runs long enough for whole drafts to be accepted"


def test_row_select_reads_the_history_the_step_and_the_uniform():
    """Row i: penalty over out[:step] + cur[1:1 + i] (once per distinct id; the pad id 0 and ids outside [0, V) included /
    ignored), the suppress while step + i < min_len, uniforms[min(step + i, rows - 1)]."""
    g = torch.Generator().manual_seed(3)
    lg = (torch.randn(4, V, generator=g) * 2).to(torch.bfloat16)
    out, cur, step = [5, 6, 5, 99], [99, 6, 0, V + 3], 3                                  # out[3] is beyond `step`: not history
    u = torch.rand(5, generator=g)
    for params in (dict(PENALISED, suppress_id=EOS, min_len=5), dict(SAMPLED, repetition_penalty=1.2, suppress_id=EOS, min_len=5)):
        got = speculate.row_select(lg, out, cur, step, params, u)
        for i in range(4):
            hist = [out[:step] + cur[1:1 + i]]
            sup = EOS if step + i < 5 else None
            if params["do_sample"]:
                p = sampling.reference_probs(lg[i:i + 1], hist, 1.2, sup, True, 0.7, 5, 0.9)
                want = int(sampling.reference_draw(p, u[min(step + i, 4)].reshape(1))[0])
            else:
                want = int(sampling.reference_greedy(lg[i:i + 1], hist, 1.3, sup)[0])
            assert got[i] == want, (i, got, want)


# ------------------------------------------------------------------------------------------------ routing
def test_lookup_route_with_the_device_sampler():
    r = genroute.lookup_route
    assert r(3, 1, 1, do_sample=True, device_sampler=True).device is True
    assert r(3, 1, 1, repetition_penalty=1.2, device_sampler=True).device is True
    assert r(3, 1, 1, do_sample=True, top_k=5, repetition_penalty=1.2, device_sampler=True).device is True
    for kw, word in ((dict(num_beams=5), "beam search"), (dict(num_beams=3, do_sample=True), "beam search"),
                     (dict(penalty_alpha=0.6, top_k=4), "contrastive search"), (dict(ngram=2), "n-gram ban"),
                     (dict(do_sample=True, ngram=2), "n-gram ban"), (dict(constraint=object()), "constraint"),
                     (dict(do_sample=True, num_return_sequences=2), "num_return_sequences")):
        with pytest.raises(ValueError, match=word):
            r(3, 1, 1, device_sampler=True, **kw)
    for k in (-1, 8):
        with pytest.raises(ValueError, match="1..7"):
            r(k, 1, 1, do_sample=True, device_sampler=True)
    with pytest.raises(ValueError, match="batch_size = 1"):
        r(3, 2, 1, do_sample=True, device_sampler=True)
    with pytest.raises(ValueError, match="tensor parallelism"):
        r(3, 1, 2, do_sample=True, device_sampler=True)
    with pytest.raises(ValueError, match="sampling"):                                     # off: as before
        r(3, 1, 1, do_sample=True)
    with pytest.raises(ValueError, match="repetition penalty"):
        r(3, 1, 1, repetition_penalty=1.2, device_sampler=False)


def test_model_route_adds_the_selection_keywords_only_when_it_selects():
    flags = dict.fromkeys(genroute.MODEL_FLAGS, True)
    assert genroute.model_route(flags, 1, False, None, None, 1.0, 0, 1, None, prompt_lookup_num_tokens=3) == \
        ("lookup_generate", dict(num_tokens=3, max_ngram=2, use_graph=True))
    assert genroute.model_route(flags, 1, True, None, None, 1.2, 0, 1, None, prompt_lookup_num_tokens=3, max_matching_ngram_size=3) == \
        ("lookup_generate", dict(num_tokens=3, max_ngram=3, use_graph=True, do_sample=True, repetition_penalty=1.2))
    off = dict(flags, device_sampler=False)
    with pytest.raises(ValueError, match="sampling"):
        genroute.model_route(off, 1, True, None, None, 1.0, 0, 1, None, prompt_lookup_num_tokens=3)


def test_models_reach_lookup_generate_with_the_sampler_keywords():
    ids, mask = torch.tensor([[1, 4, 4, 9]]), torch.ones(1, 4, dtype=torch.int64)
    demo = dict(do_sample=True, temperature=0.7, top_p=0.9, prompt_lookup_num_tokens=3)
    lm = _StubLM()
    m = _emu2(lm)
    with pytest.raises(ValueError, match="sampling"):                                     # the flag off: today's refusal
        m.generate_ids(ids, mask, max_new_tokens=6, **demo)
    assert not lm.calls and not m.embeds
    m.device_sampler = True
    m.generate_ids(ids, mask, max_new_tokens=6, **demo)
    (name, a, k), = lm.calls
    assert name == "lookup_generate" and a[2] is ids and k["num_tokens"] == 3
    assert k["do_sample"] is True and k["temperature"] == 0.7 and k["top_p"] == 0.9 and k["top_k"] is None and k["repetition_penalty"] == 1.0
    lm.calls.clear()
    m.generate(["a"], num_beams=1, max_new_tokens=6, repetition_penalty=1.3, prompt_lookup_num_tokens=2)
    assert lm.calls[0][0] == "lookup_generate" and lm.calls[0][2]["do_sample"] is False and lm.calls[0][2]["repetition_penalty"] == 1.3
    lm.calls.clear()
    m.generate_ids(ids, mask, max_new_tokens=6, prompt_lookup_num_tokens=3)               # plain greedy: no new keyword
    assert set(lm.calls[0][2]) == {"num_tokens", "max_ngram", "use_graph", "min_len", "eos_id", "pad_id", "stop_on_eos"}
    with pytest.raises(ValueError, match="beam search"):
        m.generate_ids(ids, mask, max_new_tokens=6, num_beams=5, **demo)

    from emu_amd.emu1 import Emu
    lm1 = _StubLM()
    e = Emu.__new__(Emu)
    e.lm = lm1
    e._prompt_embeds = lambda ids, *a, **k: torch.zeros(*ids.shape, 8)
    with pytest.raises(ValueError, match="sampling"):
        e.generate_ids(ids, mask, num_beams=1, max_new_tokens=6, **demo)
    e.device_sampler = True
    e.generate_ids(ids, mask, num_beams=1, max_new_tokens=6, **demo)
    (name, a, k), = lm1.calls
    assert name == "lookup_generate" and k["do_sample"] is True and k["temperature"] == 0.7 and k["top_p"] == 0.9


# ------------------------------------------------------------------------------------------------ the engine's refusals
def test_engine_refuses_before_the_prefill():
    from emu_amd._lib import SAMPLE_MAX_VOCAB
    from emu_amd.llama import LlamaEngine
    e = LlamaEngine.__new__(LlamaEngine)
    e.ctx = types.SimpleNamespace(tp_size=1, check_p2p=lambda: None)
    e.cfg = types.SimpleNamespace(max_position_embeddings=64, hidden_size=8)
    e.vocab, e.device = 50, torch.device("cpu")
    e.prefill = lambda *a, **k: pytest.fail("device work")
    x, mask, ids = torch.zeros(1, 10, 8), torch.ones(1, 10, dtype=torch.long), torch.zeros(1, 10, dtype=torch.long)
    for bad in (torch.zeros(7), torch.zeros(8, 2), torch.zeros(1, 8)):
        with pytest.raises(ValueError, match="uniforms"):
            e.lookup_generate(x, mask, ids, 8, 3, do_sample=True, uniforms=bad)
    with pytest.raises(ValueError, match="trace"):
        e.lookup_generate(x, mask, ids, 8, 3, do_sample=True, use_graph=True, trace=[])
    with pytest.raises(ValueError, match="trace"):
        e.lookup_generate(x, mask, ids, 8, 3, use_graph=True, trace=[])
    with pytest.raises(ValueError, match="1..7"):
        e.lookup_generate(x, mask, ids, 8, 9, repetition_penalty=1.2)
    with pytest.raises(ValueError, match="batch_size = 1"):
        e.lookup_generate(torch.zeros(2, 10, 8), torch.ones(2, 10), torch.zeros(2, 10), 8, 3, do_sample=True)
    e.vocab = SAMPLE_MAX_VOCAB + 1
    for kw in (dict(do_sample=True), dict(repetition_penalty=1.2)):
        with pytest.raises(ValueError, match="vocabulary"):
            e.lookup_generate(x, mask, ids, 8, 3, **kw)
