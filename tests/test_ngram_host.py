"""CPU: the no-repeat n-gram ban of the device token loops -- its specification (``sampling.banned_ngram_mask`` and the ``banned``
argument of the ``reference_*`` / ``beam_reference_*`` functions) against the installed library's NoRepeatNGramLogitsProcessor and the
host pipeline, and the routing of the opt-in ``device_ngram_ban`` through the engine and the model classes."""
import types
import warnings

import pytest
import torch

from emu_amd import _lib, sampling
from emu_amd.constrain import TokenTrie
from emu_amd.llama import LlamaEngine, ban_repeated_ngrams, process_logits
from tests import ngram_cases as nc

EOS, PAD = nc.EOS, nc.PAD
NS, CURS, V = (1, 2, 3, 4), (0, 1, 2, 3, 7, 15, 40), 40


# ------------------------------------------------------------------------------------------------ the mask
def test_mask_equals_the_librarys_processor_and_the_host_form():
    from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor
    g = torch.Generator().manual_seed(8)
    fired = 0
    for n in NS:
        for cur in CURS:
            gen = nc.alphabet_history(4, cur, g)
            scores = torch.randn(4, V, generator=g)
            mask = sampling.banned_ngram_mask(gen, n, V)
            assert mask.shape == (4, V) and mask.dtype == torch.bool
            assert torch.equal(mask, torch.isinf(NoRepeatNGramLogitsProcessor(n)(gen, scores.clone()))), (n, cur)
            assert torch.equal(mask, torch.isinf(ban_repeated_ngrams(scores.clone(), gen, n))), (n, cur)
            assert torch.equal(mask, sampling.banned_ngram_mask(gen.tolist(), n, V)), (n, cur)       # a list of rows: the same
            assert bool(mask.any()) == (cur >= n and bool(mask.any()))           # nothing is banned before a repetition fits
            fired += int(mask.any())
    assert fired > 10
    for n in (0, -1):                                                            # n < 1 means off
        assert not bool(sampling.banned_ngram_mask(nc.alphabet_history(2, 7, g), n, V).any())


def test_mask_by_hand_and_an_id_outside_the_vocabulary():
    m = sampling.banned_ngram_mask([[5, 6, 7, 5, 6]], 3, 10)                     # the last two ids (5, 6) were followed by 7
    assert m.nonzero().tolist() == [[0, 7]]
    m = sampling.banned_ngram_mask([[5, 6, 5, 7, 5]], 2, 10)                     # 5 was followed by 6 and by 7
    assert m.nonzero().tolist() == [[0, 6], [0, 7]]
    assert sampling.banned_ngram_mask([[4, 4]], 1, 10).nonzero().tolist() == [[0, 4]]
    assert not bool(sampling.banned_ngram_mask([[5, 6]], 3, 10).any())           # nh + 1 = n, but no start position yet
    # PAD 32000 as the would-be banned id: ignored, nothing raised; a real id next to it still counts
    m = sampling.banned_ngram_mask([[5, PAD, 5, 6, 5], [PAD, PAD, PAD, PAD, PAD]], 2, V)
    assert m.nonzero().tolist() == [[0, 6]]
    assert sampling.banned_ngram_mask(torch.zeros(3, 0, dtype=torch.int64), 2, V).shape == (3, V)


# ------------------------------------------------------------------------------------------------ the spec functions
def test_reference_scores_equal_the_host_pipeline():
    g = torch.Generator().manual_seed(3)
    for n in NS:
        for cur in (0, 3, 7, 15):
            gen = nc.alphabet_history(3, cur, g)
            x = torch.randn(3, V, generator=g).to(torch.bfloat16)
            mask = sampling.banned_ngram_mask(gen, n, V)
            want = process_logits(x.float(), gen, True, EOS, False, repetition_penalty=1.4, no_repeat_ngram_size=n)
            got = sampling.reference_scores(x, gen, 1.4, EOS, banned=mask)
            assert torch.equal(got, want), (n, cur)
            assert sampling.reference_greedy(x, gen, 1.4, EOS, banned=mask).tolist() == want.argmax(dim=-1).tolist()
            q = sampling.reference_probs(x, gen, 1.4, EOS, top_k=5, banned=mask)
            assert not bool((q > 0)[mask].any()) and not bool((q[:, EOS] > 0).any())
            s, kept = sampling.reference_warped(x, gen, 1.4, EOS, temperature=0.7, top_k=5, banned=mask)
            assert not bool(kept[mask].any())


def test_beam_reference_rows_equal_the_host_loops_processing():
    g = torch.Generator().manual_seed(4)
    for n in NS:
        for cur in (0, 3, 7, 15):
            gen = nc.alphabet_history(6, cur, g)
            x = (torch.randn(6, V, generator=g) * 3).to(torch.bfloat16)
            rs = torch.randn(6, generator=g)
            mask = sampling.banned_ngram_mask(gen, n, V)
            for pen in (1.0, 1.2):
                want = process_logits(torch.log_softmax(x.float(), dim=-1), gen, cur < 5, EOS, False, repetition_penalty=pen, min_keep=2,
                                      no_repeat_ngram_size=n) + rs[:, None]
                got = sampling.beam_reference_rows(x, rs, gen, pen, EOS, cur < 5, do_sample=False, banned=mask)
                assert torch.equal(torch.isinf(got), torch.isinf(want)), (n, cur, pen)
                fin = ~torch.isinf(want)
                assert float((got[fin] - want[fin]).abs().max()) < 1e-5, (n, cur, pen)       # (two forms of the log-sum-exp)
            acc = sampling.beam_reference_rows(x, rs, gen, 1.2, EOS, False, temperature=0.7, top_k=3, top_p=0.9, banned=mask)
            assert not bool((acc > -float("inf"))[mask].any())
            w = sampling.beam_reference_warp_input(x, rs, gen, 1.2, EOS, False, "4.31", banned=mask)
            assert bool(torch.isinf(w[mask]).all())


def test_beam_scenarios_bite():
    """The scenarios the kernel tests replay (tests/ngram_cases.py): from step n on some beam row has a non-empty banned set, and the
    kept sequences differ from the same logits' search without the ban."""
    for B, nb, V_, L in nc.BEAM_SHAPES:
        for n in (1, 2, 3):
            for v431 in (False, True):
                steps = nc.beam_scenario(B, nb, V_, L, n, v431)
                assert all(s["banned_rows"] > 0 for s in steps[n:]), (B, nb, V_, n, [s["banned_rows"] for s in steps])
                free = nc.beam_scenario(B, nb, V_, L, 0, v431)
                assert steps[-1]["state"]["sequences"].tolist() != free[-1]["state"]["sequences"].tolist()
                for row in steps[-1]["state"]["sequences"].view(-1, L).tolist():
                    assert not nc.has_repeated_ngram(row, n), row


# ------------------------------------------------------------------------------------------------ routing and refusals
def _stand_in_engine(tp_size=1, vocab=1000):
    """A LlamaEngine without a library: every refusal has to come before the first library call, which would fail on it."""
    e = LlamaEngine.__new__(LlamaEngine)
    e.ctx = types.SimpleNamespace(tp_size=tp_size)
    e.vocab = vocab
    return e


X, MASK = torch.zeros(1, 4, 8, dtype=torch.bfloat16), torch.ones(1, 4, dtype=torch.int64)


def test_flag_off_the_refusals_still_come():
    for flag in ({}, dict(device_ngram_ban=False)):
        with pytest.raises(ValueError, match="device_sampler: no_repeat_ngram_size > 0 is not built on the device"):
            _stand_in_engine().sample_generate(X, MASK, 4, device_sampler=True, no_repeat_ngram_size=2, **flag)
        with pytest.raises(ValueError, match="device_beam_sampler: no_repeat_ngram_size > 0 is not built on the device"):
            _stand_in_engine().beam_search_generate(X, MASK, 3, 6, do_sample=True, device_beam_sampler=True, no_repeat_ngram_size=2, **flag)


def test_flag_on_the_call_gets_past_the_refusal():
    with pytest.raises(AttributeError):                     # the stand-in gets as far as its missing engine
        _stand_in_engine().sample_generate(X, MASK, 4, device_sampler=True, no_repeat_ngram_size=2, device_ngram_ban=True)
    with pytest.raises(AttributeError):
        _stand_in_engine().beam_search_generate(X, MASK, 3, 6, do_sample=True, device_beam_sampler=True, no_repeat_ngram_size=2,
                                                device_ngram_ban=True)
    with pytest.raises(AttributeError):                     # the flag without device_sampler: no effect, the host loop's prefill
        _stand_in_engine().sample_generate(X, MASK, 4, no_repeat_ngram_size=2, device_ngram_ban=True)
    with pytest.raises(ValueError, match="tensor parallelism"):     # the sampler branches keep their tensor-parallelism refusal
        _stand_in_engine(tp_size=2).beam_search_generate(X, MASK, 3, 6, do_sample=True, device_beam_sampler=True, no_repeat_ngram_size=2,
                                                         device_ngram_ban=True)
    with pytest.raises(ValueError, match="tensor parallelism"):
        _stand_in_engine(tp_size=2).sample_generate(X, MASK, 4, device_sampler=True, no_repeat_ngram_size=2, device_ngram_ban=True)
    with pytest.raises(AttributeError):                     # the deterministic branch is not refused under tensor parallelism
        _stand_in_engine(tp_size=2).beam_search_generate(X, MASK, 3, 6, no_repeat_ngram_size=2, device_ngram_ban=True)


def _one_warning(monkeypatch, call, why):
    monkeypatch.setattr(LlamaEngine, "_warned_ngram_ban", False)
    with pytest.warns(UserWarning, match=why):
        with pytest.raises(AttributeError):                 # ... then the host path, as far as the prefill the stand-in lacks
            call()
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # once per process
        with pytest.raises(AttributeError):
            call()


def test_outside_the_kernels_range_the_host_loop_takes_over_with_one_warning(monkeypatch):
    trie = TokenTrie([[5, 6]], EOS, 1000)
    ban = dict(no_repeat_ngram_size=2, device_ngram_ban=True)
    _one_warning(monkeypatch, lambda: _stand_in_engine().sample_generate(X, MASK, 4, min_len=0, device_sampler=True, constraint=trie, **ban),
                 "TokenTrie together with the ban")
    _one_warning(monkeypatch, lambda: _stand_in_engine(vocab=5).sample_generate(X, MASK, 4, device_sampler=True, **ban), "below max_new_tokens")
    beam = lambda e, **k: e.beam_search_generate(X, MASK, 3, 6, do_sample=True, device_beam_sampler=True, **ban, **k)
    _one_warning(monkeypatch, lambda: beam(_stand_in_engine(vocab=12)), "below max_new_tokens")          # 6 + 1 + 2 * 3 = 13
    _one_warning(monkeypatch, lambda: beam(_stand_in_engine(), trace={}), "trace")
    with warnings.catch_warnings():                          # vocab = 13 is inside the range: no warning of this kind
        warnings.simplefilter("error")
        monkeypatch.setattr(LlamaEngine, "_warned_ngram_ban", False)
        with pytest.raises(AttributeError):
            beam(_stand_in_engine(vocab=13))
        # the deterministic branch asked for nothing explicitly: it keeps the host loop without a word
        with pytest.raises(AttributeError):
            _stand_in_engine(vocab=12).beam_search_generate(X, MASK, 3, 6, **ban)


def test_engine_routes_the_ban_to_the_device_loops(monkeypatch):
    """On the CPU stand-in dressed as the device engine (tests/test_constrain_host.py's): where each call ends up, and with what n."""
    from tests.test_constrain_host import _Spy, _engine
    L, eng, x, mask = _engine(monkeypatch)
    seen = []
    eng._beam_search_device = lambda *a, **k: (seen.append(("beam", k.get("ngram", 0), k.get("sampler") is not None)), (_ for _ in ()).throw(_Spy()))[1]
    eng._sample_device = lambda *a, **k: (seen.append(("sample", k.get("ngram", 0), False)), (_ for _ in ()).throw(_Spy()))[1]
    beam = lambda **k: L.LlamaEngine.beam_search_generate(eng, x, mask, 3, 6, min_len=0, eos_id=EOS, pad_id=PAD, hf_semantics="5.x", **k)
    one = lambda **k: L.LlamaEngine.sample_generate(eng, x, mask, 6, min_len=0, eos_id=EOS, pad_id=PAD, **k)
    with pytest.raises(_Spy):
        beam(no_repeat_ngram_size=2, device_ngram_ban=True)
    with pytest.raises(_Spy):
        beam(no_repeat_ngram_size=3, device_ngram_ban=True, repetition_penalty=1.2, device_beam_sampler=True)
    with pytest.raises(_Spy):
        one(do_sample=False, device_sampler=True, no_repeat_ngram_size=2, device_ngram_ban=True)
    with pytest.raises(_Spy):
        beam()                                               # no ban: the call it made before, without the keyword
    assert seen == [("beam", 2, False), ("beam", 3, True), ("sample", 2, False), ("beam", 0, False)]
    n = len(seen)
    host = beam(no_repeat_ngram_size=2)                      # without the flag: the host loop, as before
    assert len(seen) == n and not any(nc.has_repeated_ngram(r, 2) for r in host.tolist())
    trie = TokenTrie([[10, 11], [20]], EOS, 64)
    beam(no_repeat_ngram_size=2, device_ngram_ban=True, constraint=trie)         # a constraint with the ban: the host loop
    beam(no_repeat_ngram_size=2, device_ngram_ban=True, trace={})                # a trace: the host loop
    one(do_sample=False, no_repeat_ngram_size=2, device_ngram_ban=True)          # the flag without device_sampler: no effect
    assert len(seen) == n


# ------------------------------------------------------------------------------------------------ the model classes
class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a, **k):
            self.calls.append((name, k))
            return torch.zeros(1, 1, dtype=torch.int64)
        return f


def _emu2(**attrs):
    from emu_amd.emu import EmuModel
    m, rec = EmuModel.__new__(EmuModel), _Recorder()
    m.device_sampler, m.use_graph, m.hf_semantics = False, True, "5.x"
    m.n_query = m.v_query = 1
    m.decoder = types.SimpleNamespace(lm=rec)
    m._prompt_embeds = lambda ids, *a, **k: torch.zeros(ids.shape[0] * ids.shape[1], 8)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m, rec


def _emu1(**attrs):
    from emu_amd.emu1 import Emu
    m, rec = Emu.__new__(Emu), _Recorder()
    m.device_sampler, m.hf_semantics = False, "5.x"
    rec.embed_tokens = lambda ids: torch.zeros(*ids.shape, 8)
    m.lm = rec
    for k, v in attrs.items():
        setattr(m, k, v)
    return m, rec


@pytest.mark.parametrize("make", [_emu2, _emu1])
def test_models_pass_the_keyword_only_with_the_option_and_a_ban(make):
    ids, mask = torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, 4, dtype=torch.int64)
    m, rec = make(device_sampler=True, device_beam_sampler=True, device_ngram_ban=True)
    m.generate_ids(ids, mask, do_sample=True, num_beams=1, no_repeat_ngram_size=2)
    m.generate_ids(ids, mask, do_sample=True, num_beams=3, no_repeat_ngram_size=2)
    m.generate_ids(ids, mask, num_beams=3, no_repeat_ngram_size=2)               # deterministic beams: the same keywords, the engine picks
    m.generate_ids(ids, mask, do_sample=True, num_beams=1)                       # no ban: the calls of before
    m.generate_ids(ids, mask, do_sample=True, num_beams=3)
    kw = [c[1] for c in rec.calls]
    assert [c[0] for c in rec.calls] == ["sample_generate", "beam_search_generate", "beam_search_generate", "sample_generate",
                                         "beam_search_generate"]
    assert [k.get("device_ngram_ban") for k in kw] == [True, True, True, None, None]
    assert kw[0]["device_sampler"] is True and kw[1]["device_beam_sampler"] is True and kw[2]["device_beam_sampler"] is True
    assert kw[3]["device_sampler"] is True and kw[4]["device_beam_sampler"] is True
    # the option off (false, or missing as on a model made with __new__): the samplers are dropped under a ban, and no keyword
    for attrs in (dict(), dict(device_ngram_ban=False)):
        m, rec = make(device_sampler=True, device_beam_sampler=True, **attrs)
        m.generate_ids(ids, mask, do_sample=True, num_beams=1, no_repeat_ngram_size=2)
        m.generate_ids(ids, mask, do_sample=True, num_beams=3, no_repeat_ngram_size=2)
        assert all("device_ngram_ban" not in c[1] for c in rec.calls), attrs
        assert rec.calls[0][1]["device_sampler"] is False and "device_beam_sampler" not in rec.calls[1][1], attrs
    # the option alone switches no sampler on
    m, rec = make(device_ngram_ban=True)
    m.generate_ids(ids, mask, do_sample=True, num_beams=1, no_repeat_ngram_size=2)
    m.generate_ids(ids, mask, do_sample=True, num_beams=3, no_repeat_ngram_size=2)
    assert rec.calls[0][1]["device_sampler"] is False and "device_beam_sampler" not in rec.calls[1][1]
    assert all(c[1]["device_ngram_ban"] is True for c in rec.calls)


def test_the_environment_variable_is_the_default(monkeypatch):
    import emu_amd.vit as vit
    from emu_amd import emu, emu1
    from emu_amd.conf.emu_conf import LlamaCfg
    for mod in (emu, emu1):
        monkeypatch.setattr(mod, "EmuHipContext", lambda *a, **k: types.SimpleNamespace())
        monkeypatch.setattr(mod, "LlamaEngine", lambda *a, **k: _Recorder())
    monkeypatch.setattr(vit, "VitEngine", lambda *a, **k: None)
    monkeypatch.setattr(emu1, "VitEngine", lambda *a, **k: None)
    monkeypatch.setattr(emu1, "CausalFormer", lambda *a, **k: None)
    for make in (lambda **k: emu.EmuModel(llama_cfg=LlamaCfg(), device="cpu", **k), lambda **k: emu1.Emu(device="cpu", **k)):
        monkeypatch.delenv("EMU_DEVICE_NGRAM_BAN", raising=False)
        assert make().device_ngram_ban is False and make(device_ngram_ban=True).device_ngram_ban is True
        assert make(device_sampler=True, device_beam_sampler=True).device_ngram_ban is False
        for value, want in (("1", True), ("0", False), ("true", False)):
            monkeypatch.setenv("EMU_DEVICE_NGRAM_BAN", value)
            assert make().device_ngram_ban is want, value
        monkeypatch.setenv("EMU_DEVICE_NGRAM_BAN", "1")
        m = make(device_ngram_ban=False)
        assert m.device_ngram_ban is False and make().device_sampler is False and make().device_beam_sampler is False


# ------------------------------------------------------------------------------------------------ the ABI
NEW_SYMBOLS = ("emu_sample_ngram_bf16", "emu_llama_sample_step_ngram", "emu_beam_step_ngram_bf16", "emu_beam_sample_step_ngram_bf16")


def test_the_header_declares_the_four_entry_points():
    declared = _lib.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib._PROTOS, name
    txt = open(_lib.HEADER_PATH).read()
    assert txt.count("modeling_emu.py:115,177") >= 4
    # each is its parent with one more int ahead of the stream
    for name, parent in zip(NEW_SYMBOLS, ("emu_sample_bf16", "emu_llama_sample_step", "emu_beam_step_bf16", "emu_beam_sample_step_bf16")):
        res, args = _lib._PROTOS[name]
        pres, pargs = _lib._PROTOS[parent]
        assert res is pres and args == pargs[:-1] + [_lib.i32, pargs[-1]], name
