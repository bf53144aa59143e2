"""CPU tests of beam-search sampling on the device, the parts that need no device: the specification (emu_amd/sampling.py:
beam_reference_rows / beam_reference_probs / beam_reference_select) against the host pipeline of ``beam_search_generate``, the draw
rule on rows where every interval is known, the host loop drawing from a table of uniforms, and the routing of the new option."""
import os
import types

import numpy as np
import pytest
import torch

from emu_amd import sampling
from emu_amd.llama import LlamaEngine, beam_host_scores, process_logits
from tests import beam_sampler_cases as bc

NEG_INF = -float("inf")


# ------------------------------------------------------------------------------------------------ 1. spec against the host pipeline
def host_acc(x, rs, o, order, B, nb):
    """The accumulated scores of ``beam_search_generate``'s host step, [B, nb, V]: ``llama.beam_host_scores`` (log_softmax ->
    process_logits(min_keep=2) / warp_logits in the order's sequence), row by row.  The pipeline gathers by history id, so every row
    gets its in-range ids only."""
    V = x.shape[1]
    hist = o.get("history")
    out = []
    for r in range(B * nb):
        ids = [i for i in (hist[r].tolist() if hist is not None else []) if 0 <= i < V]
        min_len = len(ids) + 1 if o["suppress_eos"] else 0                  # (the step suppresses EOS while cur < min_len)
        out.append(beam_host_scores(x[r].float().view(1, 1, V), rs.reshape(-1)[r].view(1, 1), torch.tensor([[ids]], dtype=torch.int64),
                                    len(ids), min_len, o["eos_id"], True, order == "4.31", o.get("temperature"), o.get("top_k"),
                                    o.get("top_p"), o.get("repetition_penalty", 1.0)))
    return torch.cat(out).view(B, nb, V)


def spec_acc(x, rs, o, order, dtype=torch.float32, do_sample=True):
    return sampling.beam_reference_rows(x, rs, o.get("history"), o.get("repetition_penalty", 1.0), o["eos_id"], o["suppress_eos"],
                                        do_sample, o.get("temperature"), o.get("top_k"), o.get("top_p"), order, dtype)


@pytest.mark.parametrize("order", bc.ORDERS)
@pytest.mark.parametrize("name", list(bc.CASES))
@pytest.mark.parametrize("B,nb,V", bc.CPU_SHAPES)
def test_spec_keeps_what_the_host_pipeline_keeps(B, nb, V, name, order):
    x, rs, o = bc.case(B, nb, V, name, order)
    acc = spec_acc(x, rs, o, order)
    p = sampling.beam_reference_probs(acc, nb)
    want = torch.softmax(host_acc(x, rs, o, order, B, nb).reshape(B, nb * V), dim=-1)
    assert torch.equal(p > 0, want > 0)
    assert float((p - want).abs().max()) <= 1e-5
    assert torch.equal((acc == NEG_INF).view(B, -1) | (p == 0), p == 0)             # removed entries have no mass
    # the fp64 yardstick keeps the same set
    assert torch.equal(spec_acc(x, rs, o, order, torch.float64) > NEG_INF, acc > NEG_INF)


def test_penalised_beam_search_rows_are_the_host_pipelines():
    B, nb, V = 2, 3, 1000
    x, rs, o = bc.case(B, nb, V, "t20pen", "5.x")
    acc = spec_acc(x, rs, o, "5.x", do_sample=False)
    lp = torch.log_softmax(x.float(), dim=-1)
    want = torch.cat([process_logits(lp[r:r + 1], torch.tensor([[i for i in o["history"][r].tolist() if 0 <= i < V]]), False, bc.EOS,
                                     False, repetition_penalty=1.3) for r in range(B * nb)]) + rs.reshape(-1, 1)
    assert float((acc - want).abs().max()) <= 1e-5
    top_lp, top_idx = sampling.beam_reference_select(acc, nb, None, do_sample=False)
    w_lp, w_idx = torch.topk(want.view(B, nb * V), 2 * nb)
    assert top_idx.tolist() == w_idx.tolist()


# ------------------------------------------------------------------------------------------------ 2. the draw rule
def _acc_of(masses):
    """acc [1, nb, V] whose softmax is ``masses`` (powers of two, so that every boundary is a binary fraction)."""
    return torch.tensor(masses, dtype=torch.float64).log().float()[None]


MASSES = [[0.125, 0.25, 0.0, 0.125], [0.25, 0.0, 0.25, 0.0]]        # boundaries 0.125, 0.375, 0.5, 0.75; flat ids 0 1 3 4 6


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_draw_rule_on_known_intervals(dtype):
    acc = _acc_of(MASSES)
    one = 1 - 2.0 ** -24
    draws = lambda u: sampling.beam_reference_select(acc, 2, torch.tensor([u], dtype=torch.float32), True, "5.x", dtype)[1][0].tolist()
    # u = 0: the lowest entry of positive mass; u = 1 - 2^-24: the highest remaining one, whatever u * R rounds to
    d = draws([0.0, one, 0.39, 0.41])
    assert d[:2] == [0, 6]
    # masses left: id 1 0.25, id 3 0.125, id 4 0.25 (R = 0.625, boundaries at 0.25 and 0.375 -> u = 0.4 and 0.6)
    assert d[2] == 1 and d[3] == 4                                      # 0.41 * 0.375 = 0.154 of (id 3 0.125, id 4 0.25) -> id 4
    assert draws([0.3749, 0.0, 0.0, 0.0])[0] == 1 and draws([0.3751, 0.0, 0.0, 0.0])[0] == 3      # either side of 0.375
    assert draws([0.4999, 0.0, 0.0, 0.0])[0] == 3 and draws([0.5001, 0.0, 0.0, 0.0])[0] == 4
    for u in ([0.0] * 4, [one] * 4, [0.5, 0.5, 0.5, 0.5], [0.9, 0.1, 0.9, 0.1]):
        d = draws(u)
        assert len(set(d)) == 4 and all(MASSES[i // 4][i % 4] > 0 for i in d)      # never twice, never a removed entry
    assert draws([0.0] * 4) == [0, 1, 3, 4] and draws([one] * 4) == [6, 4, 3, 1]
    lp, idx = sampling.beam_reference_select(acc, 2, torch.tensor([[0.0, one, 0.39, 0.41]]), True, "5.x", dtype)
    assert torch.equal(lp, acc.reshape(1, -1).gather(1, idx))
    m = sampling.beam_draw_margin(acc, 2, torch.tensor([[0.3749, 0.0, 0.0, 0.0]]))
    assert abs(float(m[0, 0]) - 1e-4) < 1e-6 and float(m[0, 1]) == pytest.approx(0.125, abs=1e-6)


def test_zero_mass_fallback_at_the_start_of_a_search():
    """nb = 5, top_k = 3, the "5.x" start scores: beam 0 alone has mass and only three kept ids, so draws 3..9 take the lowest flat
    indices of finite score."""
    nb, V = 5, 64
    x = bc.rows(1, nb, V, 5)
    rs = bc.running_scores(1, nb, "5.x")
    acc = sampling.beam_reference_rows(x, rs, None, 1.0, bc.EOS, False, True, 0.7, 3, 0.9, "5.x")
    finite = (acc.reshape(-1) > NEG_INF).nonzero().flatten().tolist()
    assert sum(i < V for i in finite) <= 3
    for seed in range(4):
        u = torch.rand(1, 2 * nb, generator=torch.Generator().manual_seed(seed))
        for dtype in (torch.float32, torch.float64):
            lp, idx, draws = sampling.beam_reference_select(acc, nb, u, True, "5.x", dtype, return_draws=True)
            d = draws[0].tolist()
            n0 = sum(i < V for i in finite)
            assert sorted(d[:n0]) == finite[:n0]                       # first beam 0's kept ids, by mass
            assert d[n0:] == finite[n0:2 * nb]                         # then ascending flat index among the finite entries
            assert bool((lp > NEG_INF).all()) and idx.tolist() == draws.tolist()
    assert float(sampling.beam_draw_margin(acc, nb, u)[0, 3:].min()) == float("inf")


def test_the_431_sort_is_stable():
    acc = _acc_of([[0.25, 0.25], [0.25, 0.25]])
    u = torch.tensor([[0.9, 0.1, 0.6, 0.3]])
    lp, idx, draws = sampling.beam_reference_select(acc, 2, u, True, "4.31", torch.float64, return_draws=True)
    assert draws[0].tolist() == [3, 0, 2, 1] and idx.tolist() == draws.tolist()    # equal scores keep draw order
    acc = _acc_of([[0.125, 0.5], [0.125, 0.25]])
    lp, idx, draws = sampling.beam_reference_select(acc, 2, torch.tensor([[0.0, 0.0, 0.0, 0.0]]), True, "4.31", return_draws=True)
    assert draws[0].tolist() == [0, 1, 2, 3] and idx[0].tolist() == [1, 3, 0, 2]
    assert lp[0].tolist() == sorted(lp[0].tolist(), reverse=True)
    with pytest.raises(ValueError):
        sampling.beam_reference_select(acc, 2, u, True, "4.30")


# ------------------------------------------------------------------------------------------------ 3. the host loop with a table
@pytest.fixture(scope="module")
def fake_run(golden_dir):
    import emu_amd.llama as L
    from emu_amd import ops
    saved = L.BF16, ops.embed_gather
    yield bc.fake_engine_run(golden_dir)
    L.BF16, ops.embed_gather = saved


def _table(o, seed, B=2):
    return torch.rand(o["max_new_tokens"], B, 2 * o["num_beams"], generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def test_without_a_table_the_host_loop_returns_what_it_returned_before(fake_run, golden_dir):
    z = np.load(os.path.join(golden_dir, "beam_sample_parent_ids.npz"))
    for name, o in bc.PARENT_SETS.items():
        torch.manual_seed(bc.PARENT_SEED)
        assert fake_run(name, dict(o)).tolist() == z[name].tolist(), name
        torch.manual_seed(bc.PARENT_SEED)
        assert fake_run(name, dict(o), uniforms=None, device_beam_sampler=False).tolist() == z[name].tolist(), name


@pytest.mark.parametrize("name", list(bc.PARENT_SETS))
def test_host_loop_draws_from_the_table(fake_run, name):
    o = bc.PARENT_SETS[name]
    U = _table(o, 3)
    torch.manual_seed(1)
    tr = {}
    a = fake_run(name, dict(o), uniforms=U, trace=tr)
    torch.manual_seed(2)
    b = fake_run(name, dict(o), uniforms=U.clone())
    assert a.tolist() == b.tolist()                                     # deterministic in U, whatever torch's generator holds
    assert tr["draw_margin"] > 0 and "margin" in tr
    outs = {tuple(map(tuple, fake_run(name, dict(o), uniforms=_table(o, s)).tolist())) for s in range(4, 8)}
    assert len(outs) > 1                                                # and the table does decide


def _stand_in_engine(tp_size=1, vocab=1000):
    """A LlamaEngine without a library: every refusal has to come before the first library call, which would fail on it."""
    e = LlamaEngine.__new__(LlamaEngine)
    e.ctx = types.SimpleNamespace(tp_size=tp_size)
    e.vocab = vocab
    return e


def test_refusals_come_before_any_device_work():
    x, mask = torch.zeros(2, 4, 8, dtype=torch.bfloat16), torch.ones(2, 4, dtype=torch.int64)
    for shape in [(6, 2, 5), (6, 1, 6), (5, 2, 6), (6, 12)]:
        with pytest.raises(ValueError, match="uniforms"):
            _stand_in_engine().beam_search_generate(x, mask, 3, 6, do_sample=True, uniforms=torch.zeros(shape))
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        _stand_in_engine().beam_search_generate(x, mask, 3, 6, do_sample=True, device_beam_sampler=True, no_repeat_ngram_size=2)
    with pytest.raises(ValueError, match="tensor parallelism"):
        _stand_in_engine(tp_size=2).beam_search_generate(x, mask, 3, 6, repetition_penalty=1.2, device_beam_sampler=True)
    with pytest.raises(AttributeError):                     # the deterministic, unpenalised search does not look at the flag
        _stand_in_engine(tp_size=2).beam_search_generate(x, mask, 3, 6, device_beam_sampler=True, no_repeat_ngram_size=2)


@pytest.mark.parametrize("kw,why", [(dict(num_beams=9), "9 beams"), (dict(max_new_tokens=257), "257 new tokens"),
                                    (dict(vocab=40001), "vocabulary 40001"), (dict(vocab=5), "below 2"), (dict(trace={}), "trace")])
def test_outside_the_kernels_range_the_host_pipeline_takes_over_with_one_warning(monkeypatch, kw, why):
    kw = dict(kw)
    e = _stand_in_engine(vocab=kw.pop("vocab", 1000))
    nb, n_new = kw.pop("num_beams", 3), kw.pop("max_new_tokens", 6)
    x, mask = torch.zeros(1, 4, 8, dtype=torch.bfloat16), torch.ones(1, 4, dtype=torch.int64)
    monkeypatch.setattr(LlamaEngine, "_warned_beam_sampler", False)
    with pytest.warns(UserWarning, match=why):
        with pytest.raises(AttributeError):                 # the stand-in gets as far as the prefill it does not have
            e.beam_search_generate(x, mask, nb, n_new, do_sample=True, device_beam_sampler=True, **kw)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # once per process
        with pytest.raises(AttributeError):
            e.beam_search_generate(x, mask, nb, n_new, do_sample=True, device_beam_sampler=True, **kw)


# ------------------------------------------------------------------------------------------------ 4. routing
class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a, **k):
            self.calls.append((name, k))
            return torch.zeros(1, 1, dtype=torch.int64)
        return f


PARENT_KEYWORDS = {"eos_id", "pad_id", "do_sample", "temperature", "top_k", "top_p", "repetition_penalty", "no_repeat_ngram_size",
                   "num_return_sequences", "hf_semantics"}


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
def test_the_option_reaches_beam_search_generate_and_nothing_else(make):
    ids, mask = torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, 4, dtype=torch.int64)
    m, rec = make(device_beam_sampler=True)
    m.generate_ids(ids, mask, do_sample=True, num_beams=3, top_p=0.9)
    m.generate_ids(ids, mask, num_beams=3, repetition_penalty=1.2)
    m.generate_ids(ids, mask, do_sample=True, num_beams=3, no_repeat_ngram_size=2)      # the n-gram ban keeps the host loop
    m.generate_ids(ids, mask, do_sample=True, num_beams=1, top_p=0.9)                   # one beam: not this option's business
    assert [c[0] for c in rec.calls] == ["beam_search_generate"] * 3 + ["sample_generate"]
    assert [c[1].get("device_beam_sampler") for c in rec.calls] == [True, True, None, None]
    assert rec.calls[3][1]["device_sampler"] is False
    # off (the attribute missing, as on a model built with __new__, or false): the call is the old one, keyword for keyword
    for attrs in (dict(), dict(device_beam_sampler=False), dict(device_sampler=True)):
        m, rec = make(**attrs)
        m.generate_ids(ids, mask, do_sample=True, num_beams=3, top_p=0.9)
        assert rec.calls[0][0] == "beam_search_generate" and set(rec.calls[0][1]) == PARENT_KEYWORDS, attrs


def test_the_environment_variable_is_the_default(monkeypatch):
    """The constructors with stand-ins for everything that needs a device: the variable must be "1", the argument overrides it, and
    ``device_sampler`` is another switch."""
    import emu_amd.vit as vit
    from emu_amd import emu, emu1
    from emu_amd.conf.emu_conf import LlamaCfg
    for mod in (emu, emu1):
        monkeypatch.setattr(mod, "EmuHipContext", lambda *a, **k: types.SimpleNamespace())
        monkeypatch.setattr(mod, "LlamaEngine", lambda *a, **k: _Recorder())
    monkeypatch.setattr(vit, "VitEngine", lambda *a, **k: None)
    monkeypatch.setattr(emu1, "VitEngine", lambda *a, **k: None)
    monkeypatch.setattr(emu1, "CausalFormer", lambda *a, **k: None)
    makes = (lambda **k: emu.EmuModel(llama_cfg=LlamaCfg(), device="cpu", **k), lambda **k: emu1.Emu(device="cpu", **k))
    ids, mask = torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, 4, dtype=torch.int64)
    for make in makes:
        monkeypatch.delenv("EMU_DEVICE_BEAM_SAMPLER", raising=False)
        monkeypatch.delenv("EMU_DEVICE_SAMPLER", raising=False)
        assert make().device_beam_sampler is False and make(device_sampler=True).device_beam_sampler is False
        assert make(device_beam_sampler=True).device_beam_sampler is True and make(device_beam_sampler=True).device_sampler is False
        for value, want in (("1", True), ("0", False), ("true", False)):
            monkeypatch.setenv("EMU_DEVICE_BEAM_SAMPLER", value)
            assert make().device_beam_sampler is want, value
        assert make(device_beam_sampler=False).device_beam_sampler is False
        monkeypatch.setenv("EMU_DEVICE_BEAM_SAMPLER", "1")
        monkeypatch.setenv("EMU_DEVICE_SAMPLER", "0")
        m = make()
        assert m.device_beam_sampler is True and m.device_sampler is False
