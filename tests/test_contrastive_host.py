"""CPU: the specification of the device loop of contrastive search (``emu_amd/sampling.py``: ``contrastive_reference_candidates`` /
``contrastive_reference_select``) against the host loop ``LlamaEngine.contrastive_generate`` on the stand-in engine, its tie and
padding rules, and the routing and refusals of ``device_contrastive``."""
import types
import warnings

import numpy as np
import pytest
import torch

from emu_amd import llama, ops, sampling
from emu_amd.llama import LlamaEngine
from oracle import emu2_ref as R
from tests import tiny
from tests.fake_engine import FakeEngine


class _RecordingEngine(FakeEngine):
    """The stand-in engine, keeping what the host loop asked of it: the final-normed rows and the logits, call by call."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.normed, self.lgs = [], []

    def final_norm_rows(self, hidden):
        out = super().final_norm_rows(hidden)
        self.normed.append(out.clone())
        return out

    def logits(self, rows, out=None):
        lg = super().logits(rows, out)
        self.lgs.append(lg.clone())
        return lg


@pytest.mark.parametrize("alpha,k,tokens", [(0.6, 2, 8), (0.6, 4, 8)])
def test_spec_restates_the_host_loop(golden_dir, monkeypatch, alpha, k, tokens):
    """For every live step-row the spec gives the traced candidates, probabilities, penalties and selection of the host loop (fp32
    on the stand-in; the smallest winner / runner-up gaps of these runs are 1.95e-4 and 2.1e-5, so no rounding flips a choice)."""
    z = tiny.load(golden_dir, "generate_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    cfg = tiny.oracle_cfg(v, l, vocab)
    monkeypatch.setattr(llama, "BF16", torch.float32)
    monkeypatch.setattr(ops, "embed_gather", lambda ids, table, out=None: out.copy_(table[ids.long()]))
    t = lambda a: torch.from_numpy(np.asarray(a))
    ids, mask = t(z["ids2"]), t(z["mask2"])
    x = R.embed_tokens(ids, W)
    eng = _RecordingEngine(l, vocab, W, cfg.llama)
    trace = {}
    out = LlamaEngine.contrastive_generate(eng, x, mask, tokens, alpha, k, eos_id=-1, trace=trace)
    B, S, H = x.shape
    assert out.shape == (B, tokens) and len(trace["steps"]) == tokens
    kstart = (S - mask.sum(1))
    ctx = eng.normed[0].view(B, S, H).float()
    valid = torch.arange(S)[None, :] >= kstart[:, None]
    logit = eng.lgs[0].float()
    ar = torch.arange(B)
    checked = 0
    for step, st in enumerate(trace["steps"]):
        for dtype in (torch.float32, torch.float64):
            cid, p = sampling.contrastive_reference_candidates(logit, out[:, :step], 1.0, -1, step < 1, k, dtype)
            nh = eng.normed[1 + step].view(B, k, H).float()
            pen, sel = sampling.contrastive_reference_select(ctx, valid, nh, p, alpha, dtype)
            live = st["live"]
            assert torch.equal(cid[live], st["ids"][live]), (step, dtype)
            assert torch.equal(sel[live], st["sel"][live]), (step, dtype)
            assert float((p[live].double() - st["p"][live].double()).abs().max()) <= 1e-6, (step, dtype)
            assert float((pen[live].double() - st["pen"][live].double()).abs().max()) <= 1e-6, (step, dtype)
        checked += int(st["live"].sum())
        sel = st["sel"]
        ctx = torch.cat((ctx, nh[ar, sel][:, None, :]), dim=1)
        valid = torch.cat((valid, torch.ones(B, 1, dtype=torch.bool)), dim=1)
        logit = eng.lgs[1 + step].float().view(B, k, -1)[ar, sel]
    assert checked == B * tokens
    assert trace["margin"] > 1e-5


def test_candidate_ties_go_to_the_lower_id():
    x = torch.full((2, 12), -3.0)
    x[0, 7], x[0, 2] = 4.0, 3.0
    x[0, [9, 5, 10]] = 1.0                                   # three equal logits across the 3rd place: 5 wins, then 9
    x[1, [3, 1, 8]] = 2.0                                    # ties from the top
    ids, p = sampling.contrastive_reference_candidates(x.to(torch.bfloat16), k=4)
    assert ids.tolist() == [[7, 2, 5, 9], [1, 3, 8, 0]]
    assert bool((p[:, :-1] >= p[:, 1:]).all()) and float(p[0, 2]) == float(p[0, 3])
    # the penalty and the suppress act ahead of the ranking
    ids, _ = sampling.contrastive_reference_candidates(x.to(torch.bfloat16), [[7, 7], [1]], 4.0, 2, True, 3)
    assert ids.tolist() == [[5, 7, 9], [3, 8, 1]]


def test_identical_candidates_tie_and_the_lower_index_wins():
    g = torch.Generator().manual_seed(4)
    ctx = torch.randn(1, 6, 16, generator=g)
    c = torch.randn(16, generator=g)
    cand = torch.stack((torch.randn(16, generator=g), c, c))[None]
    p = torch.tensor([[0.0, 0.5, 0.5]])
    for dtype in (torch.float32, torch.float64):
        pen, sel = sampling.contrastive_reference_select(ctx, torch.ones(1, 6, dtype=torch.bool), cand, p, 0.1, dtype)
        assert float(pen[0, 1]) == float(pen[0, 2]) and sel.tolist() == [1]


def test_left_padding_is_left_out_of_the_penalty():
    g = torch.Generator().manual_seed(5)
    ctx = torch.randn(2, 7, 16, generator=g)
    cand = torch.randn(2, 2, 16, generator=g)
    ctx[:, 1] = 3.0 * cand[:, 0]                              # cosine 1 with candidate 0 -- in prompt 0 that row is padding
    valid = torch.ones(2, 7, dtype=torch.bool)
    valid[0, :2] = False
    p = torch.tensor([[0.5, 0.45], [0.5, 0.45]])
    pen, sel = sampling.contrastive_reference_select(ctx, valid, cand, p, 0.6, torch.float64)
    assert float(pen[0, 0]) < 0.9 and abs(float(pen[1, 0]) - 1.0) < 1e-12
    want0 = torch.nn.functional.cosine_similarity(ctx[0, 2:].double(), cand[0, 0].double()[None], dim=1).max()
    assert abs(float(pen[0, 0]) - float(want0)) < 1e-12
    assert int(sel[1]) == 1                                   # prompt 1 sees the row and turns candidate 0 down
    ctx[0, 0] = float("nan")                                  # whatever a padding row holds
    pen2, _ = sampling.contrastive_reference_select(ctx, valid, cand, p, 0.6, torch.float64)
    assert torch.equal(pen2[0], pen[0])


# ------------------------------------------------------------------------------------------------ routing and refusals
class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a, **k):
            self.calls.append((name, k))
            return torch.zeros(1, 1, dtype=torch.int64)
        return f


TODAY = {"eos_id", "pad_id"}                                 # the keywords of the contrastive call as it has been


def _emu2(**attrs):
    from emu_amd.emu import EmuModel
    m = EmuModel.__new__(EmuModel)
    rec = _Recorder()
    m.use_graph, m.hf_semantics = True, "5.x"
    m.n_query = m.v_query = 1
    m.decoder = types.SimpleNamespace(lm=rec)
    m._prompt_embeds = lambda ids, *a, **k: torch.zeros(ids.shape[0] * ids.shape[1], 8)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m, rec


def _emu1(**attrs):
    from emu_amd.emu1 import Emu
    m = Emu.__new__(Emu)
    rec = _Recorder()
    rec.embed_tokens = lambda ids: torch.zeros(*ids.shape, 8)
    m.hf_semantics = "5.x"
    m.lm = rec
    for k, v in attrs.items():
        setattr(m, k, v)
    return m, rec


@pytest.mark.parametrize("make", [_emu2, _emu1])
def test_model_option_routes_the_contrastive_call(make):
    ids, mask = torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, 4, dtype=torch.int64)
    m, rec = make()                                          # no attribute at all: models built with __new__ by older tests
    m.generate_ids(ids, mask, num_beams=1, penalty_alpha=0.6, top_k=4)
    assert rec.calls[-1][0] == "contrastive_generate" and set(rec.calls[-1][1]) == TODAY
    m, rec = make(device_contrastive=False, device_sampler=True, device_beam_sampler=True)     # the other options do not switch it on
    m.generate_ids(ids, mask, num_beams=1, penalty_alpha=0.6, top_k=4)
    assert set(rec.calls[-1][1]) == TODAY
    m, rec = make(device_contrastive=True)
    m.generate_ids(ids, mask, num_beams=1, penalty_alpha=0.6, top_k=4)
    assert rec.calls[-1][0] == "contrastive_generate" and rec.calls[-1][1]["device_contrastive"] is True
    m.generate_ids(ids, mask, num_beams=1, do_sample=True, top_k=4)                              # only that call carries it
    m.generate_ids(ids, mask, num_beams=2)
    m.generate_ids(ids, mask, num_beams=1)
    assert all("device_contrastive" not in c[1] for c in rec.calls[1:])
    with pytest.raises(NotImplementedError):
        m.generate_ids(ids, mask, num_beams=1, penalty_alpha=0.6, top_k=4, no_repeat_ngram_size=2)


def test_environment_variable_sets_the_option(monkeypatch):
    """The constructors read EMU_DEVICE_CONTRASTIVE beside the two sampler variables (their engines stubbed out: no GPU here)."""
    from emu_amd import emu as E, emu1 as E1, vit
    from emu_amd.conf.emu_conf import CLIPVisionCfg, TextDecoderCfg
    stub = lambda *a, **k: types.SimpleNamespace()
    monkeypatch.setattr(vit, "VitEngine", stub)
    monkeypatch.setattr(E, "LlamaEngine", stub)
    monkeypatch.setattr(E, "_Decoder", stub)
    monkeypatch.setattr(E1, "VitEngine", stub)
    monkeypatch.setattr(E1, "LlamaEngine", stub)
    monkeypatch.setattr(E1, "CausalFormer", stub)
    ctx = types.SimpleNamespace(device=torch.device("cpu"))
    mk2 = lambda **k: E.EmuModel(CLIPVisionCfg(), TextDecoderCfg(), llama_cfg=object(), device="cpu", ctx=ctx, **k)
    mk1 = lambda **k: E1.Emu(device="cpu", ctx=ctx, **k)
    for mk in (mk2, mk1):
        monkeypatch.delenv("EMU_DEVICE_CONTRASTIVE", raising=False)
        assert mk().device_contrastive is False and mk(device_contrastive=True).device_contrastive is True
        monkeypatch.setenv("EMU_DEVICE_SAMPLER", "1")
        monkeypatch.setenv("EMU_DEVICE_BEAM_SAMPLER", "1")
        assert mk().device_contrastive is False              # an option of its own
        monkeypatch.setenv("EMU_DEVICE_CONTRASTIVE", "1")
        m = mk()
        assert m.device_contrastive is True and mk(device_contrastive=False).device_contrastive is False
        monkeypatch.delenv("EMU_DEVICE_SAMPLER")
        monkeypatch.delenv("EMU_DEVICE_BEAM_SAMPLER")
    # ... and the variable alone reaches the call
    m, rec = _emu2(device_contrastive=mk2().device_contrastive)
    m.generate_ids(torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, 4, dtype=torch.int64), num_beams=1, penalty_alpha=0.6, top_k=4)
    assert rec.calls[-1][1]["device_contrastive"] is True


def _stand_in_engine(tp_size=1, vocab=1000):
    """A LlamaEngine without a library: every refusal has to come before the first library call, which would fail on it."""
    e = LlamaEngine.__new__(LlamaEngine)
    e.ctx = types.SimpleNamespace(tp_size=tp_size)
    e.vocab = vocab
    return e


def test_tensor_parallelism_is_refused_before_any_library_call():
    x, mask = torch.zeros(1, 4, 8, dtype=torch.bfloat16), torch.ones(1, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="tensor parallelism"):
        _stand_in_engine(tp_size=2).contrastive_generate(x, mask, 4, 0.6, 4, device_contrastive=True)
    with pytest.raises(AttributeError):                      # without the option the stand-in gets as far as its missing engine
        _stand_in_engine(tp_size=2).contrastive_generate(x, mask, 4, 0.6, 4)


@pytest.mark.parametrize("case", ["top_k", "vocab", "trace", "force_ids"])
def test_out_of_range_calls_warn_once_and_keep_the_host_loop(golden_dir, monkeypatch, case):
    z = tiny.load(golden_dir, "generate_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    cfg = tiny.oracle_cfg(v, l, vocab)
    monkeypatch.setattr(llama, "BF16", torch.float32)
    monkeypatch.setattr(ops, "embed_gather", lambda ids, table, out=None: out.copy_(table[ids.long()]))
    monkeypatch.setattr(LlamaEngine, "_warned_contrastive", False)
    monkeypatch.setattr(LlamaEngine, "_contrastive_device", lambda *a, **k: pytest.fail("the device loop was entered"))
    t = lambda a: torch.from_numpy(np.asarray(a))
    ids, mask = t(z["ids2"]), t(z["mask2"])
    x = R.embed_tokens(ids, W)

    def eng():
        e = FakeEngine(l, vocab, W, cfg.llama)
        e.ctx.tp_size = 1
        return e

    k = 9 if case == "top_k" else 3
    want = LlamaEngine.contrastive_generate(eng(), x, mask, 3, 0.6, k, eos_id=-1)
    kw = dict(trace={}) if case == "trace" else dict(force_ids=want) if case == "force_ids" else {}
    if case == "vocab":
        # the refusal reads the engine's vocabulary: a stand-in without a library warns, then gets as far as its missing engine
        with pytest.warns(UserWarning, match="device_contrastive") as rec:
            with pytest.raises(AttributeError):
                _stand_in_engine(vocab=40001).contrastive_generate(x, mask, 3, 0.6, k, eos_id=-1, device_contrastive=True)
        assert len(rec) == 1 and "40001" in str(rec[0].message)
        return
    with pytest.warns(UserWarning, match="device_contrastive") as rec:
        got = LlamaEngine.contrastive_generate(eng(), x, mask, 3, 0.6, k, eos_id=-1, device_contrastive=True, **kw)
    assert len(rec) == 1 and got.tolist() == want.tolist()
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # one warning per process
        again = LlamaEngine.contrastive_generate(eng(), x, mask, 3, 0.6, k, eos_id=-1, device_contrastive=True, **kw)
    assert again.tolist() == want.tolist()
    assert "trace" not in kw or kw["trace"]["steps"]
