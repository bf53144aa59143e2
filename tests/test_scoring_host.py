"""CPU: the scoring specification (emu_amd/scoring.py) against torch.log_softmax and torch.nn.CrossEntropyLoss, the reference's
candidate loss (Emu1/models/modeling_llama.py:110-116) written out from torch's loss, and the host logic of ``LlamaEngine.score`` /
``score_continuations`` / ``Emu.predict`` on stand-in engines (the pattern of tests/test_sampling_host.py)."""
import types

import pytest
import torch

from emu_amd import scoring
from emu_amd.device_loop import CapturedStep
from emu_amd.llama import LlamaEngine

BF16 = torch.bfloat16


def _rows(B, V, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, V, generator=g) * scale).to(BF16)


# ------------------------------------------------------------------------------------------------ the spec against the library
@pytest.mark.parametrize("V", (50, 1027, 32274))
def test_spec_equals_log_softmax_and_cross_entropy(V):
    x = _rows(4, V, V)
    t = torch.tensor([0, V - 1, V // 2, 7])
    xf = x.float()
    want = torch.log_softmax(xf, -1).gather(1, t[:, None])[:, 0]
    got = scoring.reference_logprob(x, t)
    assert got["lp"].dtype == torch.float32 and float((got["lp"] - want).abs().max()) < 2e-5
    ce = torch.nn.CrossEntropyLoss(ignore_index=-100, reduction="none")(xf, t)
    assert float((-got["lp"] - ce).abs().max()) < 2e-5
    assert bool(got["counted"].all())
    assert torch.equal(got["top1"], xf.argmax(-1))           # random rows have one maximum
    # fp64: the match is to rounding -- of the fp32 exponentials, which dtype does not widen: exp(x - m) carries at most 2 ulp of
    # fp32 (2 * 2^-24 relative), so does their sum, and the logarithm of it moves by at most that: 1.2e-7
    g64 = scoring.reference_logprob(x, t, dtype=torch.float64)
    w64 = torch.log_softmax(xf.double(), -1).gather(1, t[:, None])[:, 0]
    assert g64["lp"].dtype == torch.float64 and float((g64["lp"] - w64).abs().max()) < 1.2e-7
    assert float((g64["lse"] - torch.logsumexp(xf.double(), -1)).abs().max()) < 1.2e-7
    ce64 = torch.nn.CrossEntropyLoss(ignore_index=-100, reduction="none")(xf.double(), t)
    assert float((-g64["lp"] - ce64).abs().max()) < 1.2e-7


def test_ignored_targets_give_exactly_zero_and_are_not_counted():
    V = 97
    x = _rows(4, V, 1)
    t = torch.tensor([-100, V, 5, -1])
    for dt in (torch.float32, torch.float64):
        got = scoring.reference_logprob(x, t, dtype=dt)
        assert got["counted"].tolist() == [False, False, True, False]
        assert got["lp"][[0, 1, 3]].tolist() == [0.0, 0.0, 0.0] and float(got["lp"][2]) < 0
    ce = torch.nn.CrossEntropyLoss(ignore_index=-100, reduction="none")(x.float(), torch.tensor([-100, -100, 5, -100]))
    assert ce[[0, 1, 3]].tolist() == [0.0, 0.0, 0.0]        # the reference's zeros: what "ignored" restates
    assert abs(float(ce[2]) + float(scoring.reference_logprob(x, t)["lp"][2])) < 2e-5


def test_minus_infinity_at_the_target_gives_minus_infinity_not_nan():
    x = _rows(2, 50, 2)
    x[:, 3] = -float("inf")
    x[1, 10:20] = -float("inf")
    got = scoring.reference_logprob(x, torch.tensor([3, 4]))
    assert float(got["lp"][0]) == -float("inf")
    assert torch.isfinite(got["lp"][1]) and bool(torch.isfinite(got["lse"]).all())


def test_kl_of_a_row_with_itself_is_exactly_zero_and_kl_rules():
    x = _rows(3, 1027, 3)
    x[2, ::5] = -float("inf")
    t = torch.zeros(3, dtype=torch.int64)
    for dt in (torch.float32, torch.float64):
        got = scoring.reference_logprob(x, t, ref_logits=x.clone(), dtype=dt)
        assert got["kl"].tolist() == [0.0, 0.0, 0.0] and bool(got["agree"].all())
    r = _rows(3, 1027, 4)
    got = scoring.reference_logprob(x, t, ref_logits=r, dtype=torch.float64)
    # (two log-sum-exps of fp32 exponentials enter: twice the bound of one, see above)
    px, pr = torch.log_softmax(x.double(), -1), torch.log_softmax(r.double(), -1)
    want = torch.nn.functional.kl_div(px[:2], pr[:2], reduction="none", log_target=True).sum(-1)
    assert float((got["kl"][:2] - want).abs().max()) < 2.4e-7 and bool((got["kl"][:2] > 0).all())
    assert float(got["kl"][2]) == float("inf")             # x rules out tokens the reference allows
    # the other way round the -inf entries of the reference have p_r == 0 and contribute nothing
    back = scoring.reference_logprob(r, t, ref_logits=x, dtype=torch.float64)
    assert bool(torch.isfinite(back["kl"]).all()) and bool((back["kl"] > 0).all())
    assert torch.equal(back["agree"], x.float().argmax(-1) == r.float().argmax(-1))


def test_a_tie_for_top1_goes_to_the_lower_id():
    x = torch.tensor([[1.0, 3.0, 3.0, -2.0], [0.5, 0.5, 0.25, 0.5], [2.0, 2.0, 2.0, 2.0]]).to(BF16)
    assert scoring.reference_logprob(x, torch.zeros(3, dtype=torch.int64))["top1"].tolist() == [1, 0, 0]


# ------------------------------------------------------------------------------------------------ the reference's candidate loss
def test_candidate_losses_equal_the_reference_loss_written_out():
    """modeling_llama.py:110-116 written out: shift logits and labels, CrossEntropyLoss(reduction="none") over all positions,
    ``.view(B, -1).mean(1)``.  Two segments whose longest candidates differ, so the per-segment denominator shows."""
    V, S = 64, 5
    g = torch.Generator().manual_seed(7)
    cands = [[3, 9], [4], [7, 8, 1, 2], [5, 6, 7]]                        # segments [0:2] (Tmax 2) and [2:4] (Tmax 4)
    segments = scoring.split_segments(len(cands), 2)
    assert segments == [(0, 2), (2, 4)]
    Tc = max(len(c) for c in cands)
    # stand-in "model": any logits will do, the candidate's positions must see the same rows in both computations
    all_lp = torch.zeros(len(cands), Tc)
    counted = torch.zeros(len(cands), Tc, dtype=torch.bool)
    want = torch.zeros(len(cands))
    for a, b in segments:
        tmax = max(len(c) for c in cands[a:b])
        n = b - a
        logits = torch.randn(n, S + tmax, V, generator=g)
        labels = torch.full((n, S + tmax), -100, dtype=torch.int64)
        for i, c in enumerate(cands[a:b]):
            labels[i, S:S + len(c)] = torch.tensor(c)
        shift_logits = logits[..., :-1, :].contiguous()
        shift_labels = labels[..., 1:].contiguous()
        loss = torch.nn.CrossEntropyLoss(reduction="none")(shift_logits.view(-1, V), shift_labels.view(-1))
        want[a:b] = loss.view(n, -1).mean(1)
        # the same positions through the spec: position t of the candidate is scored by the row before it
        tgt = torch.full((n, tmax), -100, dtype=torch.int64)
        for i, c in enumerate(cands[a:b]):
            tgt[i, :len(c)] = torch.tensor(c)
        r = scoring.reference_logprob(logits[:, S - 1:S + tmax - 1], tgt)
        all_lp[a:b, :tmax], counted[a:b, :tmax] = r["lp"], r["counted"]
        got = scoring.reference_candidate_losses(all_lp[a:b], counted[a:b], S, tmax)
        assert float((got - want[a:b]).abs().max()) < 1e-5
    # the quirk: one denominator for all would rank differently scaled losses
    one = scoring.reference_candidate_losses(all_lp, counted, S, Tc)
    assert float((one[:2] - want[:2]).abs().max()) > 1e-3 and float((one[2:] - want[2:]).abs().max()) < 1e-5


@pytest.mark.parametrize("n,k,want", [(6, 1, [(0, 6)]), (6, 2, [(0, 3), (3, 6)]), (7, 2, [(0, 3), (3, 7)]),
                                      (7, 3, [(0, 2), (2, 4), (4, 7)]), (5, 5, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)])])
def test_segments_split_as_the_reference_does(n, k, want):
    """prediction_mixin.py:84-90: n // k candidates per segment, the last segment takes the remainder."""
    assert scoring.split_segments(n, k) == want
    ref = []
    for i in range(k):
        seg = n // k
        if i == k - 1:
            seg = n - seg * (k - 1)
        start = i * (n // k)
        ref.append((start, start + seg))
    assert ref == want


def test_segment_count_out_of_range_is_refused():
    for k in (0, -1, 7):
        with pytest.raises(ValueError):
            scoring.split_segments(6, k)


# ------------------------------------------------------------------------------------------------ host logic on stand-in engines
def _stand_in_engine(vocab=1000, hidden=8, max_pos=64):
    """A LlamaEngine without a library: every refusal has to come before the first library call, which would fail on it."""
    e = LlamaEngine.__new__(LlamaEngine)
    e.ctx = types.SimpleNamespace(tp_size=1)
    e.vocab = vocab
    e.cfg = types.SimpleNamespace(hidden_size=hidden, max_position_embeddings=max_pos)
    return e


def test_score_refusals_come_before_any_library_call():
    e = _stand_in_engine()
    x, mask = torch.zeros(2, 4, 8, dtype=BF16), torch.ones(2, 4, dtype=torch.int64)
    ids = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="via"):
        e.score(x, mask, ids, via="beam")
    with pytest.raises(ValueError, match="prefix_mask"):
        e.score(x, mask[:, :3], ids)
    with pytest.raises(ValueError, match="cont_ids"):
        e.score(x, mask, ids[:1])
    with pytest.raises(ValueError, match="cont_mask"):
        e.score(x, mask, ids, torch.ones(2, 2, dtype=torch.bool))
    with pytest.raises(ValueError, match="at least one"):
        e.score(x, mask, ids[:, :0])
    with pytest.raises(ValueError, match="max_position_embeddings"):
        e.score(x, mask, torch.zeros(2, 61, dtype=torch.int64))
    with pytest.raises(ValueError, match="prefix_embeds"):
        e.score(x[..., :4], mask, ids)
    with pytest.raises(ValueError, match="reference_logits"):
        e.score(x, mask, ids, reference_logits=torch.zeros(2, 3, 999, dtype=BF16))
    with pytest.raises(ValueError, match="64 rows"):
        e.score(torch.zeros(65, 4, 8, dtype=BF16), torch.ones(65, 4), torch.zeros(65, 3, dtype=torch.int64), via="decode")
    with pytest.raises(AttributeError):                     # valid arguments get as far as the stand-in's missing engine
        e.score(x, mask, ids)
    # score_continuations: one prefix, and the same checks per segment
    cands = torch.zeros(6, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"\[1, S, hidden\]"):
        e.score_continuations(x, mask, cands)
    with pytest.raises(ValueError, match="n_segments"):
        e.score_continuations(x[:1], mask[:1], cands, n_segments=7)
    with pytest.raises(ValueError, match="via"):
        e.score_continuations(x[:1], mask[:1], cands, via="sideways")
    with pytest.raises(ValueError, match="cont_mask"):
        e.score_continuations(x[:1], mask[:1], cands, torch.ones(6, 2, dtype=torch.bool))
    with pytest.raises(ValueError, match="max_position_embeddings"):
        e.score_continuations(x[:1], mask[:1], torch.zeros(6, 61, dtype=torch.int64))


def test_score_targets_mark_masked_and_out_of_vocabulary_ids_as_ignored():
    e = _stand_in_engine(vocab=100)
    e.device = torch.device("cpu")
    ids = torch.tensor([[5, 99, 100, -3], [7, 8, 9, 10]])
    mask = torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0]], dtype=torch.bool)
    t = e._score_targets(ids, mask)
    assert t.dtype == torch.int32
    assert t.tolist() == [[5, 99, -100, -100], [7, 8, -100, -100]]
    assert e._score_targets(ids, None).tolist() == [[5, 99, -100, -100], [7, 8, 9, 10]]


class _FakeLm:
    """Stands in for LlamaEngine below Emu.predict_ids: per-token log-probabilities by a fixed rule."""

    def __init__(self):
        self.calls = []

    def embed_tokens(self, ids):
        return torch.zeros(*ids.shape, 8)

    def score_continuations(self, x, mask, cand_ids, cand_mask, n_segments=1, via="prefill", hf_generate_positions=True):
        self.calls.append(dict(n=cand_ids.shape[0], n_segments=n_segments, via=via, hf=hf_generate_positions, S=x.shape[1]))
        lp = -(cand_ids.float() + 1.0) / 10.0
        return lp * cand_mask, cand_mask.clone()


def _stand_in_emu1():
    from emu_amd.emu1 import Emu
    m = Emu.__new__(Emu)
    m.lm = _FakeLm()
    m.ctx = types.SimpleNamespace(device=torch.device("cpu"))
    m.tokenizer = None
    return m


def test_predict_ids_ranks_by_the_reference_loss_per_segment():
    m = _stand_in_emu1()
    ids, mask = torch.ones(1, 5, dtype=torch.int64), torch.ones(1, 5, dtype=torch.int64)
    cand = torch.tensor([[4, 0, 0], [1, 1, 0], [9, 9, 9], [2, 0, 0]])
    cmask = torch.tensor([[1, 0, 0], [1, 1, 0], [1, 1, 1], [1, 0, 0]], dtype=torch.bool)
    ranks, losses = m.predict_ids(ids, mask, None, cand, cmask, n_segments=1, return_losses=True)
    assert ranks.shape == (1, 4) and ranks.dtype == torch.int64
    want = torch.tensor([0.5, 0.4, 3.0, 0.3]) / (5 + 3 - 1)
    assert float((losses - want).abs().max()) < 1e-6
    assert ranks.tolist() == [[3, 1, 0, 2]]
    assert m.lm.calls[-1] == dict(n=4, n_segments=1, via="prefill", hf=False, S=5)        # arange positions, one call
    # two segments: [0:2] is padded to 2 tokens, [2:4] to 3: another denominator
    ranks2, losses2 = m.predict_ids(ids, mask, None, cand, cmask, n_segments=2, return_losses=True)
    want2 = torch.tensor([0.5 / 6, 0.4 / 6, 3.0 / 7, 0.3 / 7])
    assert float((losses2 - want2).abs().max()) < 1e-6
    assert ranks2.tolist() == [[3, 1, 0, 2]] and m.lm.calls[-1]["n_segments"] == 2
    with pytest.raises(ValueError, match="one prompt"):
        m.predict_ids(torch.ones(2, 5, dtype=torch.int64), torch.ones(2, 5), None, cand, cmask)


class _Tok:
    """Whitespace 'tokenizer': a word is its integer value; pads with id 0 on ``padding_side``."""
    pad_token_id = 0
    padding_side = "right"

    def __call__(self, text, padding="longest", return_tensors="pt", add_special_tokens=True):
        text = [text] if isinstance(text, str) else list(text)
        rows = [([1] if add_special_tokens else []) + [int(w) for w in t.split()] for t in text]
        width = max(len(r) for r in rows)
        ids = torch.zeros(len(rows), width, dtype=torch.int64)
        am = torch.zeros(len(rows), width, dtype=torch.int64)
        for i, r in enumerate(rows):
            sl = slice(width - len(r), width) if self.padding_side == "left" else slice(0, len(r))
            ids[i, sl], am[i, sl] = torch.tensor(r), 1
        self.log = getattr(self, "log", []) + [(self.padding_side, add_special_tokens, len(rows))]
        return types.SimpleNamespace(input_ids=ids, attention_mask=am)


def test_predict_needs_a_tokenizer_and_returns_ranks():
    m = _stand_in_emu1()
    with pytest.raises(RuntimeError, match="set Emu.tokenizer"):
        m.predict({"prompt": ["3 4"], "image": None}, ["4", "1 1"])
    m.tokenizer = _Tok()
    ranks = m.predict({"prompt": ["3 4 5"], "image": None}, ["4", "1 1", "9 9 9", "2"])
    assert ranks.shape == (1, 4) and ranks.dtype == torch.int64 and ranks.tolist() == [[3, 1, 0, 2]]
    # the prompt left padded with special tokens, the candidates right padded without (prediction_mixin.py:53-60,92-97)
    assert m.tokenizer.log == [("left", True, 1), ("right", False, 4)] and m.tokenizer.padding_side == "right"
    assert m.lm.calls[-1]["S"] == 4


def test_predict_list_of_lists_concatenates():
    m = _stand_in_emu1()
    m.tokenizer = _Tok()
    m._prompt_embeds = lambda ids, image: torch.zeros(1, ids.shape[1], 8)
    samples = {"prompt": ["3 4", "5 6 7"], "image": torch.zeros(2, 3, 4, 4)}
    out = m.predict(samples, [["4", "1 1", "2"], ["2", "9", "1 1"]])
    assert isinstance(out, torch.Tensor) and out.shape == (2, 3) and out.dtype == torch.int64
    assert out.tolist() == [[2, 1, 0], [0, 2, 1]]
    assert [c["n"] for c in m.lm.calls] == [3, 3]
    ragged = m.predict(samples, (["4", "1 1", "2"], ["2", "9"]))      # lists of different length: a plain list, as the reference's
    assert ragged == [[2, 1, 0], [0, 1]]


# ------------------------------------------------------------------------------------------------ the captured step
def test_score_state_replays_one_captured_step_under_the_same_key():
    from emu_amd.llama import ScoreState
    log = []

    class G:
        def replay(self):
            log.append("replay")

    st = ScoreState.__new__(ScoreState)
    st.eng = types.SimpleNamespace(mode_epoch=3)
    st.captured = CapturedStep(capture=lambda body: (log.append("capture"), G())[1])
    st.step = lambda: log.append("step")
    st.step_graph()
    assert log == ["step", "capture"]                       # first use: one real step, then the capture
    st.step_graph()
    st.step_graph()
    assert log == ["step", "capture", "replay", "replay"]   # the same key: replays
    st.eng.mode_epoch = 4                                   # a mode switch (another weight stream): captured anew
    st.step_graph()
    assert log[-2:] == ["step", "capture"]


def test_symbols_are_declared_with_their_citations():
    from emu_amd import _lib
    txt = open(_lib.HEADER_PATH).read()
    for name in ("emu_token_logprob_bf16", "emu_llama_score_step"):
        assert name in _lib._PROTOS and name in _lib.declared_symbols()
    for cite in ("prediction_mixin.py:36-131", "modeling_llama.py:110-116"):
        assert cite in txt
