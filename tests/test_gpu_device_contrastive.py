"""GPU: the device loop of contrastive search (``LlamaEngine.contrastive_generate(device_contrastive=True)``: the kernels of
emu_amd/csrc/contrastive.hip around the decoder step, eager and replayed from a hipGraph) on the tiny model of
tests/golden/generate_tiny.npz."""
import numpy as np
import pytest
import torch

from emu_amd import llama
from tests import tiny
from tests.test_gpu_contrastive import cos_tol

pytestmark = pytest.mark.gpu
PAD = 32000
ALPHA = 0.6


def _t(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def tiny_model(golden_dir):
    from emu_amd import EmuModel, TextDecoderCfg
    z = tiny.load(golden_dir, "generate_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    m = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda", device_contrastive=False)
    m.load_state_dict(W, strict=True)
    return m, z


@pytest.fixture(scope="module")
def prompts(tiny_model):
    """(one prompt with an image, two ragged left-padded text prompts) as (embeds [B, S, hidden], mask)."""
    m, z = tiny_model
    ids1, ids2 = _t(z["ids1"]), _t(z["ids2"])
    x1 = m._prompt_embeds(ids1, _t(z["image"]).cuda(), m.n_query).view(1, ids1.shape[1], -1)
    x2 = m._prompt_embeds(ids2, None, m.n_query).view(2, ids2.shape[1], -1)
    return (x1, _t(z["mask1"])), (x2, _t(z["mask2"]))


def _dev(lm, x, mask, n, alpha, k, graph=False, **kw):
    return lm.contrastive_generate(x, mask, n, alpha, k, pad_id=PAD, device_contrastive=True, use_graph=graph, **kw).cpu()


@pytest.fixture(scope="module")
def free_runs(tiny_model, prompts):
    """8 tokens with no EOS in reach, alpha 0.6, k = 4: the ragged pair and the single prompt.  The runs the EOS tests cut short."""
    lm = tiny_model[0].decoder.lm
    return _dev(lm, *prompts[1], 8, ALPHA, 4, eos_id=-1), _dev(lm, *prompts[0], 8, ALPHA, 4, eos_id=-1)


def test_vanishing_penalty_gives_the_reference_greedy_ids(tiny_model, prompts):
    m, z = tiny_model
    lm = m.decoder.lm
    for graph in (False, True):
        assert _dev(lm, *prompts[0], 8, 1e-9, 4, graph).tolist() == z["new1"].tolist(), graph
        assert _dev(lm, *prompts[1], 6, 1e-9, 3, graph).tolist() == z["new2"].tolist(), graph


@pytest.mark.parametrize("k", [2, 4])
def test_a_real_penalty_follows_the_host_loop(tiny_model, prompts, k):
    """The host loop on the same engine replays the device's ids (``force_ids`` raises unless every one of them is among that
    step's host candidates) and traces its own numbers.  With SELECT_TOL = (1 - alpha) * 1e-5 + alpha * COS_TOL the rounding of one
    side's score, at every live step-row the device's choice scores within 2 * SELECT_TOL of the host's best, and it IS the
    host's choice wherever the host's winner leads by more than that; at least three quarters of the step-rows are decided in this
    second way.  Measured on an MI355X: the host's gaps are 4e-4 .. 8e-2 and all 16 step-rows are decided by equality, for k = 2
    and k = 4; 7 and 10 of them keep another candidate than the most probable."""
    lm = tiny_model[0].decoder.lm
    x, mask = prompts[1]
    H = x.shape[2]
    select_tol = (1.0 - ALPHA) * 1e-5 + ALPHA * cos_tol(H)
    ids = _dev(lm, x, mask, 8, ALPHA, k, eos_id=-1)
    assert ids.shape == (2, 8)
    trace = {}
    host = lm.contrastive_generate(x, mask, 8, ALPHA, k, eos_id=-1, pad_id=PAD, trace=trace, force_ids=ids).cpu()
    assert torch.equal(host, ids) and len(trace["steps"]) == 8
    rows = decided = other = 0
    for step, st in enumerate(trace["steps"]):
        score = (1.0 - ALPHA) * st["p"].double() - ALPHA * st["pen"].double()
        for b in range(2):
            assert bool(st["live"][b])
            j = st["ids"][b].tolist().index(int(ids[b, step]))
            srt = torch.sort(score[b], descending=True)[0]
            gap, short = float(srt[0] - srt[1]), float(srt[0] - score[b, j])
            print(f"k {k} step {step} row {b}: host gap {gap:.3g}, device's choice {j} is {short:.3g} below the host's best")
            rows += 1
            assert short <= 2 * select_tol, (step, b)
            if gap > 2 * select_tol:
                decided += 1
                assert j == int(score[b].argmax()), (step, b)
            other += j != 0
    print(f"k {k}: {decided} of {rows} step-rows decided by equality, {other} keep another candidate than the most probable")
    assert rows == 16 and 4 * decided >= 3 * rows
    assert other >= 1
    for graph in (False, True):                              # eager, replayed and again: the same ids
        assert torch.equal(_dev(lm, x, mask, 8, ALPHA, k, graph, eos_id=-1), ids), graph
    assert torch.equal(_dev(lm, x, mask, 8, ALPHA, k, True, eos_id=-1), ids)


def test_a_second_prompt_of_the_same_shape_replays_the_same_graph(tiny_model, prompts, free_runs):
    lm = tiny_model[0].decoder.lm
    x, mask = prompts[1]
    assert torch.equal(_dev(lm, x, mask, 8, ALPHA, 4, True, eos_id=-1), free_runs[0])
    st = lm._loop_states["contrastive"][1]
    g = st["captured"].graph
    assert g is not None
    got = _dev(lm, x.flip(0).contiguous(), mask.flip(0).contiguous(), 8, ALPHA, 4, True, eos_id=-1)
    assert torch.equal(got, free_runs[0].flip(0))            # prompts never interact
    st2 = lm._loop_states["contrastive"][1]
    assert st2 is st and st2["captured"].graph is g


def test_eos_pads_a_prompt_and_the_width_is_the_host_loops(tiny_model, prompts, free_runs, monkeypatch):
    """Prompts never interact, so with token T declared EOS the result is the free run with PAD after each prompt's first T, cut one
    past the last step at which a prompt was unfinished (``apply_eos_padding``) -- and what the host loop returns when it is led
    along the same token path.  The interval of the host's look at the flags changes nothing."""
    lm = tiny_model[0].decoder.lm
    for (x, mask), free in zip((prompts[1], prompts[0]), free_runs):
        eos = int(free[0, 2])
        want = llama.apply_eos_padding(free, eos, PAD)
        if free.shape[0] == 2:                               # prompt 0 pads from its first T on, prompt 1 goes on
            first = int((free[0] == eos).nonzero()[0, 0])
            assert bool((want[0, first + 1:] == PAD).all()) and first <= 2
            if not bool((free[1] == eos).any()):
                assert want.shape[1] == 8 and torch.equal(want[1], free[1])
        else:                                                # the only prompt ends: the width shrinks
            assert want.shape[1] <= 3
        host = lm.contrastive_generate(x, mask, 8, ALPHA, 4, min_len=0, eos_id=eos, pad_id=PAD, force_ids=free).cpu()
        assert host.tolist() == want.tolist()
        for poll in (2, 4):
            monkeypatch.setattr(llama.LlamaEngine, "BEAM_POLL", poll)
            for graph in (False, True):
                got = _dev(lm, x, mask, 8, ALPHA, 4, graph, min_len=0, eos_id=eos)      # min_len = 0: T is never suppressed
                assert got.tolist() == want.tolist(), (poll, graph)


def test_minimum_length_keeps_eos_out(tiny_model, prompts, free_runs):
    lm = tiny_model[0].decoder.lm
    x, mask = prompts[1]
    eos = int(free_runs[0][0, 0])
    for graph in (False, True):
        got = _dev(lm, x, mask, 8, ALPHA, 4, graph, min_len=3, eos_id=eos)
        assert got.shape[1] >= 3 and not bool((got[:, :3] == eos).any()), graph
    got = _dev(lm, x, mask, 8, ALPHA, 4, min_len=0, eos_id=eos)
    assert int(got[0, 0]) == eos and bool((got[0, 1:] == PAD).all())


def test_model_option_and_environment_reach_the_device_loop(tiny_model, monkeypatch):
    from emu_amd import EmuModel, TextDecoderCfg
    m, z = tiny_model
    ids, mask, img = _t(z["ids1"]), _t(z["mask1"]), _t(z["image"]).cuda()
    calls = []
    real = llama.LlamaEngine._contrastive_device
    monkeypatch.setattr(llama.LlamaEngine, "_contrastive_device", lambda self, *a, **k: calls.append(a[-1]) or real(self, *a, **k))
    assert m.device_contrastive is False
    a = m.generate_ids(ids, mask, img, max_new_tokens=8, penalty_alpha=1e-9, top_k=4)
    assert a.cpu().tolist() == z["new1"].tolist() and not calls
    monkeypatch.setattr(m, "device_contrastive", True)
    for graph in (False, True):
        monkeypatch.setattr(m, "use_graph", graph)
        assert m.generate_ids(ids, mask, img, max_new_tokens=8, penalty_alpha=1e-9, top_k=4).cpu().tolist() == z["new1"].tolist()
    assert calls == [False, True]
    m.generate_ids(ids, mask, img, max_new_tokens=4, do_sample=True, top_k=5)          # sampling: as before
    m.generate_ids(ids, mask, img, max_new_tokens=4, num_beams=2, hf_semantics="5.x")  # beam search: as before
    assert len(calls) == 2
    v, l, vocab, W = tiny.weights_from(z)
    monkeypatch.setenv("EMU_DEVICE_CONTRASTIVE", "1")
    assert EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda", ctx=m.ctx).device_contrastive is True
    monkeypatch.delenv("EMU_DEVICE_CONTRASTIVE")
    assert EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda", ctx=m.ctx).device_contrastive is False


def test_the_engine_is_left_as_it_was(tiny_model, prompts):
    """After the device loop the KV sharing is reset and the caches are intact: the next greedy run returns its usual ids."""
    m, z = tiny_model
    lm = m.decoder.lm
    _dev(lm, *prompts[1], 8, ALPHA, 4, True, eos_id=-1)
    assert lm.greedy_generate(*prompts[0], 8).cpu().tolist() == z["new1"].tolist()
    _dev(lm, *prompts[0], 8, ALPHA, 4, False, eos_id=-1)
    assert lm.greedy_generate(*prompts[1], 6).cpu().tolist() == z["new2"].tolist()
