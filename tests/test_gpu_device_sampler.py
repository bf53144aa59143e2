"""GPU: the device-side sampling loop (``LlamaEngine.sample_generate(device_sampler=True)``: ``emu_sample_bf16`` for the first token,
``emu_llama_sample_step`` per further token, eager and replayed from a hipGraph) on the tiny model of tests/golden/generate_tiny.npz."""
import numpy as np
import pytest
import torch

from emu_amd import llama, ops, sampling
from tests import tiny
from tests.test_gpu_sampler import DRAW_TOL

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
PAD = 32000
SAMPLING = dict(do_sample=True, temperature=0.9, top_p=0.95, top_k=50)


def _t(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def tiny_model(golden_dir):
    from emu_amd import EmuModel, TextDecoderCfg
    z = tiny.load(golden_dir, "generate_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    m = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda", device_sampler=False)
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


@pytest.fixture(scope="module")
def uniforms():
    return torch.rand(8, 2, generator=torch.Generator().manual_seed(21), dtype=torch.float32).cuda()


@pytest.fixture(scope="module")
def free_run(tiny_model, prompts, uniforms):
    """8 sampled tokens of the two-prompt batch with no EOS in reach: the run the EOS tests cut short."""
    lm = tiny_model[0].decoder.lm
    x, mask = prompts[1]
    return lm.sample_generate(x, mask, 8, eos_id=-1, pad_id=PAD, device_sampler=True, uniforms=uniforms, **SAMPLING).cpu()


def test_equals_the_existing_paths_eager_and_replayed(tiny_model, prompts):
    m, z = tiny_model
    lm = m.decoder.lm
    x, mask = prompts[0]
    greedy = z["new1"].tolist()
    host = lm.sample_generate(x, mask, 8, do_sample=False, repetition_penalty=1.5).cpu().tolist()
    assert host != greedy                                    # the fixture on which the penalty changes the output
    for graph in (False, True):
        got = lm.sample_generate(x, mask, 8, do_sample=False, repetition_penalty=1.5, device_sampler=True, use_graph=graph)
        assert got.cpu().tolist() == host, graph
        got = lm.sample_generate(x, mask, 8, do_sample=True, top_k=1, device_sampler=True, use_graph=graph)
        assert got.cpu().tolist() == greedy, graph


def _step_logits(lm, x, mask, ids):
    """The host-driven loop of ``sample_generate`` fed with given ids: the logits [B, V] every step's choice was made from."""
    B, S, H = x.shape
    hidden, kstart, pos = lm.prefill(x, mask, lm.kv_capacity(S + ids.shape[1]))
    row, hid, out = hidden[:, -1, :], torch.empty(B, H, device=lm.device, dtype=BF16), []
    for step in range(ids.shape[1]):
        out.append(lm.logits(row).cpu())
        ops.embed_gather(ids[:, step].to(device=lm.device, dtype=torch.int32).contiguous(), lm.embed, out=hid)
        lm.forward(hid, B, 1, pos, torch.full((B,), S + step, device=lm.device, dtype=torch.int32), kstart, ctx=S + step + 1)
        pos, row = pos + 1, hid
    return out


def test_sampling_with_injected_uniforms_follows_the_spec(tiny_model, prompts, uniforms, free_run):
    """Every id of the device loop lies in the fp64 interval of its uniform (test_gpu_sampler's criterion and tolerance) under the
    spec applied to that step's logits, which the host-driven loop reproduces from the ids.  Same uniforms, same ids -- eager and
    replayed; under ``torch.manual_seed`` without injected uniforms the run is repeatable."""
    lm = tiny_model[0].decoder.lm
    x, mask = prompts[1]
    ids = free_run
    assert ids.shape == (2, 8)
    u = uniforms.cpu().double()
    for step, lg in enumerate(_step_logits(lm, x, mask, ids)):
        q = sampling.reference_probs(lg, history=ids[:, :step], temperature=0.9, top_p=0.95, top_k=50, dtype=torch.float64)
        lo, hi = sampling.reference_intervals(q)
        t = ids[:, step, None]
        lo_t, hi_t = lo.gather(1, t)[:, 0], hi.gather(1, t)[:, 0]
        print(f"step {step}: ids {t[:, 0].tolist()}, u {u[step].tolist()}, intervals {lo_t.tolist()} .. {hi_t.tolist()}")
        assert bool((q.gather(1, t) > 0).all()), step
        assert bool(((u[step] >= lo_t - DRAW_TOL) & (u[step] <= hi_t + DRAW_TOL)).all()), step
    assert ids.unique().numel() > 4                          # it did sample
    for graph in (False, True):
        again = lm.sample_generate(x, mask, 8, eos_id=-1, pad_id=PAD, device_sampler=True, uniforms=uniforms, use_graph=graph,
                                   **SAMPLING)
        assert torch.equal(again.cpu(), ids), graph
    runs = []
    for _ in range(2):
        torch.manual_seed(3)
        runs.append(lm.sample_generate(x, mask, 8, device_sampler=True, **SAMPLING).cpu())
    assert torch.equal(runs[0], runs[1])


def test_minimum_length_keeps_eos_out(tiny_model, prompts, uniforms, free_run):
    """The first token the free run draws for row 0 is declared EOS: with min_len = 3 the same uniforms must not produce it in the
    first three tokens; with min_len = 0 they do, at once."""
    lm = tiny_model[0].decoder.lm
    x, mask = prompts[1]
    eos = int(free_run[0, 0])
    for graph in (False, True):
        got = lm.sample_generate(x, mask, 8, min_len=3, eos_id=eos, pad_id=PAD, device_sampler=True, uniforms=uniforms,
                                 use_graph=graph, **SAMPLING).cpu()
        assert got.shape[1] >= 3 and not bool((got[:, :3] == eos).any()), graph
    got = lm.sample_generate(x, mask, 8, min_len=0, eos_id=eos, pad_id=PAD, device_sampler=True, uniforms=uniforms, **SAMPLING).cpu()
    assert int(got[0, 0]) == eos and bool((got[0, 1:] == PAD).all())


def test_eos_padding_width_and_poll_interval(tiny_model, prompts, uniforms, free_run, monkeypatch):
    """Rows never interact and the uniforms go by step, so with token T declared EOS the result must be the free run with PAD after
    each row's first T, cut one past the last step at which a row was unfinished -- ``apply_eos_padding``, the host path's rule.
    The interval of the host's look at the flags changes nothing."""
    lm = tiny_model[0].decoder.lm
    x, mask = prompts[1]
    first = lambda t: [(free_run[r] == t).nonzero()[0, 0].item() if bool((free_run[r] == t).any()) else 99 for r in range(2)]
    both = [int(t) for t in free_run[0, 1:] if first(int(t))[0] != first(int(t))[1] and max(first(int(t))) < 8]
    cases = [int(free_run[0, 2])] + both[:1]                 # row 0 ends early, row 1 runs on; and, if there is one, a T both rows draw
    for eos in cases:
        want = llama.apply_eos_padding(free_run, eos, PAD)
        for poll in (2, 16, 100):
            monkeypatch.setattr(llama, "EOS_POLL", poll)
            for graph in (False, True):
                got = lm.sample_generate(x, mask, 8, min_len=0, eos_id=eos, pad_id=PAD, device_sampler=True, uniforms=uniforms,
                                         use_graph=graph, **SAMPLING).cpu()     # min_len = 0: T is never suppressed, as in the free run
                assert got.tolist() == want.tolist(), (eos, poll, graph)
        assert bool((want[0] == PAD).any())
    # every row done early: the width shrinks (a token both rows draw at step 0 under u = 0 for both)
    u0 = torch.zeros_like(uniforms)
    t0 = lm.sample_generate(x, mask, 8, eos_id=-1, pad_id=PAD, device_sampler=True, uniforms=u0, **SAMPLING).cpu()
    if int(t0[0, 0]) == int(t0[1, 0]):
        monkeypatch.setattr(llama, "EOS_POLL", 2)
        got = lm.sample_generate(x, mask, 8, min_len=0, eos_id=int(t0[0, 0]), pad_id=PAD, device_sampler=True, uniforms=u0, **SAMPLING)
        assert got.shape == (2, 1)


def test_model_option_and_environment_reach_the_device_loop(tiny_model, monkeypatch):
    from emu_amd import EmuModel, TextDecoderCfg
    m, z = tiny_model
    ids, mask, img = _t(z["ids1"]), _t(z["mask1"]), _t(z["image"]).cuda()
    calls = []
    real = llama.LlamaEngine._sample_device
    monkeypatch.setattr(llama.LlamaEngine, "_sample_device", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
    # neither set: what the parent computes, the host loop under torch's generator
    assert m.device_sampler is False
    torch.manual_seed(3)
    a = m.generate_ids(ids, mask, img, max_new_tokens=8, **SAMPLING)
    x = m._prompt_embeds(ids, img, m.n_query).view(1, ids.shape[1], -1)
    torch.manual_seed(3)
    b = m.decoder.lm.sample_generate(x, mask, 8, device_sampler=False, **SAMPLING)
    assert torch.equal(a, b) and not calls
    monkeypatch.setattr(m, "device_sampler", True)
    assert m.generate_ids(ids, mask, img, max_new_tokens=8, do_sample=True, top_k=1).cpu().tolist() == z["new1"].tolist()
    assert len(calls) == 1
    m.generate_ids(ids, mask, img, max_new_tokens=4, do_sample=True, top_k=5, no_repeat_ngram_size=2)      # keeps the host loop
    m.generate_ids(ids, mask, img, max_new_tokens=4, do_sample=True, num_beams=2, hf_semantics="5.x")      # beam sampling: as before
    assert len(calls) == 1
    v, l, vocab, W = tiny.weights_from(z)
    monkeypatch.setenv("EMU_DEVICE_SAMPLER", "1")
    assert EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda", ctx=m.ctx).device_sampler is True
    monkeypatch.delenv("EMU_DEVICE_SAMPLER")
    assert EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda", ctx=m.ctx).device_sampler is False
