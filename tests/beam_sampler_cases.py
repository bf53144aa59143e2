"""Inputs shared by tests/test_beam_sampling_host.py (CPU) and tests/test_gpu_beam_sampler.py: seeded bf16 logit rows for the beams
of a few prompts, their histories and running scores, the option sets, and the seeds chosen by screening on the CPU
(``python -m tests.beam_sampler_cases`` prints the table below; ``--record FILE`` writes the ids of the host loop's multinomial path
for ``PARENT_SETS``, which is how tests/golden/beam_sample_parent_ids.npz was made on the commit before the table of uniforms).

Screened property, asserted again by the tests on every use (``check_screen``), the one of tests/sampler_cases.py on the rows the
warpers act on (``sampling.beam_reference_warp_input``: the penalised log-probabilities, under the "4.31" order with the running score
added): the group of tokens at the top-p threshold value has ONE member, and the top-p decision is at least ``MARGIN`` of probability
mass away from its bound at every distinct score.
"""
import sys

import torch

from emu_amd import sampling

MARGIN = 1e-4
EOS = 2
SCALE = {64: 3.0, 1000: 4.0, 4099: 6.0, 32274: 16.0}
ORDERS = ("5.x", "4.31")
CPU_SHAPES = [(2, nb, V) for V in (64, 1000, 4099) for nb in (2, 3, 5)]
# less than a wave's stride; not a multiple of 8; prime and more than 4 per thread; the model's own vocabulary
GPU_SHAPES = [(1, 2, 64), (3, 3, 1000), (2, 8, 4099), (1, 5, 32274), (2, 5, 32274)]

# name -> options of sampling.beam_reference_rows ("history" is filled in per shape; "suppress_eos" = cur < min_len)
CASES = {
    "demo": dict(temperature=0.7, top_k=3, top_p=0.9, repetition_penalty=1.2, history=True),     # the demo backend's call
    "k50p": dict(top_k=50, top_p=0.9),
    "p09": dict(top_p=0.9),
    "t20pen": dict(temperature=2.0, top_p=0.95, repetition_penalty=1.3, history=True),
    "sup": dict(top_k=10, top_p=0.9, suppress_eos=True),
    "plain": dict(),                                                                              # no warper removes anything
}


def history(rows, V):
    """Ids generated so far, per beam row: duplicates, an id >= V (ignored), and one row with no usable id."""
    base = [[5, 5, 17, V - 1, 5, V + 3], [0, 1, 1, 33, 40, 40], [V + 3] * 6, [7, 7, 7, 7, 7, 7], [3, 9, 27, 61, 2, 6]]
    return torch.tensor([base[r % len(base)] for r in range(rows)], dtype=torch.int64)


def running_scores(B, nb, order):
    """Prompt 0: the start of a search ("5.x": 0 and -1e9 for the other beams; "4.31" sampling starts every beam at 0); the other
    prompts: scores of a search under way."""
    mid = torch.tensor([-1.25, -2.875, -0.5, -5.0625, -3.375, -4.5, -2.0, -6.125])
    rs = torch.stack([mid[:nb] - 0.75 * b for b in range(B)])
    rs[0] = 0.0
    if order == "5.x":
        rs[0, 1:] = -1.0e9
    return rs


def options(B, nb, V, name):
    o = dict(CASES[name])
    o["eos_id"] = EOS
    o.setdefault("suppress_eos", False)
    if o.pop("history", False):
        o["history"] = history(B * nb, V)
    return o


def scale_mul(V, name):
    """As in tests/sampler_cases.py: temperature 2 halves every score, so those rows are drawn wider; a case without a top-p cut keeps
    the narrow scale at every V (at the wide one the low end of the row would underflow fp32)."""
    if CASES[name].get("top_p", 1.0) >= 1.0:
        return 3.0 / SCALE[V]
    return 2.5 if name == "t20pen" else 1.0


def rows(B, nb, V, seed, mul=1.0):
    g = torch.Generator().manual_seed(int(seed))
    return (torch.randn(B * nb, V, generator=g) * (SCALE[V] * mul)).to(torch.bfloat16)


def check_screen(logits, rs, opts, order):
    w = sampling.beam_reference_warp_input(logits, rs.reshape(-1), opts.get("history"), opts.get("repetition_penalty", 1.0),
                                           opts["eos_id"], opts["suppress_eos"], order)
    group, margin = sampling.top_p_threshold_group(w, temperature=opts.get("temperature"), top_k=opts.get("top_k"),
                                                   top_p=opts.get("top_p"), min_keep=sampling.BEAM_MIN_KEEP)
    return bool((group == 1).all()) and float(margin.min()) >= MARGIN


# (B, nb, V, case, order) -> seed, from `python -m tests.beam_sampler_cases`
SEEDS = {
    (1, 2, 64, 'demo', '5.x'): 1, (1, 2, 64, 'demo', '4.31'): 1, (1, 2, 64, 'k50p', '5.x'): 1,
    (1, 2, 64, 'k50p', '4.31'): 1, (1, 2, 64, 'p09', '5.x'): 1, (1, 2, 64, 'p09', '4.31'): 1,
    (1, 2, 64, 't20pen', '5.x'): 1, (1, 2, 64, 't20pen', '4.31'): 1, (1, 2, 64, 'sup', '5.x'): 1,
    (1, 2, 64, 'sup', '4.31'): 1, (1, 2, 64, 'plain', '5.x'): 1, (1, 2, 64, 'plain', '4.31'): 1,
    (1, 5, 32274, 'demo', '5.x'): 2, (1, 5, 32274, 'demo', '4.31'): 2, (1, 5, 32274, 'k50p', '5.x'): 2,
    (1, 5, 32274, 'k50p', '4.31'): 2, (1, 5, 32274, 'p09', '5.x'): 2, (1, 5, 32274, 'p09', '4.31'): 2,
    (1, 5, 32274, 't20pen', '5.x'): 9, (1, 5, 32274, 't20pen', '4.31'): 9, (1, 5, 32274, 'sup', '5.x'): 2,
    (1, 5, 32274, 'sup', '4.31'): 2, (1, 5, 32274, 'plain', '5.x'): 1, (1, 5, 32274, 'plain', '4.31'): 1,
    (2, 2, 64, 'demo', '5.x'): 1, (2, 2, 64, 'demo', '4.31'): 1, (2, 2, 64, 'k50p', '5.x'): 1,
    (2, 2, 64, 'k50p', '4.31'): 1, (2, 2, 64, 'p09', '5.x'): 1, (2, 2, 64, 'p09', '4.31'): 1,
    (2, 2, 64, 't20pen', '5.x'): 1, (2, 2, 64, 't20pen', '4.31'): 1, (2, 2, 64, 'sup', '5.x'): 1,
    (2, 2, 64, 'sup', '4.31'): 1, (2, 2, 64, 'plain', '5.x'): 1, (2, 2, 64, 'plain', '4.31'): 1,
    (2, 2, 1000, 'demo', '5.x'): 2, (2, 2, 1000, 'demo', '4.31'): 2, (2, 2, 1000, 'k50p', '5.x'): 3,
    (2, 2, 1000, 'k50p', '4.31'): 3, (2, 2, 1000, 'p09', '5.x'): 2, (2, 2, 1000, 'p09', '4.31'): 2,
    (2, 2, 1000, 't20pen', '5.x'): 2, (2, 2, 1000, 't20pen', '4.31'): 2, (2, 2, 1000, 'sup', '5.x'): 2,
    (2, 2, 1000, 'sup', '4.31'): 2, (2, 2, 1000, 'plain', '5.x'): 1, (2, 2, 1000, 'plain', '4.31'): 1,
    (2, 2, 4099, 'demo', '5.x'): 2, (2, 2, 4099, 'demo', '4.31'): 2, (2, 2, 4099, 'k50p', '5.x'): 3,
    (2, 2, 4099, 'k50p', '4.31'): 3, (2, 2, 4099, 'p09', '5.x'): 3, (2, 2, 4099, 'p09', '4.31'): 3,
    (2, 2, 4099, 't20pen', '5.x'): 3, (2, 2, 4099, 't20pen', '4.31'): 3, (2, 2, 4099, 'sup', '5.x'): 1,
    (2, 2, 4099, 'sup', '4.31'): 1, (2, 2, 4099, 'plain', '5.x'): 1, (2, 2, 4099, 'plain', '4.31'): 1,
    (2, 3, 64, 'demo', '5.x'): 1, (2, 3, 64, 'demo', '4.31'): 1, (2, 3, 64, 'k50p', '5.x'): 1,
    (2, 3, 64, 'k50p', '4.31'): 1, (2, 3, 64, 'p09', '5.x'): 1, (2, 3, 64, 'p09', '4.31'): 1,
    (2, 3, 64, 't20pen', '5.x'): 1, (2, 3, 64, 't20pen', '4.31'): 1, (2, 3, 64, 'sup', '5.x'): 1,
    (2, 3, 64, 'sup', '4.31'): 1, (2, 3, 64, 'plain', '5.x'): 1, (2, 3, 64, 'plain', '4.31'): 1,
    (2, 3, 1000, 'demo', '5.x'): 2, (2, 3, 1000, 'demo', '4.31'): 2, (2, 3, 1000, 'k50p', '5.x'): 3,
    (2, 3, 1000, 'k50p', '4.31'): 3, (2, 3, 1000, 'p09', '5.x'): 2, (2, 3, 1000, 'p09', '4.31'): 2,
    (2, 3, 1000, 't20pen', '5.x'): 6, (2, 3, 1000, 't20pen', '4.31'): 6, (2, 3, 1000, 'sup', '5.x'): 8,
    (2, 3, 1000, 'sup', '4.31'): 8, (2, 3, 1000, 'plain', '5.x'): 1, (2, 3, 1000, 'plain', '4.31'): 1,
    (2, 3, 4099, 'demo', '5.x'): 2, (2, 3, 4099, 'demo', '4.31'): 2, (2, 3, 4099, 'k50p', '5.x'): 3,
    (2, 3, 4099, 'k50p', '4.31'): 3, (2, 3, 4099, 'p09', '5.x'): 3, (2, 3, 4099, 'p09', '4.31'): 3,
    (2, 3, 4099, 't20pen', '5.x'): 3, (2, 3, 4099, 't20pen', '4.31'): 3, (2, 3, 4099, 'sup', '5.x'): 2,
    (2, 3, 4099, 'sup', '4.31'): 2, (2, 3, 4099, 'plain', '5.x'): 1, (2, 3, 4099, 'plain', '4.31'): 1,
    (2, 5, 64, 'demo', '5.x'): 1, (2, 5, 64, 'demo', '4.31'): 1, (2, 5, 64, 'k50p', '5.x'): 1,
    (2, 5, 64, 'k50p', '4.31'): 1, (2, 5, 64, 'p09', '5.x'): 1, (2, 5, 64, 'p09', '4.31'): 1,
    (2, 5, 64, 't20pen', '5.x'): 1, (2, 5, 64, 't20pen', '4.31'): 1, (2, 5, 64, 'sup', '5.x'): 1,
    (2, 5, 64, 'sup', '4.31'): 1, (2, 5, 64, 'plain', '5.x'): 1, (2, 5, 64, 'plain', '4.31'): 1,
    (2, 5, 1000, 'demo', '5.x'): 2, (2, 5, 1000, 'demo', '4.31'): 2, (2, 5, 1000, 'k50p', '5.x'): 280,
    (2, 5, 1000, 'k50p', '4.31'): 280, (2, 5, 1000, 'p09', '5.x'): 12, (2, 5, 1000, 'p09', '4.31'): 12,
    (2, 5, 1000, 't20pen', '5.x'): 74, (2, 5, 1000, 't20pen', '4.31'): 74, (2, 5, 1000, 'sup', '5.x'): 8,
    (2, 5, 1000, 'sup', '4.31'): 8, (2, 5, 1000, 'plain', '5.x'): 1, (2, 5, 1000, 'plain', '4.31'): 1,
    (2, 5, 4099, 'demo', '5.x'): 2, (2, 5, 4099, 'demo', '4.31'): 2, (2, 5, 4099, 'k50p', '5.x'): 88,
    (2, 5, 4099, 'k50p', '4.31'): 88, (2, 5, 4099, 'p09', '5.x'): 32, (2, 5, 4099, 'p09', '4.31'): 32,
    (2, 5, 4099, 't20pen', '5.x'): 4, (2, 5, 4099, 't20pen', '4.31'): 4, (2, 5, 4099, 'sup', '5.x'): 2,
    (2, 5, 4099, 'sup', '4.31'): 2, (2, 5, 4099, 'plain', '5.x'): 1, (2, 5, 4099, 'plain', '4.31'): 1,
    (2, 5, 32274, 'demo', '5.x'): 2, (2, 5, 32274, 'demo', '4.31'): 2, (2, 5, 32274, 'k50p', '5.x'): 2,
    (2, 5, 32274, 'k50p', '4.31'): 2, (2, 5, 32274, 'p09', '5.x'): 2, (2, 5, 32274, 'p09', '4.31'): 2,
    (2, 5, 32274, 't20pen', '5.x'): 9, (2, 5, 32274, 't20pen', '4.31'): 9, (2, 5, 32274, 'sup', '5.x'): 2,
    (2, 5, 32274, 'sup', '4.31'): 2, (2, 5, 32274, 'plain', '5.x'): 1, (2, 5, 32274, 'plain', '4.31'): 1,
    (2, 8, 4099, 'demo', '5.x'): 10, (2, 8, 4099, 'demo', '4.31'): 10, (2, 8, 4099, 'k50p', '5.x'): 248,
    (2, 8, 4099, 'k50p', '4.31'): 248, (2, 8, 4099, 'p09', '5.x'): 147, (2, 8, 4099, 'p09', '4.31'): 147,
    (2, 8, 4099, 't20pen', '5.x'): 159, (2, 8, 4099, 't20pen', '4.31'): 159, (2, 8, 4099, 'sup', '5.x'): 22,
    (2, 8, 4099, 'sup', '4.31'): 22, (2, 8, 4099, 'plain', '5.x'): 1, (2, 8, 4099, 'plain', '4.31'): 1,
    (3, 3, 1000, 'demo', '5.x'): 2, (3, 3, 1000, 'demo', '4.31'): 2, (3, 3, 1000, 'k50p', '5.x'): 181,
    (3, 3, 1000, 'k50p', '4.31'): 181, (3, 3, 1000, 'p09', '5.x'): 12, (3, 3, 1000, 'p09', '4.31'): 12,
    (3, 3, 1000, 't20pen', '5.x'): 14, (3, 3, 1000, 't20pen', '4.31'): 14, (3, 3, 1000, 'sup', '5.x'): 8,
    (3, 3, 1000, 'sup', '4.31'): 8, (3, 3, 1000, 'plain', '5.x'): 1, (3, 3, 1000, 'plain', '4.31'): 1,
}


def case(B, nb, V, name, order):
    """(logits [B * nb, V] bf16, running scores [B, nb], options) of a screened case; asserts the screened property."""
    x, rs, o = rows(B, nb, V, SEEDS[(B, nb, V, name, order)], mul=scale_mul(V, name)), running_scores(B, nb, order), options(B, nb, V, name)
    assert check_screen(x, rs, o, order), f"inputs of case {(B, nb, V, name, order)} lost the screened property"
    return x, rs, o


# ---- the host loop on the tiny model: the calls whose ids the commit before the table of uniforms returns (uniforms=None must
# still return them), and the tables under which the host loop's draws keep their distance from every boundary
PARENT_SETS = {
    "demo431": dict(num_beams=3, max_new_tokens=6, do_sample=True, temperature=0.7, top_k=3, top_p=0.9, repetition_penalty=1.2,
                    hf_semantics="4.31", length_penalty=1.0),
    "wide5x": dict(num_beams=3, max_new_tokens=6, do_sample=True, temperature=0.7, top_k=40, top_p=0.9, hf_semantics="5.x"),
}
PARENT_SEED = 99


def record_parent_ids(run, path):
    """``run(name, options)`` -> ids of ``beam_search_generate`` under ``torch.manual_seed(PARENT_SEED)`` with exactly these
    keywords (the ones the function had before ``uniforms``)."""
    import numpy as np
    out = {}
    for name, o in PARENT_SETS.items():
        torch.manual_seed(PARENT_SEED)
        out[name] = run(name, dict(o)).cpu().numpy()
    np.savez(path, **out)


def fake_engine_run(golden_dir):
    """The host loop through tests/fake_engine.py on the prompts of generate_beam_sample_tiny.npz (CPU, fp32 arithmetic)."""
    import numpy as np
    from emu_amd import llama as L, ops
    from oracle import emu2_ref as R
    from tests import tiny
    from tests.fake_engine import FakeEngine
    z = tiny.load(golden_dir, "generate_beam_sample_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    cfg = tiny.oracle_cfg(v, l, vocab)
    L.BF16 = torch.float32
    ops.embed_gather = lambda ids, table, out=None: out.copy_(table[ids.long()])
    ids, mask = torch.from_numpy(np.asarray(z["ids"])), torch.from_numpy(np.asarray(z["mask"]))
    x = R.embed_tokens(ids, W)

    def run(name, o, **extra):
        nb, n_new = o.pop("num_beams"), o.pop("max_new_tokens")
        return L.LlamaEngine.beam_search_generate(FakeEngine(l, vocab, W, cfg.llama), x, mask, nb, n_new, **o, **extra)
    return run


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--record":
        import os
        record_parent_ids(fake_engine_run(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")), sys.argv[2])
        sys.exit(0)
    for shape in sorted(set(CPU_SHAPES + GPU_SHAPES)):
        for name in CASES:
            for order in ORDERS:
                B, nb, V = shape
                seed = next(s for s in range(1, 2000) if check_screen(rows(B, nb, V, s, mul=scale_mul(V, name)),
                                                                      running_scores(B, nb, order), options(B, nb, V, name), order))
                print(f"    ({B}, {nb}, {V}, {name!r}, {order!r}): {seed},", flush=True)
