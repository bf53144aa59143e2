"""Inputs shared by tests/test_sampling_host.py (CPU) and tests/test_gpu_sampler.py: seeded bf16 logit rows, the option sets, and
the seeds chosen by screening on the CPU (``python -m tests.sampler_cases`` prints the table below).

Screened property, asserted again by the tests on every use (``check_screen``): for every row, the group of tokens at the top-p
threshold value has ONE member (so the specification's whole-group rule and transformers' sort keep the same set), and the top-p
decision is at least ``MARGIN`` of probability mass away from its bound at every distinct score (so no fp32 summation order can flip
it: the kernel's and torch's sums are good to a few 1e-6).  Gaussian rows at a small scale never pass at V = 32 274 -- dozens of
tokens share every bf16 value near the threshold -- so the scale grows with the vocabulary until the threshold lies in the sparse
upper tail.
"""
import torch

from emu_amd import sampling

ROWS = 5
MARGIN = 1e-4
VOCABS = (97, 1000, 4099, 32274)
SCALE = {97: 3.0, 1000: 4.0, 4099: 6.0, 32274: 16.0}
SUPPRESS = 2


def history(V):
    """Ids generated so far, per row: duplicates, an id >= V (ignored), and one row with no usable id."""
    rows = [[5, 5, 17, V - 1, 5, V + 3], [0, 1, 1, 96, 40, 40], [V + 3] * 6, [7, 7, 7, 7, 7, 7], [3, 9, 27, 81, 2, 6]]
    return torch.tensor(rows, dtype=torch.int64)


# name -> options of sampling.reference_probs ("history" is filled in per vocabulary)
CASES = {
    "k1": dict(top_k=1),
    "k50": dict(top_k=50),
    "kV10": dict(top_k=-10),                               # top_k = V + 10, resolved in options()
    "p005": dict(top_p=0.05),
    "p09": dict(top_p=0.9),
    "p1": dict(top_p=1.0),
    "both": dict(top_k=50, top_p=0.9),
    "mk2": dict(top_p=1e-4, min_keep=2),                   # top_p so small that only min_keep survive
    "t07": dict(temperature=0.7, top_p=0.9),
    "t10": dict(temperature=1.0, top_k=50, top_p=0.95),
    "t20": dict(temperature=2.0, top_p=0.9),
    "pen": dict(repetition_penalty=1.3, top_p=0.9, history=True),
    "sup": dict(suppress_id=SUPPRESS, top_k=50, top_p=0.9),
}

# (V, case) -> seed, from `python -m tests.sampler_cases`
SEEDS = {
    (97, 'k1'): 1, (97, 'k50'): 1, (97, 'kV10'): 1, (97, 'p005'): 1, (97, 'p09'): 1, (97, 'p1'): 1, (97, 'both'): 1, (97, 'mk2'): 1,
    (97, 't07'): 1, (97, 't10'): 1, (97, 't20'): 1, (97, 'pen'): 2, (97, 'sup'): 1,
    (1000, 'k1'): 1, (1000, 'k50'): 1, (1000, 'kV10'): 1, (1000, 'p005'): 1, (1000, 'p09'): 2, (1000, 'p1'): 1, (1000, 'both'): 3,
    (1000, 'mk2'): 2, (1000, 't07'): 3, (1000, 't10'): 18, (1000, 't20'): 2, (1000, 'pen'): 2, (1000, 'sup'): 3,
    (4099, 'k1'): 1, (4099, 'k50'): 1, (4099, 'kV10'): 1, (4099, 'p005'): 1, (4099, 'p09'): 3, (4099, 'p1'): 1, (4099, 'both'): 3,
    (4099, 'mk2'): 2, (4099, 't07'): 1, (4099, 't10'): 3, (4099, 't20'): 3, (4099, 'pen'): 3, (4099, 'sup'): 3,
    (32274, 'k1'): 1, (32274, 'k50'): 1, (32274, 'kV10'): 1, (32274, 'p005'): 1, (32274, 'p09'): 1, (32274, 'p1'): 1,
    (32274, 'both'): 1, (32274, 'mk2'): 2, (32274, 't07'): 1, (32274, 't10'): 1, (32274, 't20'): 2, (32274, 'pen'): 1,
    (32274, 'sup'): 1,
}


def options(V, name):
    o = dict(CASES[name])
    if o.get("top_k") == -10:
        o["top_k"] = V + 10
    if o.pop("history", False):
        o["history"] = history(V)
    return o


def rows(V, seed, n=ROWS, mul=1.0):
    g = torch.Generator().manual_seed(int(seed))
    return (torch.randn(n, V, generator=g) * (SCALE[V] * mul)).to(torch.bfloat16)


def scale_mul(V, name):
    """Temperature 2 halves every score: those rows are drawn 2.5 times wider, or the threshold falls among the tied many.  A case
    without a top-p cut keeps the narrow scale at every V: there the whole row stays, and at the wide scale its low end would
    underflow fp32 (a token is then 'removed' by rounding alone, which is not what these cases are about)."""
    if CASES[name].get("top_p", 1.0) >= 1.0:
        return 3.0 / SCALE[V]
    return 2.5 if name == "t20" else 1.0


def check_screen(logits, opts):
    group, margin = sampling.top_p_threshold_group(logits, **opts)
    return bool((group == 1).all()) and float(margin.min()) >= MARGIN


def case(V, name):
    """(logits [ROWS, V] bf16, options) of a screened case; asserts the screened property."""
    x, o = rows(V, SEEDS[(V, name)], mul=scale_mul(V, name)), options(V, name)
    assert check_screen(x, o), f"inputs of case {(V, name)} lost the screened property"
    return x, o


if __name__ == "__main__":
    for V in VOCABS:
        for name in CASES:
            seed = next(s for s in range(1, 2000) if check_screen(rows(V, s, mul=scale_mul(V, name)), options(V, name)))
            print(f"    ({V}, {name!r}): {seed},", flush=True)
