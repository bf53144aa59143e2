"""CPU: ``sampling.beam_scorer_step`` against a record of the statements it was extracted from.  tests/golden/beam_scorer_steps.npz
holds, for six multi-step searches under both scorer conventions, every step's candidates (the stable top-2N of the host loop's scores)
and the state, tokens and cache rows after it, as the hand-written step of tests/test_gpu_beam.py computed them on the CPU at the
commit before the extraction (the snippet and the hash: profiles/beam_host_step_refactor_equivalence.md).  Same inputs, same torch ops
in the same order: nothing less than bit equality is expected."""
import os

import numpy as np
import pytest
import torch

from emu_amd import sampling

EOS, PAD = 2, 32000
KEYS = ("running_seq", "sequences", "running_scores", "beam_scores", "finished", "seq_len", "open")


@pytest.fixture(scope="module")
def record(golden_dir):
    return np.load(os.path.join(golden_dir, "beam_scorer_steps.npz"))


def _replay(z, i, v431):
    """Feed scenario i's recorded candidates to the step; torch.equal on every recorded tensor after every step.  Returns (did a
    hypothesis finish, the first step after which a prompt's heuristic was closed or None)."""
    B, nb, V, L, _, lp, _ = z["scenarios"][i].tolist()
    B, nb, V, L = int(B), int(nb), int(V), int(L)
    rec = {k: torch.from_numpy(z[f"s{i}_v{int(v431)}_{k}"]) for k in KEYS + ("top_lp", "top_idx", "toks", "flat")}
    st = sampling.beam_start_state(B, nb, L, PAD)
    closed = None
    for cur in range(L):
        toks, flat, _, _ = sampling.beam_scorer_step(st, rec["top_lp"][cur], rec["top_idx"][cur], V, cur, L, lp, EOS, v431)
        for k in KEYS:
            assert st[k].dtype == rec[k].dtype and torch.equal(st[k], rec[k][cur]), (i, v431, cur, k)
        assert torch.equal(toks, rec["toks"][cur]) and torch.equal(flat, rec["flat"][cur]), (i, v431, cur)
        if closed is None and not bool(st["open"].all()):
            closed = cur
    return bool(st["finished"].any()), closed, L


@pytest.mark.parametrize("v431", [False, True])
def test_scorer_step_reproduces_the_recorded_steps_bit_for_bit(record, v431):
    n = len(record["scenarios"])
    assert n == 6
    runs = [_replay(record, i, v431) for i in range(n)]
    assert all(fin for fin, _, _ in runs)                                     # every scenario finishes hypotheses
    early = [i for i, (_, closed, L) in enumerate(runs) if closed is not None and closed < L - 1]
    assert early, runs                                                        # the heuristic closes ahead of the limit somewhere
