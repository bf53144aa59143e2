"""GPU tests of the one-launch beam-search step (csrc/beam.hip, emu_beam_step_bf16) against the host step of
emu_amd.llama.beam_search_generate -- ``llama.beam_host_scores``, the stable top-2N, ``sampling.beam_scorer_step``: the statements the
host loop itself runs -- which restates transformers' vectorised beam search and is itself pinned to the real reference's ids
(tests/test_host_logic.py, tests/test_gpu_model.py).  Run on an MI355X with `-m gpu`."""
import pytest
import torch

from emu_amd import sampling
from emu_amd.llama import beam_host_scores
from tests.beam_step_common import BeamBuffers, assert_beam_state

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def torch_step(st, lp_rows, cur, min_len, max_len, length_penalty, eos_id, v431=False):
    """One iteration of the host loop (emu_amd/llama.py::beam_search_generate, deterministic branch) on a state of
    ``sampling.beam_start_state``: its scores, the top-2N with ties to the lower index (the kernel's rule; torch.topk leaves the order
    of ties unspecified, and ties are the rule here, not the exception: bf16 logits take few distinct values, and every entry that
    carries the -1e9 offset is the same fp32 number), its bookkeeping.  v431: the scorer conventions of transformers 4.31
    (hf_semantics="4.31")."""
    B, nb, V = lp_rows.shape
    acc = beam_host_scores(lp_rows, st["running_scores"], st["running_seq"], cur, min_len, eos_id)
    top_lp, top_idx = sampling.beam_reference_select(acc, nb, None, False)
    return sampling.beam_scorer_step(st, top_lp, top_idx, V, cur, max_len, length_penalty, eos_id, v431)[:2]


@pytest.mark.parametrize("v431", [False, True])
@pytest.mark.parametrize("B,nb,V,max_len,min_len,lp,eos_boost", [
    (1, 5, 32274, 10, 1, -1.0, 0.0),           # the reference's defaults
    (2, 5, 32274, 12, 1, -1.0, 6.0),           # EOS often among the best: results finish, the heuristic closes
    (3, 3, 1000, 8, 4, 1.0, 8.0),              # min_length masks EOS for four steps; positive length penalty
    (2, 8, 4096, 6, 1, 0.0, 5.0),              # 8 beams, length_penalty 0 (Emu1's captions)
    (1, 2, 64, 5, 1, -1.0, 3.0),               # tiny vocabulary
])
def test_beam_step_kernel_equals_the_torch_pipeline(B, nb, V, max_len, min_len, lp, eos_boost, v431):
    """Random bf16 logits (exact ties included: bf16 takes few values), the EOS logit raised so that finished hypotheses, the merge
    with the kept results and the early-stopping heuristic all happen: after every step the kernel's state -- running and kept
    sequences, both score sets, finished flags, lengths, the heuristic flag -- and its outputs (tokens to feed, cache rows to
    continue) equal the torch pipeline's under the same tie rule, for both scorer conventions (hf431 = 0: transformers 5.x, 1: the
    4.31 the reference pins).  Scores are compared to 1e-4 (the log-sum-exp is summed in another order; a near-tie closer than that
    between two beams could legitimately flip -- none does on these seeds).  Under v431 the step index comes from a DEVICE counter
    (the hipGraph-replay form of the call), and a call beyond the length limit must leave every piece of state untouched."""
    from emu_amd import ops
    from emu_amd._lib import lib, check
    dev = torch.device("cuda", 0)
    eos = 2
    g = torch.Generator().manual_seed(B * 1000 + nb * 10 + max_len)
    ref = sampling.beam_start_state(B, nb, max_len, 32000, dev)
    k = BeamBuffers(ref, dev)
    L = lib()
    ws = torch.empty(L.emu_beam_step_workspace_bytes(B, nb, V), dtype=torch.uint8, device=dev)

    def call(cur):
        check(L.emu_beam_step_bf16(*k.step_args(lg.data_ptr(), ld_prompt, ld_beam, V, cur, min_len, eos, lp, v431, ws, counter=v431),
                                   ops.stream(dev)), "emu_beam_step_bf16")

    for cur in range(max_len):
        if cur == 0:
            lg = (torch.randn(B, V, generator=g) * 3.0).to(BF16).to(dev)
            lg[:, eos] += eos_boost
            lp_rows = lg.float()[:, None, :].expand(B, nb, V)
            ld_prompt, ld_beam = lg.stride(0), 0
        else:
            lg = (torch.randn(B * nb, V, generator=g) * 3.0).to(BF16).to(dev)
            lg[:, eos] += eos_boost
            lp_rows = lg.float().view(B, nb, V)
            ld_prompt, ld_beam = nb * lg.stride(0), lg.stride(0)
        toks, flat = torch_step(ref, lp_rows, cur, min_len, max_len, lp, eos, v431)
        call(cur)
        torch.cuda.synchronize()
        assert_beam_state(k, ref, toks, flat, f"step {cur}")
    assert bool(ref["finished"].any())                                       # the scenario did finish hypotheses
    if v431:                                                                 # a replay beyond the limit is a no-op
        snap = [t_.clone() for t_ in k.state()]
        call(max_len)
        torch.cuda.synchronize()
        assert all(torch.equal(a_, b_) for a_, b_ in zip(snap, k.state()))


def test_beam_step_rejects_shapes_outside_its_range():
    from emu_amd import ops
    from emu_amd._lib import lib
    dev = torch.device("cuda", 0)
    z = torch.zeros(1 << 18, device=dev)
    lg = torch.zeros(1, 64, dtype=BF16, device=dev)
    p = z.data_ptr()
    for nb, L_, cur, V in ((9, 8, 0, 64), (2, 300, 0, 64), (2, 8, 8, 64), (5, 8, 0, 8)):
        st = lib().emu_beam_step_bf16(lg.data_ptr(), 64, 0, V, 1, nb, L_, cur, None, 0, 2, 1.0, 0, p, p, p, p, p, p, p, p, p, p, 1 << 20,
                                      ops.stream(dev))
        assert st == -22, (nb, L_, cur, V, st)
