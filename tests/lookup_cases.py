"""Shared by the lookup tests: the CPU screen of a prompt (plain greedy search through tests/fake_engine.py, fp32 arithmetic on the
model's bf16 weights, with every step's top-2 logit margin) and the draft tables that force a given acceptance."""
import torch

from oracle import emu2_ref as R
from tests.fake_engine import FakeEngine

MARGIN = 0.08                  # the project's divergence threshold (tests/test_gpu_fp4_gemm.py)


def cpu_greedy(l, vocab, W, rcfg, embeds, mask, max_new, min_len, eos):
    """Plain greedy search of one prompt on the CPU stand-in -> (ids up to and including the first EOS, the smallest top-2 logit
    margin of the steps that produced them).  EOS is suppressed at indices below min_len, as greedy_generate suppresses it."""
    eng = FakeEngine(l, vocab, W, rcfg)
    h, kstart, pos = eng.prefill(embeds.float(), mask, 64 + embeds.shape[1])
    S = embeds.shape[1]
    row, ids, margin = h[:, -1, :], [], float("inf")
    for i in range(max_new):
        lg = eng.logits(row)[0].clone()
        if i < min_len:
            lg[eos] = -float("inf")
        t2 = lg.topk(2)
        margin = min(margin, float(t2.values[0] - t2.values[1]))
        ids.append(int(t2.indices[0]))
        if ids[-1] == eos or i + 1 == max_new:
            break
        x = R.embed_tokens(torch.tensor([[ids[-1]]]), W)[:, 0].float().clone()
        row = eng.forward(x, 1, 1, pos + i, torch.tensor([S + i]), kstart, S + i + 1)
    return ids, margin


def forced_drafts(g, k, max_new, right, vocab):
    """[max_new, k] int32: row s guesses the greedy ids g[s], g[s + 1], .. right for its first ``right`` entries and wrong (the id
    plus one) from there on; behind the end of g the guess is wrong by construction (nothing is there to accept)."""
    d = torch.zeros(max_new, k, dtype=torch.int32)
    for s in range(max_new):
        for j in range(k):
            gid = g[s + j] if s + j < len(g) else 0
            d[s, j] = gid if j < right and s + j < len(g) else (gid + 1) % vocab
    return d


def greedy_rows(g):
    """``speculate.simulate``'s model for a prompt whose greedy ids are g: row i emits g[step + i] for as long as the ids fed up to
    it are the greedy ones (behind a wrong id the arg-max is unknown -- and never consulted: acceptance stops in front of it)."""
    def rows(fed, step):
        out = []
        for i in range(len(fed)):
            ok = all(step + j - 1 < len(g) and fed[j] == g[step + j - 1] for j in range(1, i + 1))
            out.append(g[step + i] if ok and step + i < len(g) else -1)
        return out
    return rows
