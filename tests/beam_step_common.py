"""What the GPU tests of the beam-step kernels share (tests/test_gpu_beam.py, test_gpu_beam_sampler.py, test_gpu_constrain.py,
test_gpu_ngram.py): the device buffers of a step with the argument list every ``emu_beam_*step*_bf16`` entry point begins with, and
the comparison of a kernel's state with the specification's (``emu_amd.sampling.beam_scorer_step`` on a ``beam_start_state``)."""
import torch


class BeamBuffers:
    """The device copy of a host state ``st`` (``sampling.beam_start_state``, or a search under way) in the kernels' types, the two
    outputs ``tok`` / ``flat`` (pre-filled with ``fill``) and a device step counter."""

    def __init__(self, st, device="cuda", fill=0):
        d = lambda t, dt: t.to(dt).to(device).contiguous()
        self.B, self.nb, self.L = st["running_seq"].shape
        self.run, self.seq = d(st["running_seq"], torch.int32), d(st["sequences"], torch.int32)
        self.rs, self.bs = d(st["running_scores"], torch.float32), d(st["beam_scores"], torch.float32)
        self.fin, self.len = d(st["finished"], torch.uint8), d(st["seq_len"], torch.int32)
        self.open = d(st["open"].view(-1), torch.uint8)
        self.tok = torch.full((self.B * self.nb,), fill, dtype=torch.int32, device=device)
        self.flat = torch.full((self.B * self.nb,), fill, dtype=torch.int64, device=device)
        self.cur_dev = torch.zeros(1, dtype=torch.int32, device=device)

    def state(self):
        return (self.run, self.seq, self.rs, self.bs, self.fin, self.len, self.open, self.tok, self.flat)

    def step_args(self, lg_ptr, ld_prompt, ld_beam, V, cur, min_len, eos, lp, hf431, ws, counter=False, override=None):
        """The 24 leading arguments of a beam-step entry point for step ``cur``: from the host, or (``counter``) from the device
        counter with -7 in the host's place.  ``override``: B, nb, L, run, ws, ws_bytes as the call should see them."""
        self.cur_dev.fill_(cur)
        a = dict(B=self.B, nb=self.nb, L=self.L, run=self.run.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel())
        a.update(override or {})
        return (lg_ptr, ld_prompt, ld_beam, V, a["B"], a["nb"], a["L"], -7 if counter else cur,
                self.cur_dev.data_ptr() if counter else None, min_len, eos, lp, int(hf431), a["run"],
                *[t.data_ptr() for t in self.state()[1:]], a["ws"], a["ws_bytes"])


def logit_strides(lg, B, nb):
    """(ld_prompt, ld_beam) of logits [B, V] (step 0: the beams share the prompt's row) or [B * nb, V]."""
    return (lg.stride(0), 0) if lg.shape[0] == B else (nb * lg.stride(0), lg.stride(0))


def assert_beam_state(bufs, ref, toks, flat, what):
    """The kernel's state and outputs (``bufs.state()``) against the specification's state ``ref`` and outputs ``toks`` / ``flat``:
    sequences, tokens, cache rows, flags, lengths and the heuristic flag equal; both score sets free of NaN, live (above -1e8: entries
    at -1e9 are compared as such) and -inf in the same places, the live values within 1e-4."""
    k_run, k_seq, k_rs, k_bs, k_fin, k_len, k_open, k_tok, k_flat = [t.cpu() for t in bufs.state()]
    ref = {k: v.cpu() for k, v in ref.items()}
    assert k_run.long().tolist() == ref["running_seq"].tolist(), what
    assert k_seq.long().tolist() == ref["sequences"].tolist(), what
    assert k_tok.long().tolist() == toks.tolist() and k_flat.tolist() == flat.tolist(), what
    assert k_fin.bool().tolist() == ref["finished"].tolist() and k_len.long().tolist() == ref["seq_len"].tolist(), what
    assert k_open.bool().tolist() == ref["open"].view(-1).tolist(), what
    for a_, b_ in ((k_rs, ref["running_scores"]), (k_bs, ref["beam_scores"])):
        assert not bool(torch.isnan(a_).any()), what
        live = b_ > -1.0e8
        assert torch.equal(a_ > -1.0e8, live) and torch.equal(torch.isinf(a_), torch.isinf(b_)), what
        if bool(live.any()):
            assert float((a_[live] - b_[live]).abs().max()) < 1e-4, what
