"""LLaMA decoder engine: host side of the ``emu_llama_*`` C ABI.

Plays the role of ``transformers.LlamaForCausalLM`` inside the reference's ``EmuForClsAndRegression``
(Emu2/emu/lm.py:30-40) for the calls the hot path makes: ``lm.model.embed_tokens`` (emu.py:119,193),
``lm.model(inputs_embeds=...)`` (emu.py:133-138) and greedy ``lm.generate`` (emu.py:213-229).
All arithmetic runs in libemu_hip.so; torch only owns the memory.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import time
from typing import Dict, Iterable, Optional, Tuple

import torch

from . import bf16pack, genroute, mxfp4, ops, speculate
from ._lib import SAMPLE_MAX_VOCAB, Bf16Pack12SetC, Bf16PackSetC, EmuHipError, LlamaCfgC, SampleParamsC, check, lib
from .conf.emu_conf import LlamaCfg
from .constrain import TokenTrie
from .device_loop import CapturedStep, run_polled, warn_once
from .sampling import beam_draw_margin, beam_reference_select, beam_scorer_step, beam_start_state, beam_topk
from .scoring import IGNORE_INDEX, shared_prefix_plan, split_segments
from .tp import ShardPlan

BF16 = torch.bfloat16
EOS_POLL = 16          # greedy decode: steps between two host looks at the emitted ids (early stop on EOS)
_LAYER_KEYS = ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight",
               "self_attn.o_proj.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight",
               "input_layernorm.weight", "post_attention_layernorm.weight")


def rope_tables(head_dim: int, max_pos: int, theta: float, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos/sin [max_pos, D] bf16 exactly as transformers' LlamaRotaryEmbedding builds them (fp32 math, cast)."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim))
    freqs = torch.arange(max_pos, dtype=torch.float32)[:, None] * inv[None, :]
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().to(BF16).to(device).contiguous(), emb.sin().to(BF16).to(device).contiguous()


class EmuHipContext:
    """One per (process, device): owns the emu_ctx handle and, for tp_size > 1, the RCCL communicator.  One process drives
    one GPU: creating the context makes its device the process's current device (explicitly, here and nowhere else --
    ``ops.stream`` refuses operands of another device instead of switching to it)."""

    def __init__(self, device: torch.device, tp_rank: int = 0, tp_size: int = 1):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("emu_amd needs a GPU device (no CPU path)")
        if self.device.index is not None and self.device.index != torch.cuda.current_device():
            torch.cuda.set_device(self.device)
        self.tp_rank, self.tp_size = tp_rank, tp_size
        self.p2p = False
        self.p2p_fence_free = False
        h = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        check(lib().emu_ctx_create(idx, tp_rank, tp_size, C.byref(h)), "emu_ctx_create")
        self.handle = h

    def init_tp(self, broadcast_bytes, force: bool = False, allgather_bytes=None, rccl: bool = True,
                p2p_timeout_ms: int = 0) -> None:
        """Create the RCCL communicator.  ``broadcast_bytes(b: bytes|None) -> bytes`` must return rank 0's
        128-byte unique id on every rank (e.g. via the torch.distributed store).  ``force`` creates a communicator
        even for tp_size 1 (a 1-rank RCCL all-reduce: used to exercise the RCCL + hipGraph path on a single GPU).

        ``allgather_bytes(b: bytes) -> list[bytes]`` (every rank's bytes, in rank order) additionally sets up the one-shot
        peer-to-peer all-reduce for the decode-sized messages (csrc/p2p.hip): IPC handles are exchanged, every rank runs a
        self-test, and the path is enabled only if it passed on ALL ranks -- otherwise the all-reduces stay on RCCL and
        ``self.p2p`` is False.  ``rccl=False`` skips the communicator (ranks sharing one GPU in the tests, which RCCL
        refuses); the P2P path is then mandatory."""
        if self.tp_size == 1 and not force:
            return
        if rccl:
            buf = (C.c_char * 128)()
            if self.tp_rank == 0:
                check(lib().emu_tp_unique_id(buf), "emu_tp_unique_id")
                uid = broadcast_bytes(bytes(buf))
            else:
                uid = broadcast_bytes(None)
            buf = (C.c_char * 128).from_buffer_copy(uid)
            with torch.cuda.device(self.device):
                check(lib().emu_tp_init(self.handle, buf), "emu_tp_init", self.handle)
        if allgather_bytes is not None:
            self.p2p = self._init_p2p(allgather_bytes, p2p_timeout_ms)
        if not rccl and not self.p2p:
            raise RuntimeError("tensor parallelism without RCCL needs the peer-to-peer all-reduce, and its self-test failed")

    def _init_p2p(self, allgather_bytes, timeout_ms: int) -> bool:
        L = lib()
        h = (C.c_char * 64)()
        ok = L.emu_tp_p2p_create(self.handle, h) == 0
        handles = allgather_bytes(bytes(h) if ok else b"")
        if not all(len(x) == 64 for x in handles):           # some rank could not export: nobody maps anything
            return False
        ok = L.emu_tp_p2p_open(self.handle, (C.c_char * (64 * self.tp_size)).from_buffer_copy(b"".join(handles)), timeout_ms) == 0
        ok = all(x == b"1" for x in allgather_bytes(b"1" if ok else b"0"))   # also the barrier: every peer block is mapped
        if ok:
            # self-test: four all-reduces (both slots, one reuse each) of rank-dependent vectors; exact in bf16
            n = 6656
            base = torch.arange(n, device=self.device, dtype=torch.float32) % 13
            want = sum(base * (r + 1) + r for r in range(self.tp_size)).to(BF16)
            s = ops.stream(self.device)
            for it in range(4):
                x = (base * (self.tp_rank + 1) + self.tp_rank).to(BF16)
                ok = ok and L.emu_tp_p2p_allreduce_bf16(self.handle, x.data_ptr(), n, s) == 0
                torch.cuda.synchronize(self.device)
                ok = ok and bool(torch.equal(x, want))
            ok = ok and L.emu_tp_p2p_giveups() == 0
        ok = all(x == b"1" for x in allgather_bytes(b"1" if ok else b"0"))
        if ok:
            # the self-test above ran the FENCED form (system-scope release / acquire: the memory model's guarantee).  The fence-free
            # form (3.3 instead of 6.8 us per decode all-reduce) rests on write-through + acknowledgement behaviour instead, so it is
            # switched on only after a soak of it passed on EVERY rank of this very job (real xGMI links where the ranks have their
            # own GPUs); EMU_P2P_FENCE_FREE=0 keeps the fenced form, =1 skips the soak (tools on one GPU).
            want_ff = os.environ.get("EMU_P2P_FENCE_FREE", "auto")
            ff = want_ff == "1"
            if want_ff == "auto":
                check(L.emu_tp_p2p_set_fenced(self.handle, 0), "emu_tp_p2p_set_fenced", self.handle)
                ff = self._soak_p2p()
                ff = all(x == b"1" for x in allgather_bytes(b"1" if ff else b"0"))
                if not ff and self.tp_rank == 0:
                    import warnings
                    warnings.warn("fence-free peer-to-peer all-reduce failed its soak; keeping the fenced form")
            check(L.emu_tp_p2p_set_fenced(self.handle, 0 if ff else 1), "emu_tp_p2p_set_fenced", self.handle)
            self.p2p_fence_free = ff
            check(L.emu_tp_p2p_enable(self.handle, 1), "emu_tp_p2p_enable", self.handle)
        elif self.tp_rank == 0:
            import warnings
            warnings.warn("peer-to-peer all-reduce self-test failed; tensor-parallel all-reduces stay on RCCL")
        return ok

    def _soak_p2p(self, iters: int = 384) -> bool:
        """Back-to-back all-reduces of sequence- and rank-dependent vectors in the CURRENT form of the exchange, one host
        synchronisation at the end, every word of every result checked against the closed form (small integers: exact in bf16).
        Both slots are reused ~190 times each with no host gap between uses -- the window in which a late write-through or a
        stale read would surface -- and two slot-sized (256 KiB) messages exercise all 32 pieces."""
        L, n, dev = lib(), 6656, self.device
        i = torch.arange(n, device=dev, dtype=torch.int64)
        k = torch.arange(iters, device=dev, dtype=torch.int64)[:, None]
        val = lambda r: ((i * 7 + k * 3 + r * 5) % 16).to(torch.float32)
        x = val(self.tp_rank).to(BF16).contiguous()
        want = sum(val(r) for r in range(self.tp_size)).to(BF16)
        s = ops.stream(dev)
        ok = True
        for j in range(iters):
            ok = ok and L.emu_tp_p2p_allreduce_bf16(self.handle, x[j].data_ptr(), n, s) == 0
        nb = 128 * 1024
        ib = torch.arange(nb, device=dev, dtype=torch.int64)
        big = [((ib * 3 + j + self.tp_rank * 11) % 8).to(BF16) for j in range(2)]
        for j in range(2):
            ok = ok and L.emu_tp_p2p_allreduce_bf16(self.handle, big[j].data_ptr(), nb, s) == 0
        torch.cuda.synchronize(dev)
        ok = ok and bool(torch.equal(x, want))
        for j in range(2):
            ok = ok and bool(torch.equal(big[j], sum(((ib * 3 + j + r * 11) % 8).to(torch.float32) for r in range(self.tp_size)).to(BF16)))
        return ok and L.emu_tp_p2p_giveups() == 0

    def check_p2p(self) -> None:
        """Raise if a device-side wait of the P2P all-reduce ever timed out (the sums since then are invalid)."""
        if self.p2p and lib().emu_tp_p2p_giveups() != 0:
            # the path cannot recover (its per-piece sequence counters have diverged across the ranks): leave it for good, so
            # that whatever this process runs next goes through RCCL (where a communicator exists) instead of summing stale slots
            self.p2p = False
            lib().emu_tp_p2p_enable(self.handle, 0)
            raise RuntimeError("peer-to-peer all-reduce timed out waiting for a peer rank; the results of this generation are invalid "
                               "(the peer-to-peer path is now switched off for this process)")

    def allreduce(self, t: torch.Tensor) -> torch.Tensor:
        check(lib().emu_allreduce_bf16(self.handle, t.data_ptr(), t.numel(), ops.stream(self.device)), "emu_allreduce_bf16", self.handle)
        return t

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                lib().emu_ctx_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class LlamaEngine:
    # the weight mode as the setters below left it (defaults of the class, so that every engine has them before any setter ran)
    fp8_decode = fp8_wide = False      # use_fp8(True[, wide=True]): 1..2 [and 3..16] rows stream the fp8 set
    fp8_mid = False            # use_fp8(True, wide=True, mid=True) is on: steps of 17..64 rows stream the fp8 set too
    fp8_all = False            # use_fp8(True, wide=True, mid=True, all_rows=True) is on: every row count runs the fp8 set
    fp4_decode = fp4_wide = False      # use_fp4(True[, wide=True]): the same row ranges on the MXFP4 set
    fp4_all = False            # use_fp4(True, wide=True, all_rows=True) is on: every row count runs the 4-bit set
    bf16_released = False      # release_bf16() was called: the bf16 matrices and lm_head are gone, fp4_all / fp8_all is pinned
    bf16_pack_on = bf16_pack_wide = False      # use_bf16_pack / use_bf16_pack_wide: the 13-bit packed streams at 1 / 4..16 rows

    def __init__(self, cfg: LlamaCfg, vocab: int, ctx: EmuHipContext):
        self.cfg, self.vocab, self.ctx = cfg, vocab, ctx
        self.device = ctx.device
        self.plan = ShardPlan(cfg.hidden_size, cfg.num_attention_heads, cfg.head_dim, cfg.intermediate_size,
                              ctx.tp_size, ctx.tp_rank)
        c = LlamaCfgC(cfg.hidden_size, self.plan.heads_local, cfg.head_dim, self.plan.ffn_local,
                      cfg.num_hidden_layers, vocab, cfg.max_position_embeddings, cfg.rms_norm_eps)
        h = C.c_void_p()
        check(lib().emu_llama_create(ctx.handle, C.byref(c), C.byref(h)), "emu_llama_create", ctx.handle)
        self.handle = h
        # prefill() always hands the rows of a prompt over in slot order, which is what the fused RoPE / KV-append / V^T epilogue of
        # the qkv projection needs to be told (include/emu_hip.h: emu_llama_set_prefill_fusion); set_prefill_fusion(False) = the
        # three-launch sequence (A/B timing, parity tests)
        self.set_prefill_fusion(True)
        self._keep: Dict[str, torch.Tensor] = {}          # packed weights (owned here, pointers held by the lib)
        self._pending: Dict[int, Dict[str, torch.Tensor]] = {}
        self.layers_loaded = set()          # indices of the packed layers (a reload must not count twice)
        self.cos, self.sin = rope_tables(cfg.head_dim, cfg.max_position_embeddings, cfg.rope_theta, self.device)
        self.embed = self.final_norm = self.lm_head = None
        self.head_rows = None                               # (row0, row1) of the vocabulary this rank's lm_head holds under TP
        self.kcache = self.vcache = None
        self.kv_batch = self.s_max = 0
        self._ws = None
        # every captured decode graph (GreedyState, beam search, EmuModel's regress loop) carries the epoch it was captured under in
        # its key: a mode switch (fp8 weights, decode tail, fused layers) bumps it, so no graph of another mode is ever replayed
        self.mode_epoch = 0
        # whole decoder layers per launch (csrc/decode_layer.hip): built, bit-identical, and measured SLOWER than the launches on
        # MI355X (12.45 vs 10.57 ms per token at TP = 1, 3.95 vs 3.57 for a TP = 8 shard: profiles/r05_decode_fused_*.log), so it
        # is an option (EMU_DECODE_FUSED=1|2 or set_decode_fused), off by default
        self.decode_fused = 0
        if os.environ.get("EMU_L2_WARM") and hasattr(lib(), "emu_llama_set_l2_warm"):      # A/B aid: the warm mask of this engine
            self.set_l2_warm(int(os.environ["EMU_L2_WARM"], 0))
        mode = int(os.environ.get("EMU_DECODE_FUSED", "0"))
        if mode:
            self.set_decode_fused(mode)
        # tensor parallelism: the two-lane prefill (prompts of >= N rows run as two row halves whose all-reduces travel behind the
        # other half's GEMMs, emu_llama_set_tp_overlap) is OPT-IN: EMU_TP_OVERLAP=N (e.g. 1024) or set_tp_overlap(N).  What it costs
        # is measured (+17...21 % per rank under graph replay, +40...47 % eager, profiles/r05_tp_prefill_two_lane_per_rank_cost.log);
        # what it hides is an estimate until a multi-GPU node has run it (bench.py --tp-prefill-leg collects that evidence), and it
        # issues RCCL all-reduces of one communicator from two streams, which no run has exercised against a real ring.
        self.tp_overlap_rows = 0
        if ctx.tp_size > 1 and int(os.environ.get("EMU_TP_OVERLAP", "0")) > 0:
            self.set_tp_overlap(int(os.environ["EMU_TP_OVERLAP"]))

    def _mode_changed(self) -> None:
        self.mode_epoch += 1
        self._drop_loop_states()

    def _drop_loop_states(self) -> None:
        """Forget every cached loop state (``_loop_state``): its buffers, and a graph that holds pointers into a cache or a mode
        that is gone.  (The keys hold the epoch and the cache pointer, so a stale graph is never replayed; this frees it.)"""
        self.__dict__.setdefault("_loop_states", {}).clear()          # loop name -> (key, state)

    def _loop_state(self, name: str, key: tuple, rows: int, build) -> dict:
        """The cached state of the device loop ``name`` ("beam", "contrastive") for ``key``, or a new one: ``build()``'s buffers, the
        decoder step's workspace ``fws`` for ``rows`` rows and ``captured``, the ``CapturedStep`` of the loop's body.  ``key`` must
        hold everything that body reads besides the state."""
        states = self.__dict__.setdefault("_loop_states", {})
        if name not in states or states[name][0] != key:
            states.pop(name, None)                          # one signature at a time: its buffers are a few MB, its graph ~430 nodes
            st = build()
            # the decoder step's workspace: owned here, because the pointers a captured graph holds must outlive any re-allocation
            # of the engine's shared workspace by a later, larger call
            need = max(int(lib().emu_llama_workspace_bytes(self.handle, rows, 1)), rows * self.cfg.hidden_size * 2)
            st["fws"] = torch.empty(need, dtype=torch.uint8, device=self.device)
            st["captured"] = CapturedStep()
            states[name] = (key, st)
        return states[name][1]

    def set_l2_warm(self, mask: int) -> None:
        """L2 warming across the launch boundaries of the default one-row decode step (include/emu_hip.h: emu_llama_set_l2_warm):
        bits 0-4 = combine -> o_proj, o_proj -> gate/up, gate/up -> down, down -> next qkv / lm_head, qkv -> K/V rows; bit 5 = first
        trips instead of whole blocks; bits 8-15 = budget in MiB.  Same bits whatever the mask.  Invalidates captured decode graphs."""
        check(lib().emu_llama_set_l2_warm(self.handle, int(mask)), "emu_llama_set_l2_warm", self.ctx.handle)
        self._mode_changed()

    def l2_warm_count(self) -> int:
        """Launches that carried a non-empty warm plan since the engine was created (tests)."""
        return int(lib().emu_llama_l2_warm_count(self.handle))

    def set_decode_tail(self, enable: bool) -> None:
        """Decode attention in one launch (the last split workgroup of a head merges the splits) or, the default, with the separate
        combine launch.  Same bits; measured 0.4 % slower in one launch.  Invalidates captured decode graphs."""
        check(lib().emu_llama_set_decode_tail(self.handle, 1 if enable else 0), "emu_llama_set_decode_tail", self.ctx.handle)
        self._mode_changed()

    def set_decode_fused(self, enable: int, layers_per_launch: int = 0) -> None:
        """One-row decode steps (greedy decode, ``generate_image``'s regress loop) with bf16 weights run whole decoder layers per
        launch (csrc/decode_layer.hip: ``layers_per_launch`` layers, 0 = all) instead of six launches + two all-reduces per layer;
        bit-identical to the launches.  Under tensor parallelism 1 = cut at the all-reduces (four launches per layer), 2 = all-reduces
        inside the launch over the P2P comm blocks (one GPU per rank), 3 = stand-alone launches whose last workgroup runs the
        all-reduce in its tail (attention, o_proj, down_proj as single-role launches: five per layer, safe on a shared device);
        4 = the persistent weight-streaming engine (csrc/decode_engine.hip: the attention launches, then ONE launch per layer for
        o_proj -> all-reduce -> gate/up -> down -> all-reduce -> the next layer's qkv; tensor-parallel shards with rows of at most
        13 KiB, i.e. TP >= 4, over the P2P comm blocks, one GPU per rank; anything else silently keeps the launches).  OFF by default:
        every mode measured slower than the launches (see __init__; EMU_DECODE_FUSED=<mode> in the environment switches one on).
        Invalidates captured decode graphs."""
        check(lib().emu_llama_set_decode_fused(self.handle, int(enable), int(layers_per_launch)), "emu_llama_set_decode_fused",
              self.ctx.handle)
        self.decode_fused = int(enable)
        self._mode_changed()

    def decode_fused_stats(self) -> Tuple[int, int]:
        """(give-ups of the fused path's bounded waits -- non-zero means garbage was computed --, forwards that took the fused path)."""
        g, f = C.c_uint(0), C.c_long(0)
        check(lib().emu_llama_decode_fused_stats(self.handle, C.byref(g), C.byref(f)), "emu_llama_decode_fused_stats", self.ctx.handle)
        return int(g.value), int(f.value)

    def check_decode_fused(self) -> None:
        g, _ = self.decode_fused_stats()
        if g:
            raise EmuHipError(f"fused decode layers: {g} in-kernel wait(s) ran into the time limit; the step's outputs are invalid")

    def set_tp_overlap(self, min_rows: int) -> None:
        """Tensor-parallel prefill of prompts with at least ``min_rows`` rows (B = 1; clamped up to 512) in two row halves: the
        all-reduce of one half's o_proj / down_proj partial sums runs on the context's second stream while this stream computes the
        other half's stage (include/emu_hip.h: emu_llama_set_tp_overlap).  0 = every all-reduce serially between the GEMMs.  Results
        agree with the serial schedule to bf16 rounding (a half may take another GEMM tile configuration)."""
        check(lib().emu_llama_set_tp_overlap(self.handle, int(min_rows)), "emu_llama_set_tp_overlap", self.ctx.handle)
        self.tp_overlap_rows = 0 if min_rows <= 0 else max(512, int(min_rows))

    def tp_overlap_count(self) -> int:
        """Forwards that took the two-half schedule."""
        return int(lib().emu_llama_tp_overlap_count(self.handle))

    def set_prefill_fusion(self, enable: bool) -> None:
        """Whether ``prefill`` promises the library slot-ordered rows (the fused RoPE / KV-append / V^T / norm epilogues).  The
        promise itself is per call (emu_llama_set_prefill_fusion is consumed by the next T > 1 forward): ``prefill`` renews it
        before every forward it issues; a direct ``forward`` call with rows in any other slot order never inherits it."""
        self.prefill_fusion = bool(enable)
        if not enable:
            check(lib().emu_llama_set_prefill_fusion(self.handle, 0), "emu_llama_set_prefill_fusion", self.ctx.handle)

    # ------------------------------------------------------------------ weights
    def _dev(self, t: torch.Tensor) -> torch.Tensor:
        return t.to(device=self.device, dtype=BF16).contiguous()

    def load_tensor(self, name: str, t: torch.Tensor) -> bool:
        """Consume one reference-named tensor (``model.layers.N...`` / ``model.embed_tokens.weight`` /
        ``model.norm.weight`` / ``lm_head.weight``, i.e. keys relative to ``decoder.lm.``). Returns True if used."""
        if name == "model.embed_tokens.weight":
            self.embed = self._dev(t)
        elif name == "model.norm.weight":
            self.final_norm = self._dev(t)
        elif name == "lm_head.weight":
            if self.ctx.tp_size > 1 and os.environ.get("EMU_TP_VOCAB_SHARD", "1") != "0":
                # vocabulary-sharded head: this rank keeps rows [r0, r1) only -- 4035 of 32 274 at TP = 8, 54 MB instead of
                # 430 MB of the token's byte budget; emu_llama_logits all-reduces the rows whole again (bit-identical logits)
                r0, r1 = self.plan.vocab_range(t.shape[0])
                self.lm_head = self._dev(t[r0:r1])
                self.head_rows = (r0, r1)
            else:
                self.lm_head = self._dev(t)
            self._drop_bf16_pack(["lm_head"])                  # (a reloaded matrix: its packed set is stale)
        elif name.startswith("model.layers."):
            rest = name[len("model.layers."):]
            idx, key = rest.split(".", 1)
            if key not in _LAYER_KEYS:
                return False                                   # e.g. rotary_emb.inv_freq buffers of old checkpoints
            d = self._pending.setdefault(int(idx), {})
            d[key] = t
            if len(d) == len(_LAYER_KEYS):
                self._pack_layer(int(idx), self._pending.pop(int(idx)))
        else:
            return False
        if self.embed is not None and self.final_norm is not None and self.lm_head is not None:
            check(lib().emu_llama_set_head(self.handle, self.final_norm.data_ptr(), self.lm_head.data_ptr(),
                                           self.embed.data_ptr(), self.cos.data_ptr(), self.sin.data_ptr()),
                  "emu_llama_set_head")
            if self.head_rows is not None:
                check(lib().emu_llama_set_head_shard(self.handle, self.head_rows[0], self.head_rows[1] - self.head_rows[0]),
                      "emu_llama_set_head_shard", self.ctx.handle)
        if self.ready:
            self._auto_pack_bf16()
        return True

    def _pack_layer(self, i: int, d: Dict[str, torch.Tensor]) -> None:
        g = lambda k: d[k].to(device=self.device, dtype=BF16)
        p = self.plan.pack_layer(g("self_attn.q_proj.weight"), g("self_attn.k_proj.weight"),
                                 g("self_attn.v_proj.weight"), g("self_attn.o_proj.weight"),
                                 g("mlp.gate_proj.weight"), g("mlp.up_proj.weight"), g("mlp.down_proj.weight"))
        self._drop_bf16_pack([f"{i}.{k}" for k in self._PACK_KINDS])       # (a reloaded layer: its packed sets are stale)
        p["ln1"] = self._dev(d["input_layernorm.weight"])
        p["ln2"] = self._dev(d["post_attention_layernorm.weight"])
        for k, v in p.items():
            self._keep[f"{i}.{k}"] = v
        check(lib().emu_llama_set_layer(self.handle, i, p["wqkv"].data_ptr(), p["wo"].data_ptr(), p["wgu"].data_ptr(),
                                        p["wdown"].data_ptr(), p["ln1"].data_ptr(), p["ln2"].data_ptr()),
              "emu_llama_set_layer")
        self.layers_loaded.add(i)

    def load_weights(self, items: Iterable[Tuple[str, torch.Tensor]], prefix: str = "decoder.lm.") -> None:
        for name, t in items:
            if name.startswith(prefix):
                self.load_tensor(name[len(prefix):], t)

    @property
    def ready(self) -> bool:
        return (len(self.layers_loaded) == self.cfg.num_hidden_layers and self.embed is not None
                and self.final_norm is not None and (self.lm_head is not None or self.bf16_released))

    def weight_bytes_per_token(self) -> int:
        """Algorithmic bytes one decode step of THIS shard must stream (all packed matrices once + lm_head)."""
        if self.bf16_released and self.fp8_all:      # only the fp8 tensors are left: one byte per weight
            return sum(q.numel() for q, _ in self._fp8.values())
        if self.bf16_released:          # only the 4-bit tensors are left: their shapes
            return sum(self._fp4_shape(k)[0] * mxfp4.bytes_per_row(self._fp4_shape(k)[1]) for k in self._fp4_keys())
        if self.fp4_decode:             # MXFP4: K/2 element bytes + K/32 scale bytes per row
            size = lambda v: v.shape[0] * mxfp4.bytes_per_row(v.shape[1])
        else:
            b = 1 if self.fp8_decode else 2
            size = lambda v: v.numel() * b
        # the 13-bit packed stream (use_bf16_pack): a matrix that has a set streams its planes and flag words instead
        pk = getattr(self, "_pack", {}) if self.bf16_pack_on and b == 2 and not self.fp4_decode else {}
        one = lambda k, v: self._set_bytes(pk[k]) if k in pk else size(v)
        per = sum(one(k, v) for k, v in self._keep.items() if k.split(".")[1] in ("wqkv", "wo", "wgu", "wdown"))
        return per + (one("lm_head", self.lm_head) if self.lm_head is not None else 0)

    # ------------------------------------------------------------------ the 13-bit lossless bf16 decode stream (on by default)
    _PACK_KINDS = {"wqkv": (1, ops.EPI_NONE), "wo": (0, ops.EPI_RESID), "wgu": (1, ops.EPI_SWIGLU), "wdown": (0, ops.EPI_RESID)}

    def _pack_keys(self):
        return [f"{i}.{k}" for i in range(self.cfg.num_hidden_layers) for k in self._PACK_KINDS] + ["lm_head"]

    def _pack_rows(self, key: str, tune: int, head_form: bool) -> int:
        """Rows per group of the packed set of ``key`` (the form the planner names for its one-row stream), 0 = the matrix stays bf16.
        The head form's matrices (sets of 4 rows, fused RMSNorm: qkv, gate/up, lm_head) get a set only when ``head_form`` asks for it:
        the engine by itself packs the two plain streams, ``pack_bf16_default`` adds these (profiles/bf16_pack_head8.md)."""
        w = self.lm_head if key == "lm_head" else self._keep[key]
        norm, epi = (1, ops.EPI_NONE) if key == "lm_head" else self._PACK_KINDS[key.split(".")[1]]
        N, K = w.shape
        rows = 0 if K % 32 else int(lib().emu_bf16_pack_rows(N, K, norm, epi, tune))
        return rows if rows == 2 or head_form else 0

    @staticmethod
    def _set_bytes(p) -> int:
        """Bytes one pass over a packed set streams: its planes, its flag words and (12 bits) its patch records."""
        return (bf16pack.packed_bytes12 if "patch" in p else bf16pack.packed_bytes)(*p["shape"], p["rows"])

    def _pack12_default(self) -> bool:
        """Whether the default packing may give a matrix a 12-bit set (``bf16pack.set_bits`` then decides matrix by matrix):
        EMU_BF16_PACK12=0 forces 13 bits everywhere, tensor-parallel shards keep the 13-bit sets (nothing at TP has been timed),
        EMU_BF16_PACK_WIDE=1 keeps them too (the request for the 13-bit few-row twin; =12 asks for the 12-bit one and keeps the 12-bit
        sets), and a library that predates the format has no packer for it."""
        return (os.environ.get("EMU_BF16_PACK12", "1") != "0" and os.environ.get("EMU_BF16_PACK_WIDE") != "1" and self.ctx.tp_size == 1
                and hasattr(lib(), "emu_bf16_pack12"))

    def _register_bf16_pack(self, keys) -> None:
        """Hand the sets of the layers / the head named in ``keys`` to the library: the 13-bit setter takes a layer's four entries
        (an empty one clears that matrix's set), then the 12-bit setter overrides the matrices that hold a 12-bit set."""
        pk = self.__dict__.setdefault("_pack", {})
        is12 = lambda k: "patch" in pk.get(k, ())
        for i in sorted({int(k.split(".")[0]) for k in keys if k != "lm_head"}):
            names = [f"{i}.{k}" for k in self._PACK_KINDS]
            sets = (Bf16PackSetC * 4)(*[ops.pack_set_c(pk.get(k)) for k in names])
            check(lib().emu_llama_set_layer_bf16_pack(self.handle, i, sets), "emu_llama_set_layer_bf16_pack", self.ctx.handle)
            if any(is12(k) for k in names):
                sets12 = (Bf16Pack12SetC * 4)(*[ops.pack12_set_c(pk.get(k)) for k in names])
                check(lib().emu_llama_set_layer_bf16_pack12(self.handle, i, sets12), "emu_llama_set_layer_bf16_pack12", self.ctx.handle)
        if "lm_head" in keys and self.lm_head is not None:
            if is12("lm_head"):
                one = ops.pack12_set_c(pk["lm_head"])
                check(lib().emu_llama_set_head_bf16_pack12(self.handle, C.byref(one), int(self.lm_head.shape[0])),
                      "emu_llama_set_head_bf16_pack12", self.ctx.handle)
            else:
                one = ops.pack_set_c(pk.get("lm_head"))
                check(lib().emu_llama_set_head_bf16_pack(self.handle, C.byref(one), int(self.lm_head.shape[0])),
                      "emu_llama_set_head_bf16_pack", self.ctx.handle)

    def _drop_bf16_pack(self, keys) -> None:
        pk = getattr(self, "_pack", None)
        hit = [k for k in keys if pk and k in pk]
        if hit:
            for k in hit:
                del pk[k]
            self._register_bf16_pack(hit)
            self._mode_changed()

    def _pack_one(self, w: torch.Tensor, kind: str, rows: int, bits12: bool):
        """The packed set of one matrix: 12 bits where ``bits12`` allows, the kind has a 12-bit twin (``bf16pack.PACK12_KINDS``) and
        ``bf16pack.set_bits`` picks it from the flagged share the 12-bit pack reports; else 13 bits.  One set per matrix."""
        if bits12 and kind in bf16pack.PACK12_KINDS:
            p = ops.pack12_bf16_rows(w, rows)
            if bf16pack.set_bits(p["flagged"], (w.shape[0] + rows - 1) // rows, rows, w.shape[1], True) == 12:
                return p
            del p
        return ops.pack_bf16_rows(w, rows)

    def pack_bf16(self, tune: int = 0, head_form: bool = False, bits12: bool = False) -> Tuple[int, int]:
        """Build and register the packed set (``emu_amd.bf16pack``) of every matrix whose one-row stream has a packed twin and
        that has none yet; ``tune``: the emu_gemm_tune mask the streams will run under; ``head_form``: also the matrices behind a fused
        RMSNorm (``_pack_rows``); ``bits12``: 12-bit sets where ``_pack_one`` picks them (the default packing asks for them), else 13
        bits.  Returns (matrices packed, bytes of their sets).  The bf16 matrices stay: prefill, steps of more rows and flagged row
        groups read them."""
        if not self.ready:
            raise RuntimeError("pack_bf16: load all weights first")
        if self.bf16_released:
            raise RuntimeError("pack_bf16: the bf16 weights were released (release_bf16); flagged row groups read them")
        pk = self.__dict__.setdefault("_pack", {})
        new, nbytes = [], 0
        for key in self._pack_keys():
            rows = 0 if key in pk else self._pack_rows(key, tune, head_form)
            if rows:
                pk[key] = self._pack_one(self.lm_head if key == "lm_head" else self._keep[key], key.split(".")[-1], rows, bits12)
                new.append(key)
                nbytes += self._set_bytes(pk[key])
        if new:
            self._register_bf16_pack(new)
            self._mode_changed()
        return len(new), nbytes

    def use_bf16_pack(self, enable: bool = True) -> None:
        """One-row decode steps on the bf16 kernels stream the packed sets (same bits, 13/16 of the bytes) or, off, the bf16 matrices
        (invalidates captured decode graphs).  Only matrices that ``pack_bf16`` gave a set are affected."""
        check(lib().emu_llama_use_bf16_pack(self.handle, 1 if enable else 0), "emu_llama_use_bf16_pack", self.ctx.handle)
        self.bf16_pack_on = bool(enable)
        self._mode_changed()

    def use_bf16_pack_wide(self, enable: bool = True, keep12: bool = False) -> None:
        """Steps of 4..16 rows (beam search, small batches, contrastive search, the lookup chunk step) stream the packed sets too,
        through the matrix-core twin of the bf16 few-row stream: same bits, 13/16 of the bytes.  Off by default
        (profiles/bf16_pack_wide.md); needs ``use_bf16_pack`` on.  Invalidates captured graphs.  Without ``keep12`` every 12-bit set
        is repacked to 13 bits first (the one-row steps then stream 13 bits too); with it the sets stay as they are and a matrix that
        holds a 12-bit set goes to the twin's 12-bit form (the library's switch value 2, profiles/bf16_pack12_wide.md): one resident
        set serves both the one-row and the few-row step.  Tensor-parallel shards hold 13-bit sets either way."""
        if enable and not self.bf16_released and not self.bf16_pack_on:
            raise RuntimeError("use_bf16_pack_wide: switch the packed stream on first (use_bf16_pack)")
        if enable and keep12 and not hasattr(lib(), "emu_linear_bf16pack12_thin"):
            raise RuntimeError("use_bf16_pack_wide: this library has no 12-bit few-row stream (keep12)")
        if enable and not keep12:
            self._repack_13()
        check(lib().emu_llama_use_bf16_pack_wide(self.handle, (2 if keep12 else 1) if enable else 0), "emu_llama_use_bf16_pack_wide",
              self.ctx.handle)
        self.bf16_pack_wide = bool(enable)
        self._mode_changed()

    def _repack_13(self) -> None:
        """``use_bf16_pack_wide`` without ``keep12``: give every matrix that holds a 12-bit set a 13-bit one in its place (the one-row
        steps then stream 13 bits too; a matrix holds one set).  Nothing to do where the sets are 13-bit already."""
        pk = getattr(self, "_pack", {})
        k12 = [k for k, v in pk.items() if "patch" in v]
        for k in k12:
            pk[k] = ops.pack_bf16_rows(self.lm_head if k == "lm_head" else self._keep[k], pk[k]["rows"])
        if k12:
            self._register_bf16_pack(k12)
            self._mode_changed()
            print(f"emu_amd: bf16 pack stream: {len(k12)} sets repacked from 12 to 13 bits per weight for the 4..16-row stream", file=sys.stderr)

    def _pack_wide_default(self) -> None:
        """EMU_BF16_PACK_WIDE=1 switches the few-row stream on where the default packing has switched the one-row stream on (on
        13-bit sets); =12 does so with ``keep12``, on the sets the default packing made."""
        want = os.environ.get("EMU_BF16_PACK_WIDE")
        if want == "1" and not self.bf16_pack_wide and hasattr(lib(), "emu_llama_use_bf16_pack_wide"):
            self.use_bf16_pack_wide(True)
        elif want == "12" and not self.bf16_pack_wide and hasattr(lib(), "emu_linear_bf16pack12_thin"):
            self.use_bf16_pack_wide(True, keep12=True)

    def _auto_pack_bf16(self) -> None:
        """The default: when the engine is ready, pack and switch the stream on -- unless EMU_BF16_PACK=0, the library predates the
        stream (a tools A/B run against an older build), no matrix has a packed twin (small models, tensor-parallel shards), or the
        sets would take more than half of the free device memory (the KV cache and the workspaces need the rest).  EMU_BF16_PACK=all
        packs the head-form matrices here too; a model's loader adds them by default (``pack_bf16_default``)."""
        if os.environ.get("EMU_BF16_PACK", "1") == "0" or self.bf16_released or not hasattr(lib(), "emu_llama_use_bf16_pack"):
            return
        pk = getattr(self, "_pack", {})
        head_form = os.environ.get("EMU_BF16_PACK") == "all"
        todo = [(k, self._pack_rows(k, 0, head_form)) for k in self._pack_keys() if k not in pk]
        need = sum(bf16pack.packed_bytes(*(self.lm_head if k == "lm_head" else self._keep[k]).shape, r) for k, r in todo if r)
        if not need:
            return
        free = torch.cuda.mem_get_info(self.device)[0]
        if 2 * need > free:
            print(f"emu_amd: bf16 pack stream off: its sets need {need / 2**30:.1f} GiB, {free / 2**30:.1f} GiB are free", file=sys.stderr)
            return
        t0 = time.time()
        n, nbytes = self.pack_bf16(head_form=head_form, bits12=self._pack12_default())
        torch.cuda.synchronize(self.device)
        self.use_bf16_pack(True)
        self._pack_wide_default()
        n12 = sum("patch" in v for v in self._pack.values())
        print(f"emu_amd: bf16 pack stream on: {n} matrices packed ({nbytes / 2**30:.2f} GiB) in {time.time() - t0:.2f} s; "
              f"{n12} of {len(self._pack)} sets at 12 bits per weight, the rest at 13", file=sys.stderr)

    def pack_bf16_default(self) -> str:
        """The model-level default (``EmuModel.load_weights`` / ``Emu.load_state_dict`` call it once the engine is ready): on top of
        what ``_auto_pack_bf16`` packed at load, the head-form matrices (qkv, gate/up, lm_head), whose packed twin of 8 rows per
        workgroup beats the bf16 kernel (profiles/bf16_pack_head8.md) -- where ``bf16pack.default_pack`` says "all".  Packs what is
        missing, so a second call packs nothing and a reloaded matrix (its stale set dropped) gets a fresh one.  Returns the rule's
        answer."""
        if not self.ready or not hasattr(lib(), "emu_llama_use_bf16_pack"):
            return "off"
        pk = getattr(self, "_pack", {})
        todo = [(k, self._pack_rows(k, 0, True)) for k in self._pack_keys() if k not in pk] if not self.bf16_released else []
        need = sum(bf16pack.packed_bytes(*(self.lm_head if k == "lm_head" else self._keep[k]).shape, r) for k, r in todo if r)
        free = torch.cuda.mem_get_info(self.device)[0] if need else 0
        rule = bf16pack.default_pack(os.environ.get("EMU_BF16_PACK"), self.ctx.tp_size, self.bf16_released, need, free)
        if rule != "all" or not need:
            if rule == "plain" and need and self.ctx.tp_size == 1 and os.environ.get("EMU_BF16_PACK") != "plain":
                print(f"emu_amd: bf16 pack stream: the head-form sets need {need / 2**30:.1f} GiB, {free / 2**30:.1f} GiB are free; "
                      "qkv, gate/up and lm_head stay bf16", file=sys.stderr)
            return rule
        t0 = time.time()
        n, nbytes = self.pack_bf16(head_form=True, bits12=self._pack12_default())
        torch.cuda.synchronize(self.device)
        self.use_bf16_pack(True)
        self._pack_wide_default()
        total = sum(self._set_bytes(v) for v in self._pack.values())
        n12 = sum("patch" in v for v in self._pack.values())
        print(f"emu_amd: bf16 pack stream on: {n} matrices packed ({nbytes / 2**30:.2f} GiB) in {time.time() - t0:.2f} s"
              f"; {len(self._pack)} matrices, {total / 2**30:.2f} GiB of sets in all, {n12} of them at 12 bits per weight", file=sys.stderr)
        return rule

    # ------------------------------------------------------------------ optional fp8 decode stream
    def quantize_fp8(self) -> None:
        """Build per-row-scaled e4m3fn copies of every packed matrix (+ lm_head) on the device and register them for the
        decode stream (B*T <= 2 rows).  Prefill keeps the bf16 weights, so both sets stay resident (288 GB HBM:
        33B bf16 + fp8 = 98 GB).  Not a reference feature (the reference is bf16 end to end); off unless enabled."""
        if not self.ready:
            raise RuntimeError("quantize_fp8: load all weights first")
        if self.bf16_released:
            raise RuntimeError("quantize_fp8: the bf16 weights were released (release_bf16); there is nothing left to quantise")
        self.__dict__.setdefault("_fp8", {})
        for key in self._fp4_keys():                               # (the same keys; whatever load_fp8 provided is kept)
            if key not in self._fp8:
                self._fp8[key] = ops.quantize_fp8_rows(self._fp4_source(key))
                self._fp8_register(key)

    def _fp8_register(self, key: str) -> None:
        """Hand the library the pointers of a layer once its four matrices are here (or of the head)."""
        if key == "lm_head":
            q, sc = self._fp8[key]
            check(lib().emu_llama_set_head_fp8(self.handle, q.data_ptr(), sc.data_ptr()), "emu_llama_set_head_fp8", self.ctx.handle)
            return
        i = key.split(".")[0]
        if all(f"{i}.{k}" in self._fp8 for k in self._FP4_KINDS):
            a = [t.data_ptr() for k in self._FP4_KINDS for t in self._fp8[f"{i}.{k}"]]
            check(lib().emu_llama_set_layer_fp8(self.handle, int(i), *a), "emu_llama_set_layer_fp8", self.ctx.handle)

    def load_fp8(self, key: str, q: torch.Tensor, scale: torch.Tensor) -> None:
        """Register externally prepared fp8 tensors (``ops.quantize_fp8_rows`` or any quantiser that writes e4m3fn bytes and one fp32
        scale per row) for ``"<layer>.wqkv|wo|wgu|wdown"`` or ``"lm_head"``: ``q`` uint8 [N, K], ``scale`` float32 [N] for the [N, K]
        packed bf16 matrix of this rank (the tensor-parallel shard; lm_head: the rows this rank holds).  A layer is registered once
        its four matrices are here; ``quantize_fp8`` fills in whatever was not loaded."""
        src = self._fp4_source(key)
        if src is None:
            raise RuntimeError(f"load_fp8({key!r}): load the bf16 weights first (their packed shapes define the fp8 shapes)")
        N, K = src.shape
        for name, t, dt, shape in (("q", q, torch.uint8, (N, K)), ("scale", scale, torch.float32, (N,))):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != shape:
                raise ValueError(f"load_fp8({key!r}): {name} must be {dt} {shape}, got "
                                 f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
        if self.fp8_decode:
            raise RuntimeError("load_fp8: switch the fp8 stream off first (use_fp8(False)); captured graphs hold the old pointers")
        self.__dict__.setdefault("_fp8", {})
        self._fp8[key] = (q.to(self.device).contiguous(), scale.to(self.device).contiguous())
        self._fp8_register(key)

    def use_fp8(self, enable: bool = True, prefill: bool = False, wide: bool = False, mid: bool = False, all_rows: bool = False) -> None:
        """Switch the decode stream between the bf16 and the fp8 weights (invalidates captured decode graphs).  The matrices are
        quantised on the device first (``quantize_fp8``).  Exclusive with ``use_fp4``.

        ``use_fp8(True)``: steps of B*T <= 2 rows (greedy / sampled decode) stream the fp8 set; everything else streams bf16.
        ``prefill=True`` also runs the prefill GEMMs (17 rows and more) W8A8 on the block-scaled fp8 MFMA (activations quantised per
        row).
        ``wide=True``: steps of 3..16 rows (the default 5-beam search, a batch of prompts, contrastive search, ``score(via="decode")``
        on a few candidates) stream the fp8 set as well, through the matrix-core kernel (csrc/gemv_fp8_thin.hip; weight-only: the
        activations stay bf16, as at 1..2 rows); needs hidden, heads_local * head_dim and ffn_local to be multiples of 256 (the
        library refuses otherwise and says why: every TP = 1 / 2 sharding of the 33B shapes runs, the TP = 4 / 8 shards do not).
        Without ``wide`` those steps stream bf16, as they always did.
        ``wide=True, mid=True``: steps of 17..64 rows (four prompts x five beams, contrastive search on a batch) stream the fp8 set
        too, through the W8A16 GEMM (csrc/gemm_fp8.hip; activations bf16; a prompt of 17..64 rows runs without the RoPE and RMSNorm
        epilogue fusions of the bf16 prefill).  Same width requirement as ``wide``; ``mid`` without ``wide`` is a ``ValueError``.
        Above 64 rows nothing changes without ``all_rows``: bf16, or the W8A8 GEMMs with ``prefill=True``.
        ``wide=True, mid=True, all_rows=True``: calls of 65 rows and more (a prompt, ``score(via="prefill")``, beams x batch) stay on
        the fp8 set too, through the 64 x 128 form of the W8A16 GEMM (csrc/gemm_fp8.hip; weight-only, bit-identical row by row to
        the 17..64-row form; the RoPE and RMSNorm epilogue fusions and the two-lane prefill are off).  With ``prefill=True`` the layer
        projections keep the faster W8A8 GEMMs there and only the head, which has none, runs the new form.  One generation then sees
        one weight set and ``release_bf16`` may free the bf16 matrices.  Needs the head's fp8 copy; same width requirement as
        ``wide``; ``all_rows`` without ``mid`` is a ``ValueError``.  Not a reference feature; quality on a trained checkpoint is
        unmeasured."""
        if mid and not wide:
            raise ValueError("use_fp8: mid=True needs wide=True (modes 5 / 6 are modes 3 / 4 plus the steps of 17..64 rows)")
        if all_rows and not mid:
            raise ValueError("use_fp8: all_rows=True needs wide=True, mid=True (the switch sits beside modes 5 / 6: the calls of 65 rows and more)")
        if enable and not self.bf16_released:   # (after release_bf16 the library refuses and says why)
            self.quantize_fp8()
        mode = ((2 if prefill else 1) + (2 if wide else 0) + (2 if mid else 0)) if enable else 0
        if self.bf16_released and not (enable and all_rows):     # (before the mode moves: the library pins the switch, and says why)
            check(lib().emu_llama_use_fp8_all(self.handle, 0), "emu_llama_use_fp8_all", self.ctx.handle)
        check(lib().emu_llama_use_fp8(self.handle, mode), "emu_llama_use_fp8", self.ctx.handle)
        self.fp8_decode = bool(enable)
        self.fp8_wide = bool(enable and wide)
        self.fp8_mid = bool(enable and mid)
        self.fp8_all = False                                     # (a mode below 5 clears the switch in the library)
        self._mode_changed()
        if mode >= 5:
            check(lib().emu_llama_use_fp8_all(self.handle, 1 if all_rows else 0), "emu_llama_use_fp8_all", self.ctx.handle)
            self.fp8_all = bool(all_rows)
            self._mode_changed()

    def fp8_dequantized(self, key: str) -> torch.Tensor:
        """fp32 value of a registered fp8 tensor (tests: feed the oracle the exact weights the stream uses)."""
        q, sc = self._fp8[key]
        return q.view(torch.float8_e4m3fn).to(torch.float32) * sc[:, None]

    # ------------------------------------------------------------------ optional MXFP4 decode stream
    _FP4_KINDS = ("wqkv", "wo", "wgu", "wdown")

    def _fp4_shape(self, key: str) -> Tuple[int, int]:
        """[N, K] of the matrix a registered fp4 key stands for, from its element bytes [N, K/2]."""
        q = self._fp4[key][0]
        return int(q.shape[0]), int(q.shape[1]) * 2

    def _fp4_source(self, key: str) -> torch.Tensor:
        """The packed (and sharded) bf16 matrix an fp4 key stands for: "<layer>.wqkv|wo|wgu|wdown" or "lm_head".  After
        ``release_bf16`` the matrix is gone: a storage-less (meta) bf16 tensor of its shape, taken from the 4-bit tensors."""
        layer, _, kind = key.partition(".")
        if key != "lm_head" and (kind not in self._FP4_KINDS or not layer.isdigit() or int(layer) >= self.cfg.num_hidden_layers):
            raise KeyError(f"fp4 key {key!r}: expected '<layer>.wqkv|wo|wgu|wdown' or 'lm_head'")
        if self.bf16_released:
            shape = tuple(self._fp8[key][0].shape) if self.fp8_all else self._fp4_shape(key)
            return torch.empty(shape, dtype=BF16, device="meta")
        return self.lm_head if key == "lm_head" else self._keep[key]

    def _fp4_keys(self):
        return [f"{i}.{k}" for i in range(self.cfg.num_hidden_layers) for k in self._FP4_KINDS] + ["lm_head"]

    def _fp4_register(self, key: str) -> None:
        """Hand the library the pointers of a layer once its four matrices are here (or of the head)."""
        if key == "lm_head":
            q, sc = self._fp4[key]
            check(lib().emu_llama_set_head_fp4(self.handle, q.data_ptr(), sc.data_ptr()), "emu_llama_set_head_fp4", self.ctx.handle)
            return
        i = key.split(".")[0]
        if all(f"{i}.{k}" in self._fp4 for k in self._FP4_KINDS):
            a = [t.data_ptr() for k in self._FP4_KINDS for t in self._fp4[f"{i}.{k}"]]
            check(lib().emu_llama_set_layer_fp4(self.handle, int(i), *a), "emu_llama_set_layer_fp4", self.ctx.handle)

    def quantize_fp4(self) -> None:
        """Build MXFP4 copies (4-bit elements, one power-of-two scale per 32: ``emu_amd.mxfp4``) of every packed matrix and of
        lm_head with the device quantiser and register them for the decode stream (B*T <= 2 rows; with ``use_fp4(wide=True)`` also
        steps of 3..16 rows, with ``all_rows=True`` every row count).  Keys already provided through ``load_fp4`` are kept.  Prefill and
        steps of more than 16 rows keep the bf16 weights unless ``all_rows``, so both sets stay resident (33B: bf16 66 GB + fp4
        17 GB) until ``release_bf16``.  The scale tensors are kept with their rows padded to ``mxfp4.scale_stride(K)`` bytes (byte 127;
        only where K is no multiple of 256), which is how the matrix-core kernels read them.  Round-to-nearest, not calibrated; not a reference feature; quality on a trained checkpoint is unmeasured."""
        if not self.ready:
            raise RuntimeError("quantize_fp4: load all weights first")
        self.__dict__.setdefault("_fp4", {})
        for key in self._fp4_keys():
            if key not in self._fp4:
                if self.bf16_released:
                    raise RuntimeError(f"quantize_fp4: the bf16 weights were released (release_bf16); {key!r} cannot be quantised anew")
                q, sc = ops.quantize_mxfp4_rows(self._fp4_source(key))
                self._fp4[key] = (q, mxfp4.pad_scales(sc, q.shape[1] * 2))
                self._fp4_register(key)

    def load_fp4(self, key: str, packed: torch.Tensor, scales: torch.Tensor) -> None:
        """Register externally prepared MXFP4 tensors (``mxfp4.quantize_rows`` or any quantiser that writes the format) for
        ``"<layer>.wqkv|wo|wgu|wdown"`` or ``"lm_head"``: ``packed`` uint8 [N, K/2], ``scales`` uint8 [N, K/32] for the [N, K] packed
        bf16 matrix of this rank (the tensor-parallel shard; lm_head: the rows this rank holds).  The scale rows are padded to
        ``mxfp4.scale_stride(K)`` on registration (a copy of the scales only, never of the element bytes)."""
        src = self._fp4_source(key)
        if src is None:
            raise RuntimeError(f"load_fp4({key!r}): load the bf16 weights first (their packed shapes define the fp4 shapes)")
        N, K = src.shape
        if K % 32:
            raise ValueError(f"load_fp4({key!r}): K = {K} is not a multiple of 32")
        for name, t, shape in (("packed", packed, (N, K // 2)), ("scales", scales, (N, K // 32))):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or tuple(t.shape) != shape:
                raise ValueError(f"load_fp4({key!r}): {name} must be uint8 {shape}, got "
                                 f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
        if self.fp4_decode:
            raise RuntimeError("load_fp4: switch the fp4 stream off first (use_fp4(False)); captured graphs hold the old pointers")
        self.__dict__.setdefault("_fp4", {})
        self._fp4[key] = (packed.to(self.device).contiguous(), mxfp4.pad_scales(scales.to(self.device).contiguous(), K))
        self._fp4_register(key)

    def use_fp4(self, enable: bool = True, wide: bool = False, all_rows: bool = False) -> None:
        """Switch the decode stream between the bf16 and the MXFP4 weights (invalidates captured decode graphs).  Whatever was not
        provided through ``load_fp4`` is quantised on the device first.  Exclusive with ``use_fp8``.

        ``use_fp4(True)``: steps of B*T <= 2 rows (greedy / sampled decode) stream the 4-bit set; everything else streams bf16.
        ``use_fp4(True, wide=True)``: steps of 3..16 rows (the default 5-beam search, a batch of prompts, contrastive search) stream
        the 4-bit set as well, through the matrix-core kernel (csrc/gemv_fp4_thin.hip); needs hidden, heads_local * head_dim and
        ffn_local to be at least 256 (the library refuses otherwise and says why; any multiple of 32 from there on will do, so the
        TP = 4 / 8 shards of the 33B shapes run: a width that is no multiple of 256 ends in a partial K stage).  Prefill and steps
        of more than 16 rows stream bf16 unless ``all_rows``.
        ``use_fp4(True, wide=True, all_rows=True)``: prefill and steps of 17 rows and more (beams x batch) run the 4-bit set too,
        through the 4-bit GEMM (csrc/gemm_fp4.hip; the RoPE and RMSNorm epilogue fusions of the bf16 prefill and the two-lane
        prefill are off), so one generation sees one weight set and ``release_bf16`` may free the bf16 matrices.  Same width
        requirement as ``wide``; ``all_rows`` without ``wide`` is a ``ValueError``."""
        if all_rows and not wide:
            raise ValueError("use_fp4: all_rows=True needs wide=True (mode 3 is mode 2 plus the calls of 17 rows and more)")
        if enable and not self.fp8_decode and not self.bf16_released:
            self.quantize_fp4()                                    # (with fp8 on, the library refuses and says why)
        mode = (3 if all_rows else 2 if wide else 1) if enable else 0
        check(lib().emu_llama_use_fp4(self.handle, mode), "emu_llama_use_fp4", self.ctx.handle)
        self.fp4_decode = bool(enable)
        self.fp4_wide = bool(enable and wide)
        self.fp4_all = bool(enable and all_rows)
        self._mode_changed()

    def release_bf16(self) -> None:
        """Free the bf16 packed matrices and the bf16 lm_head; needs ``use_fp4(True, wide=True, all_rows=True)``, which it pins (33B:
        65 GB leave, the 17 GB of 4-bit tensors stay; the norm gains, the embedding and the RoPE tables stay), or
        ``use_fp8(True, wide=True, mid=True, all_rows=True)`` with or without ``prefill``, which it pins likewise (the 32 GB of fp8
        tensors stay).  Afterwards ``use_fp4(False)``, ``use_fp4(True)`` without ``all_rows``, ``use_fp8`` and
        ``set_decode_fused(!= 0)`` raise with the library's message -- after an fp8 release everything but
        ``use_fp8(True, wide=True, mid=True, all_rows=True)``, ``use_fp4`` included; there is no way back short of a new engine.
        Invalidates captured decode graphs."""
        if not (self.fp4_all or self.fp8_all):
            raise RuntimeError("release_bf16: switch every row count to one quantised set first (use_fp4(True, wide=True, all_rows=True) "
                               "or use_fp8(True, wide=True, mid=True, all_rows=True))")
        check(lib().emu_llama_release_bf16(self.handle), "emu_llama_release_bf16", self.ctx.handle)
        self.bf16_released = True
        for key in [k for k in self._keep if k.split(".")[1] in self._FP4_KINDS]:
            del self._keep[key]
        self.lm_head = None
        self.__dict__.pop("_pack", None)                     # (the library dropped the sets with the bf16 rows)
        self.bf16_pack_on = self.bf16_pack_wide = False
        self._mode_changed()

    def fp4_dequantized(self, key: str) -> torch.Tensor:
        """fp32 value of a registered MXFP4 tensor (exact in bf16; tests feed the oracle the weights the stream uses)."""
        q, sc = self._fp4[key]
        return mxfp4.dequantize(q, sc[:, :q.shape[1] // 16])        # (the scale rows are kept padded: mxfp4.scale_stride)

    # ------------------------------------------------------------------ KV cache / workspace
    KV_BUCKETS = (256, 512, 1024)

    def kv_capacity(self, need: int) -> int:
        """KV slots to allocate for a request that will touch ``need`` positions: the smallest bucket that holds it
        (requests up to 1024 positions run the one-launch decode attention and a smaller cache), else the model
        maximum.  Buckets keep the allocation -- and any captured decode graph's launch geometry -- reusable."""
        cap = self.cfg.max_position_embeddings
        if need > cap:
            raise ValueError("prompt + max_new_tokens exceeds max_position_embeddings")
        for b in self.KV_BUCKETS:
            if need <= b <= cap:
                return b
        return cap

    def alloc_kv(self, batch: int, s_max: int, zero: bool = True, which: str = "main") -> None:
        """Make a cache of ``batch`` rows x ``s_max`` slots the engine's current one.  Three caches persist side by side, the
        "main" one (prefill, greedy / sampling), the "beam" one (``fan_out_kv``: prompts x beams rows) and the "suffix" one (the
        candidates' own few slots behind a shared prompt: ``score_continuations(share_prefix=True)``), each re-used while its
        shape stays the same: the pointers a captured hipGraph holds stay valid from call to call.  A KV prefix
        (``set_kv_prefix``) does not survive a change of cache."""
        slots = self.__dict__.setdefault("_kv_slots", {})
        cur = slots.get(which)
        if cur is None or cur[2] != batch or cur[3] != s_max:
            L, Hl, D = self.cfg.num_hidden_layers, self.plan.heads_local, self.cfg.head_dim
            slots[which] = None                            # free the old one first
            cur = None
            make = torch.zeros if zero else torch.empty
            cur = (make(L, batch, Hl, s_max, D, device=self.device, dtype=BF16),
                   make(L, batch, Hl, s_max, D, device=self.device, dtype=BF16), batch, s_max)
            slots[which] = cur
            self._ws = None
            self._drop_loop_states()                       # graphs captured on the replaced cache are void
        if self.kcache is cur[0]:
            self.set_kv_share(0, 0)
            self.set_kv_prefix(None, None, 0, 0)
            return
        self.kcache, self.vcache, self.kv_batch, self.s_max = cur
        check(lib().emu_llama_set_kv(self.handle, self.kcache.data_ptr(), self.vcache.data_ptr(), batch, s_max),
              "emu_llama_set_kv")
        self._kv_share = False
        self._kv_prefix = None                             # (emu_llama_set_kv switched it off)

    KV_SHARE_MAX = 8                                   # DECODE_SHARE_MAX of the decode attention kernel

    def release_kv(self, which: Optional[str] = None) -> None:
        """Free the persistent KV caches (``which`` = "main" / "beam" / "suffix" / None for all): alloc_kv keeps its caches
        resident for the life of the engine (several GB per rank after one 5-beam search at 60 layers) so that captured graphs stay
        valid; a server that is done with beam search hands the memory back here.  Captured decode graphs are dropped."""
        slots = self.__dict__.get("_kv_slots", {})
        self.set_kv_prefix(None, None, 0, 0)               # a prefix may point into the cache that goes
        for k in ([which] if which else list(slots)):
            cur = slots.pop(k, None)
            if cur is not None and self.kcache is cur[0]:      # the engine's current cache goes: the next prefill allocates anew
                self.kcache = self.vcache = None
        if self.kcache is None:
            # the library must not keep pointers into memory the allocator may hand out again: detach, so that a forward / step /
            # regress call before the next alloc_kv fails with -22 instead of writing K / V into freed memory
            self.kv_batch = self.s_max = 0
            check(lib().emu_llama_set_kv(self.handle, None, None, 0, 0), "emu_llama_set_kv", self.ctx.handle)
        self._mode_changed()

    def set_kv_share(self, rows_per_prompt: int, shared_slots: int) -> None:
        """Groups of ``rows_per_prompt`` consecutive cache rows keep their first ``shared_slots`` slots (the prompt) in the
        group's first row only (include/emu_hip.h: emu_llama_set_kv_share); (0, 0) = every row owns its slots."""
        if rows_per_prompt <= 1 and not getattr(self, "_kv_share", False):
            return
        if rows_per_prompt > 1 and getattr(self, "_kv_prefix", None) is not None:
            raise ValueError("set_kv_share: not while a KV prefix is set (set_kv_prefix(None, None, 0, 0) first)")
        check(lib().emu_llama_set_kv_share(self.handle, int(rows_per_prompt), int(shared_slots)), "emu_llama_set_kv_share")
        self._kv_share = rows_per_prompt > 1

    def set_kv_prefix(self, kprefix: Optional[torch.Tensor], vprefix: Optional[torch.Tensor], prefix_s_max: int,
                      prefix_len: int) -> None:
        """While set, ``forward`` with T > 1 attends slots [kstart, prefix_len) of the read-only caches ``kprefix`` / ``vprefix``
        [L, 1, Hl, prefix_s_max, D] plus the rows' own slots of the current cache (include/emu_hip.h: emu_llama_set_kv_prefix);
        ``None`` / 0 switches it off.  One-row, chunk and token steps and ``set_kv_share`` are refused meanwhile."""
        on = kprefix is not None and vprefix is not None and prefix_len > 0
        if not on and getattr(self, "_kv_prefix", None) is None:
            return
        if on:
            L, Hl, D = self.cfg.num_hidden_layers, self.plan.heads_local, self.cfg.head_dim
            want = (L, 1, Hl, int(prefix_s_max), D)
            if tuple(kprefix.shape) != want or tuple(vprefix.shape) != want or not (kprefix.is_contiguous() and vprefix.is_contiguous()) \
                    or kprefix.dtype != BF16 or vprefix.dtype != BF16:
                raise ValueError(f"set_kv_prefix: contiguous bf16 caches of shape {want}, got {tuple(kprefix.shape)}")
        check(lib().emu_llama_set_kv_prefix(self.handle, ops._p(kprefix) if on else None, ops._p(vprefix) if on else None,
                                            int(prefix_s_max) if on else 0, int(prefix_len) if on else 0),
              "emu_llama_set_kv_prefix", self.ctx.handle)
        self._kv_prefix = (kprefix, vprefix, int(prefix_s_max), int(prefix_len)) if on else None      # (keeps the tensors alive)

    def fan_out_kv(self, B: int, n: int, S: int, s_max: int, share: bool = True) -> None:
        """After a prefill of B prompts: a cache of B * n rows (n beams / candidates per prompt) that continue the prompts.
        transformers copies the prompt's keys and values to every beam (``_expand_inputs_for_generation``); here, for
        n <= 8, they stay in ONE row per prompt and the decode attention reads them from there (``set_kv_share``): no n-fold
        copy (6 GB at S = 770, 5 beams, 60 layers) and the prompt's keys cross the memory system once per step, not n times.
        ``share=False`` copies for every n: rows that run T > 1 tokens at a time (``score_continuations``) cannot share."""
        k_old, v_old = self.kcache, self.vcache
        # no zero fill: every slot a row reads was written first (the prompt's by the copy below -- with set_kv_share only the
        # group's first row is ever read there -- and a generated slot by the step that appends it)
        self.alloc_kv(B * n, s_max, zero=False, which="beam")
        if share and 2 <= n <= self.KV_SHARE_MAX:
            first = torch.arange(B, device=self.device) * n
            self.kcache[:, first, :, :S] = k_old[:, :, :, :S]
            self.vcache[:, first, :, :S] = v_old[:, :, :, :S]
            self.set_kv_share(n, S)
        else:
            rep = torch.arange(B, device=self.device).repeat_interleave(n)
            self.kcache[:, :, :, :S] = k_old[:, rep, :, :S]
            self.vcache[:, :, :, :S] = v_old[:, rep, :, :S]

    def _workspace(self, B: int, T: int) -> torch.Tensor:
        need = lib().emu_llama_workspace_bytes(self.handle, B, T)
        need = max(need, B * T * self.cfg.hidden_size * 2)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, device=self.device, dtype=torch.uint8)
        return self._ws

    # ------------------------------------------------------------------ forward
    def embed_tokens(self, ids: torch.Tensor) -> torch.Tensor:
        """lm.model.embed_tokens (emu.py:119,193): ids [..] -> [.., hidden] bf16."""
        flat = ids.reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        return ops.embed_gather(flat, self.embed).view(*ids.shape, self.cfg.hidden_size)

    def forward(self, hidden: torch.Tensor, B: int, T: int, pos: torch.Tensor, slot: torch.Tensor,
                kstart: Optional[torch.Tensor], ctx: int, ctx_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
        """All decoder layers in place on the residual stream ``hidden`` [B*T, hidden] (not final-normed)."""
        assert hidden.is_contiguous() and hidden.dtype == BF16 and hidden.shape == (B * T, self.cfg.hidden_size)
        ws = self._workspace(B, T)
        check(lib().emu_llama_forward(self.handle, hidden.data_ptr(), B, T, pos.data_ptr(), slot.data_ptr(),
                                      ops._p(kstart), ops._p(ctx_dev), ctx, ws.data_ptr(), ws.numel(), ops.stream(self.device)),
              "emu_llama_forward", self.ctx.handle)
        return hidden

    CHUNK_MAX = 8                                      # DECODE_CHUNK_MAX of the chunk attention kernel

    def forward_chunk(self, hidden: torch.Tensor, B: int, T: int, pos0: torch.Tensor, slot0: torch.Tensor,
                      kstart: Optional[torch.Tensor], ctx: int, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
        """All decoder layers in place on ``hidden`` [B*T, hidden] for a chunk of T rows per sequence on top of the cache
        (include/emu_hip.h: emu_llama_forward_chunk): row i of sequence b at cache slot ``slot0[b] + i`` and position
        ``pos0[b] + i`` (int32 [B] on the device), ``ctx`` >= max slot0 + T sizes the launches.  What the engine cannot run this way
        is a ``ValueError`` before any device work."""
        if not 2 <= T <= self.CHUNK_MAX or B < 1 or B * T > 16:
            raise ValueError(f"forward_chunk: T in 2..{self.CHUNK_MAX} and B * T <= 16, got B = {B}, T = {T}")
        if tp_size_of(self) > 1:
            raise ValueError("forward_chunk: no tensor-parallel form")
        if getattr(self, "_kv_share", False):
            raise ValueError("forward_chunk: shared-prefix KV rows serve single-token steps only")
        if getattr(self, "_kv_prefix", None) is not None:
            raise ValueError("forward_chunk: a KV prefix serves forward with T > 1 only")
        if getattr(self, "decode_fused", 0):
            raise ValueError("forward_chunk: the fused decode modes 1-4 are one-row steps (set_decode_fused(0) first)")
        assert hidden.is_contiguous() and hidden.dtype == BF16 and hidden.shape == (B * T, self.cfg.hidden_size)
        assert pos0.dtype == torch.int32 and slot0.dtype == torch.int32 and pos0.numel() == B and slot0.numel() == B
        if ws is None:
            ws = self._workspace_chunk(B, T)
        try:
            check(lib().emu_llama_forward_chunk(self.handle, hidden.data_ptr(), B, T, pos0.data_ptr(), slot0.data_ptr(), ops._p(kstart),
                                                None, int(ctx), ws.data_ptr(), ws.numel(), ops.stream(self.device)),
                  "emu_llama_forward_chunk", self.ctx.handle)
        except EmuHipError as e:
            if "status -22" in str(e):
                raise ValueError(str(e)) from None
            raise
        return hidden

    def _workspace_chunk(self, B: int, T: int) -> torch.Tensor:
        """A workspace of its own for the chunk step of B x T rows (and the logits of its rows): a captured step holds its address."""
        need = max(int(lib().emu_llama_chunk_workspace_bytes(self.handle, B, T)), int(lib().emu_llama_workspace_bytes(self.handle, B * T, 1)),
                   B * T * self.cfg.hidden_size * 2)
        return torch.empty(need, device=self.device, dtype=torch.uint8)

    def set_layer_range(self, l0: int = 0, l1: int = -1) -> None:
        """Parity hook (include/emu_hip.h: emu_llama_set_layer_range): ``forward`` / ``prefill`` run layers [l0, l1) only;
        (0, -1) restores the whole stack.  Tests only."""
        check(lib().emu_llama_set_layer_range(self.handle, int(l0), int(l1)), "emu_llama_set_layer_range", self.ctx.handle)

    def final_norm_rows(self, hidden: torch.Tensor) -> torch.Tensor:
        out = torch.empty_like(hidden)
        check(lib().emu_llama_final_norm(self.handle, hidden.data_ptr(), out.data_ptr(), hidden.shape[0], ops.stream(self.device)),
              "emu_llama_final_norm")
        return out

    def logits(self, hidden_rows: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """final RMSNorm + lm_head on rows [M, hidden] -> [M, vocab] bf16."""
        M = hidden_rows.shape[0]
        if out is None:
            out = torch.empty(M, self.vocab, device=self.device, dtype=BF16)
        ws = self._workspace(max(M, 1), 1)
        check(lib().emu_llama_logits(self.handle, hidden_rows.data_ptr(), hidden_rows.stride(0), M, out.data_ptr(),
                                     out.stride(0), ws.data_ptr(), ws.numel(), ops.stream(self.device)),
              "emu_llama_logits", self.ctx.handle)
        return out

    # ------------------------------------------------------------------ model-level calls
    def prefill(self, embeds: torch.Tensor, attention_mask: torch.Tensor, s_max: Optional[int] = None,
                hf_generate_positions: bool = True):
        """Run S prompt slots through all layers and fill the KV cache.

        ``embeds`` [B,S,hidden] bf16, ``attention_mask`` [B,S] (1 = real token, left padded).
        ``hf_generate_positions``: position_ids = cumsum(mask)-1 as ``lm.generate`` does; False = arange(S) as the
        bare ``lm.model(...)`` call of generate_image does (emu.py:133-138).
        Returns (hidden [B,S,hidden] residual stream, kstart [B] int32, next_pos [B] int32)."""
        B, S, H = embeds.shape
        am = attention_mask.to(device=self.device, dtype=torch.int64)
        n_real = am.sum(dim=1)
        self.alloc_kv(B, s_max or self.cfg.max_position_embeddings)
        if S > self.s_max:
            raise ValueError(f"prompt length {S} exceeds KV capacity {self.s_max}")
        if hf_generate_positions:
            pos = (am.cumsum(-1) - 1).masked_fill(am == 0, 1)
            next_pos = n_real
        else:
            pos = torch.arange(S, device=self.device)[None].expand(B, -1)
            next_pos = torch.full((B,), S, device=self.device)
        slot = torch.arange(S, device=self.device)[None].expand(B, -1)
        kstart = (S - n_real).to(torch.int32).contiguous()
        hidden = embeds.to(device=self.device, dtype=BF16).reshape(B * S, H).contiguous().clone()
        if self.prefill_fusion:                          # slot = arange(S) below: the promise the fused epilogues need, for this call
            check(lib().emu_llama_set_prefill_fusion(self.handle, 1), "emu_llama_set_prefill_fusion", self.ctx.handle)
        self.forward(hidden, B, S, pos.reshape(-1).to(torch.int32).contiguous(),
                     slot.reshape(-1).to(torch.int32).contiguous(), kstart, ctx=S)
        return hidden.view(B, S, H), kstart, next_pos.to(torch.int32).contiguous()

    def decode_embeds(self, x: torch.Tensor, pos: torch.Tensor, slot_idx: int, kstart: torch.Tensor) -> torch.Tensor:
        """One cached step on explicit input embeddings x [B, hidden] (used by generate_image)."""
        B = x.shape[0]
        hidden = x.to(BF16).contiguous().clone()
        slot = torch.full((B,), slot_idx, device=self.device, dtype=torch.int32)
        self.forward(hidden, B, 1, pos, slot, kstart, ctx=slot_idx + 1)
        return hidden

    @torch.no_grad()
    def greedy_generate(self, embeds: torch.Tensor, attention_mask: torch.Tensor, max_new_tokens: int,
                        min_len: int = 1, eos_id: int = 2, pad_id: int = 32000, use_graph: bool = False,
                        stop_on_eos: bool = True) -> torch.Tensor:
        """``lm.generate(inputs_embeds=..., num_beams=1, do_sample=False)`` (emu.py:213-229): returns only the
        new ids [B, n].  The whole token loop stays on the device (embed -> layers -> logits -> argmax ->
        state advance per step, optionally replayed from one hipGraph); EOS/PAD bookkeeping of finished rows is
        applied afterwards on the host, which is equivalent because rows never interact."""
        B, S, H = embeds.shape
        s_max = self.kv_capacity(S + max_new_tokens)
        hidden, kstart, next_pos = self.prefill(embeds, attention_mask, s_max)
        last = hidden[:, -1, :]
        logits = torch.empty(B, self.vocab, device=self.device, dtype=BF16)
        self.logits(last, out=logits)
        cur = ops.argmax(logits, suppress_id=eos_id if min_len >= 1 else -1)
        out_ids = torch.full((max_new_tokens, B), pad_id, device=self.device, dtype=torch.int32)
        out_ids[0] = cur
        if max_new_tokens > 1:
            st = GreedyState(self, B, cur, next_pos, S, kstart, out_ids)
            n_eager = max(0, min_len - 1)
            done = [1]                                          # rows of out_ids written so far

            def one(i):
                if i < n_eager and eos_id >= 0:
                    st.step_eager_suppress(eos_id)
                else:
                    (st.step_graph if use_graph else st.step)()
                done[0] = i + 2

            # the reference's loop ends when every row has emitted EOS (transformers' stopping criteria): look at the
            # device-side ids every EOS_POLL steps (one small host read; the launches in between stay queued ahead)
            run_polled(one, max_new_tokens - 1, EOS_POLL,
                       lambda: stop_on_eos and bool((out_ids[: done[0]] == eos_id).any(dim=0).all()))
        ids = out_ids.t().to(torch.int64)                       # [B, max_new]
        self.ctx.check_p2p()
        self.check_decode_fused()
        if not stop_on_eos:
            return ids
        return apply_eos_padding(ids, eos_id, pad_id)

    LOOKUP_POLL = 4        # lookup decode: steps between two host looks at the step counter and the finished flag

    @torch.no_grad()
    def lookup_generate(self, embeds: torch.Tensor, attention_mask: torch.Tensor, prompt_ids: torch.Tensor, max_new_tokens: int,
                        num_tokens: int, max_ngram: int = 2, min_len: int = 1, eos_id: int = 2, pad_id: int = 32000,
                        use_graph: bool = False, stop_on_eos: bool = True, drafts: Optional[torch.Tensor] = None,
                        stats: Optional[dict] = None, do_sample: bool = False, temperature: Optional[float] = None,
                        top_k: Optional[int] = None, top_p: Optional[float] = None, repetition_penalty: float = 1.0,
                        uniforms: Optional[torch.Tensor] = None, trace: Optional[list] = None) -> torch.Tensor:
        """``lm.generate(inputs_embeds=..., prompt_lookup_num_tokens=num_tokens, max_matching_ngram_size=max_ngram)``: greedy
        decoding that verifies up to ``num_tokens`` guessed ids per step (``emu_amd/speculate.py``), one sequence.  The guess is the
        continuation of the last n-gram's earlier occurrence in ``prompt_ids`` [1, S] (the ids behind ``embeds``; where
        ``attention_mask`` is 0 they are not history) followed by the generated ids.  A step is one ``emu_llama_lookup_step``:
        embed of 1 + k ids, the chunk forward, logits of the 1 + k rows, accept / append / next draft / state advance on the
        device; replayed from one hipGraph with ``use_graph``.  The host reads the step counter and the finished flag every
        ``LOOKUP_POLL`` steps.  Every emitted id is the arg-max of the model's own logits, through the few-row weight streams:
        the ids can differ from ``greedy_generate``'s only where a top-2 margin is inside bf16 rounding.

        ``drafts`` int [max_new_tokens, num_tokens]: row ``step`` (the number of ids emitted so far) is the draft, in place of
        the lookup -- tests and timing only.  ``stats``: a dict that receives ``steps_run`` and ``tokens_emitted`` (the ids the
        steps emitted: all but the first).  Rejected drafts leave stale K / V rows behind the accepted ones; the next step
        overwrites them before any query sees them, so the cache needs ``num_tokens`` slots beyond prompt + max_new_tokens.

        ``do_sample`` or ``repetition_penalty`` != 1 (the library's assisted decoding with a candidate generator that has no logits):
        every row picks its id with the device sampler's kernel, row i exactly as ``sample_generate(device_sampler=True)`` picks output
        index step + i -- the history extended by the draft ids before the row, the uniform ``uniforms[step + i]``
        (``speculate.row_select``; one ``emu_llama_lookup_sample_step`` per step, a loop state and a captured graph of its own) -- and
        the draft is kept for as long as each picked id equals the next draft id.  The first id is ``emu_sample_bf16``'s at step 0.
        ``uniforms`` fp32 [max_new_tokens] or [max_new_tokens, 1], by default ONE ``torch.rand`` from the global generator up front.
        With the same uniforms the ids are those of the one-row device loop wherever both see the same logits: the few-row streams
        round differently from the one-row ones, so a draw within that rounding of an interval's boundary (or an arg-max within it of
        the runner-up) may fall the other way.  ``trace``: a list that receives one host record per step (``step``, ``n_draft``,
        ``cur`` = the fed ids, ``logits`` = a CPU copy of the step's [T, V] rows, ``n_emit``); eager runs only."""
        B, S, H = embeds.shape
        k, max_new = int(num_tokens), int(max_new_tokens)
        select = bool(do_sample) or float(repetition_penalty) != 1.0
        genroute.lookup_route(k, B, tp_size_of(self), do_sample=bool(do_sample), repetition_penalty=float(repetition_penalty),
                              device_sampler=True)                             # a ValueError before any device work
        if select and self.vocab > SAMPLE_MAX_VOCAB:
            raise ValueError(f"lookup_generate: vocabulary {self.vocab} is above the sample kernel's bound {SAMPLE_MAX_VOCAB}")
        if uniforms is not None and tuple(uniforms.shape) not in ((max_new,), (max_new, 1)):
            raise ValueError(f"lookup_generate: uniforms must be [max_new_tokens] or [max_new_tokens, 1] = [{max_new}], "
                             f"got {tuple(uniforms.shape)}")
        if trace is not None and use_graph:
            raise ValueError("lookup_generate: trace reads every step's logits on the host; not together with use_graph")
        if max_ngram < 1 or max_new < 1:
            raise ValueError(f"lookup_generate: max_matching_ngram_size and max_new_tokens must be at least 1, got {max_ngram}, {max_new}")
        if S + max_new + k > self.cfg.max_position_embeddings:
            raise ValueError(f"lookup_generate: prompt + max_new_tokens + prompt_lookup_num_tokens = {S + max_new + k} exceeds "
                             f"max_position_embeddings {self.cfg.max_position_embeddings}")
        if tuple(prompt_ids.shape) != (B, S):
            raise ValueError(f"lookup_generate: prompt_ids must be [{B}, {S}], got {tuple(prompt_ids.shape)}")
        if drafts is not None and tuple(drafts.shape) != (max_new, k):
            raise ValueError(f"lookup_generate: drafts must be [max_new_tokens, num_tokens] = [{max_new}, {k}], got {tuple(drafts.shape)}")
        if getattr(self, "decode_fused", 0):
            raise ValueError("lookup_generate: the fused decode modes 1-4 are one-row steps (set_decode_fused(0) first)")
        T, dev, V = k + 1, self.device, self.vocab
        s_max = self.kv_capacity(S + max_new + k)
        hidden, kstart, next_pos = self.prefill(embeds, attention_mask, s_max)
        if select:
            params = sample_params(do_sample, temperature, top_k, top_p, repetition_penalty, eos_id, min_len, eos_id, pad_id)
            uni = None if not do_sample else torch.rand(max_new, dtype=torch.float32, device=dev) if uniforms is None else \
                uniforms.to(device=dev, dtype=torch.float32).reshape(max_new).contiguous()
            i32z = torch.zeros(1, dtype=torch.int32, device=dev)
            first = int(ops.sample(self.logits(hidden[:, -1, :]), i32z, params, hist=torch.zeros(max_new, 1, dtype=torch.int32, device=dev),
                                   uniforms=None if uni is None else uni.view(max_new, 1))[0])
        else:
            first = int(ops.argmax(self.logits(hidden[:, -1, :]), suppress_id=eos_id if min_len >= 1 else -1)[0])
        hist0 = [int(t) for t in prompt_ids[0][attention_mask[0].to(prompt_ids.device) != 0]] + [first]
        finished0 = max_new <= 1 or (stop_on_eos and first == eos_id)
        if finished0:
            d0 = []
        elif drafts is not None:
            d0 = [int(t) for t in drafts[1]]
        else:
            d0 = speculate.lookup_draft(hist0, k, max_ngram)
        key = (T, self.s_max, max_new, int(max_ngram), int(min_len), int(eos_id), bool(stop_on_eos), drafts is not None,
               self.kcache.data_ptr(), self.mode_epoch)
        if select:                                                 # the launch holds the options: they are part of the graph's key
            key += tuple(getattr(params, name) for name, _ in params._fields_)

        def build():
            i32 = dict(dtype=torch.int32, device=dev)
            return dict(cur=torch.zeros(T, **i32), amax=torch.zeros(T, **i32), st=torch.zeros(ops.LOOKUP_STATE_INTS, **i32),
                        pos0=torch.zeros(1, **i32), slot0=torch.zeros(1, **i32), ctx=torch.zeros(1, **i32),
                        out_ids=torch.zeros(max_new, **i32), hist=torch.zeros(self.s_max, **i32), kstart=torch.zeros(1, **i32),
                        drafts=None if drafts is None else torch.zeros(max_new, k, **i32),
                        hid=torch.empty(T, H, device=dev, dtype=BF16), lg=torch.empty(T, V, device=dev, dtype=BF16),
                        cws=self._workspace_chunk(1, T), uni=torch.zeros(max_new, dtype=torch.float32, device=dev) if select else None)

        st = self._loop_state("lookup_sample" if select else "lookup", key, T, build)
        i32c = lambda v: torch.tensor(v, dtype=torch.int32)
        st["cur"].copy_(i32c([first] + d0 + [0] * (k - len(d0))))
        st["st"].copy_(i32c([1, int(finished0), len(d0), len(hist0), 0, 0, 0, 0]))
        st["pos0"].copy_(next_pos); st["slot0"].fill_(S); st["ctx"].fill_(S + 1); st["kstart"].copy_(kstart)
        st["out_ids"].fill_(pad_id); st["out_ids"][0] = first
        st["hist"][:len(hist0)] = i32c(hist0).to(dev)
        if drafts is not None:
            st["drafts"].copy_(drafts.to(torch.int32))
        if select and uni is not None:
            st["uni"].copy_(uni)
        p = lambda name: None if st[name] is None else st[name].data_ptr()
        Lb = lib()

        def body():
            args = (self.handle, T, p("cur"), p("amax"), p("st"), p("pos0"), p("slot0"), p("kstart"), p("ctx"), p("out_ids"), p("hist"),
                    st["hist"].numel(), p("drafts"), int(max_ngram), max_new, int(min_len), int(eos_id), int(bool(stop_on_eos)), self.s_max,
                    p("hid"), p("lg"), st["lg"].stride(0), p("cws"), st["cws"].numel())
            if select:
                check(Lb.emu_llama_lookup_sample_step(*args, C.byref(params), p("uni") if do_sample else None, max_new,
                                                      ops.stream(self.device)), "emu_llama_lookup_sample_step", self.ctx.handle)
            else:
                check(Lb.emu_llama_lookup_step(*args, ops.stream(self.device)), "emu_llama_lookup_step", self.ctx.handle)

        def finished() -> bool:
            step, fin = st["st"][:2].tolist()                                  # the one host read
            return bool(fin) or step >= max_new

        launched = [0]

        def one(i):
            if trace is not None:
                before = st["st"].tolist()
                fed = st["cur"].tolist()
            st["captured"].step(body, use_graph, key)
            launched[0] += 1
            if trace is not None and not before[1] and before[0] < max_new:
                trace.append(dict(step=before[0], n_draft=before[2], cur=fed, logits=st["lg"].cpu(),
                                  n_emit=int(st["st"][0]) - before[0]))

        timing = stats is not None and stats.get("timing")          # tools: time the loop alone (two device synchronisations)
        if timing:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        if not finished0:
            run_polled(one, max_new - 1, self.LOOKUP_POLL, finished)
        if stats is not None:
            vals = st["st"].tolist()
            stats.update(steps_run=vals[4], tokens_emitted=vals[5])
            if timing:                                             # steps_launched includes the no-op replays behind the end
                stats.update(loop_seconds=time.perf_counter() - t0, steps_launched=launched[0])
        ids = st["out_ids"][None].to(torch.int64)                               # [1, max_new]
        self.ctx.check_p2p()
        if not stop_on_eos:
            return ids
        return apply_eos_padding(ids, eos_id, pad_id)

    # ------------------------------------------------------------------ sampling
    @torch.no_grad()
    def sample_generate(self, embeds: torch.Tensor, attention_mask: torch.Tensor, max_new_tokens: int, min_len: int = 1,
                        do_sample: bool = True, temperature: Optional[float] = None, top_k: Optional[int] = None,
                        top_p: Optional[float] = None, repetition_penalty: float = 1.0, eos_id: int = 2,
                        pad_id: int = 32000, no_repeat_ngram_size: int = 0, num_return_sequences: int = 1,
                        device_sampler: bool = False, use_graph: bool = False,
                        uniforms: Optional[torch.Tensor] = None, constraint=None, device_ngram_ban: bool = False) -> torch.Tensor:
        """``lm.generate(inputs_embeds=..., num_beams=1)`` with logits processing: repetition penalty, min_length, then
        (when sampling) temperature / top-k / top-p warpers and a multinomial draw from torch's global CUDA generator
        (transformers' processor order).  The decoder runs on the HIP engine; the tiny per-step logits post-processing is
        host-driven, so this path is not graph-replayed.  ``num_return_sequences`` = n samples every prompt n times (rows
        prompt-major, as the library expands its inputs); without sampling the library refuses n > 1 and so does this.

        ``device_sampler=True`` (opt-in) keeps the token loop on the device instead: the first token comes from
        ``emu_sample_bf16`` on the prefill logits, every further one from one ``emu_llama_sample_step`` call (embed -> layers ->
        logits -> penalty / suppress / temperature / top-k / top-p / draw / EOS bookkeeping in one kernel -> state advance),
        replayed from one hipGraph with ``use_graph``; the host only reads the rows' ``unfinished`` flags every ``EOS_POLL`` steps.
        What is computed is specified in ``emu_amd/sampling.py``.  The draws use ``uniforms`` [max_new_tokens, rows] fp32 in [0, 1)
        -- by default ONE ``torch.rand`` from the global generator up front: seed-stable, but a different random stream from the
        host path's ``multinomial``, which is why this is an option.

        ``constraint`` (``emu_amd.constrain.TokenTrie`` or a callable (batch_id, ids generated so far) -> allowed ids, the library's
        ``prefix_allowed_tokens_fn``): the mask stands where the library's PrefixConstrainedLogitsProcessor does, after the
        processors and ahead of the warpers (``do_sample=False`` = constrained greedy).  ``device_ngram_ban=True`` (opt-in, read only
        with ``device_sampler=True``): the ban of ``no_repeat_ngram_size`` runs inside the selection kernel (``sampling.banned_ngram_mask``
        over the ids the row has generated), and the loop stays capturable.

        Which of this runs on the device, in which variant of the selection kernels, and what is refused (a ValueError before any
        device work) or handed back to the host loop with one warning: ``genroute.sample_route``."""
        trie, allow_fn = resolve_constraint(constraint, self.vocab, eos_id, min_len, num_return_sequences)
        ngram = int(no_repeat_ngram_size or 0)
        route = genroute.sample_route(self.vocab, tp_size_of(self), max_new_tokens, device_sampler, ngram, device_ngram_ban,
                                      genroute.constraint_kind(constraint))
        if route.warning is not None:
            warn_once(LlamaEngine, *route.warning)
        if num_return_sequences > 1:
            if not do_sample:
                raise ValueError("Greedy methods without beam search do not support `num_return_sequences` different than 1")
            embeds = embeds.repeat_interleave(num_return_sequences, dim=0)
            attention_mask = attention_mask.repeat_interleave(num_return_sequences, dim=0)
        B, S, H = embeds.shape
        dev = self.device
        s_max = self.kv_capacity(S + max_new_tokens)
        if route.device and uniforms is not None and tuple(uniforms.shape) != (max_new_tokens, B):
            raise ValueError(f"uniforms must be [max_new_tokens, rows] = [{max_new_tokens}, {B}], got {tuple(uniforms.shape)}")
        hidden, kstart, pos = self.prefill(embeds, attention_mask, s_max)
        row = hidden[:, -1, :]
        if route.device:
            return self._sample_device(row, B, S, kstart, pos, max_new_tokens, min_len, do_sample, temperature, top_k, top_p,
                                       repetition_penalty, eos_id, pad_id, use_graph, uniforms, trie, **route.device_kw)
        out = torch.full((B, max_new_tokens), pad_id, dtype=torch.int64, device=dev)
        unfinished = torch.ones(B, dtype=torch.int64, device=dev)
        hid = torch.empty(B, H, device=dev, dtype=BF16)
        n = 0
        for step in range(max_new_tokens):
            scores = process_logits(self.logits(row).float(), out[:, :step], step < min_len, eos_id, do_sample, temperature,
                                    top_k, top_p, repetition_penalty, no_repeat_ngram_size=ngram,
                                    allowed=None if allow_fn is None else allowed_mask(allow_fn, out[:, :step], 1, self.vocab))
            if do_sample:
                nxt = torch.multinomial(torch.softmax(scores, dim=-1), num_samples=1).squeeze(1)
            else:
                nxt = scores.argmax(dim=-1)
            nxt = nxt * unfinished + pad_id * (1 - unfinished)
            out[:, step] = nxt
            n = step + 1
            unfinished = unfinished * (nxt != eos_id).long()
            if int(unfinished.max().item()) == 0 or n == max_new_tokens:
                break
            ops.embed_gather(nxt.to(torch.int32).contiguous(), self.embed, out=hid)
            slot = torch.full((B,), S + step, device=dev, dtype=torch.int32)
            self.forward(hid, B, 1, pos, slot, kstart, ctx=S + step + 1)
            pos = pos + 1
            row = hid
        self.ctx.check_p2p()
        return out[:, :n]

    _warned_sampler_vocab = False          # one warning per process (sample_generate)
    _warned_ngram_ban = False              # ... and for device_ngram_ban outside what the kernels take (both generate loops)

    def _sample_device(self, row: torch.Tensor, B: int, S: int, kstart: torch.Tensor, next_pos: torch.Tensor, max_new: int,
                       min_len: int, do_sample: bool, temperature, top_k, top_p, repetition_penalty: float, eos_id: int,
                       pad_id: int, use_graph: bool, uniforms: Optional[torch.Tensor], trie: Optional[TokenTrie] = None,
                       ngram: int = 0) -> torch.Tensor:
        """The device-side loop of ``sample_generate(device_sampler=True)``, after the prefill.  ``trie``: the selection's "trie"
        variant (``ops.SELECT_ENTRY``), every row starting at the root.  ``ngram`` > 0: its "ngram" variant."""
        dev = self.device
        if do_sample:
            uni = torch.rand(max_new, B, dtype=torch.float32, device=dev) if uniforms is None else \
                uniforms.to(device=dev, dtype=torch.float32).contiguous()
        else:
            uni = None
        out_ids = torch.full((max_new, B), pad_id, device=dev, dtype=torch.int32)
        st = SampleState(self, B, next_pos, S, kstart, out_ids, uni,
                         sample_params(do_sample, temperature, top_k, top_p, repetition_penalty, eos_id, min_len, eos_id, pad_id),
                         None if trie is None else trie.tables(dev), ngram)
        self.logits(row, out=st.logits)
        st.first()
        # the only host read: the rows' flags, every EOS_POLL steps (the launches in between stay queued ahead)
        run_polled(lambda i: (st.step_graph if use_graph else st.step)(), max_new - 1, EOS_POLL, lambda: not bool(st.unfinished.any()))
        ids = out_ids.t().to(torch.int64)
        self.ctx.check_p2p()
        # a finished row emitted PAD on the device; steps between the last row's EOS and the poll that saw it are cut off here:
        # the width is one past the last step at which any row was still unfinished, the host path's rule
        return apply_eos_padding(ids, eos_id, pad_id)

    # ------------------------------------------------------------------ scoring given text
    SCORE_CHUNK_ROWS = 256     # rows of logits per lm_head call of score(via="prefill"), see there
    SCORE_MAX_ROWS = 64        # rows of one teacher-forced step (the advance kernel's one wave of rows)

    def _score_args(self, prefix_embeds, prefix_mask, cont_ids, cont_mask, via, reference_logits) -> Tuple[int, int, int]:
        """The refusals of ``score``, before any device work; returns (B, S, T)."""
        if via not in ("decode", "prefill"):
            raise ValueError(f"score: via must be 'decode' or 'prefill', got {via!r}")
        if prefix_embeds.dim() != 3 or prefix_embeds.shape[2] != self.cfg.hidden_size:
            raise ValueError(f"score: prefix_embeds must be [B, S, {self.cfg.hidden_size}], got {tuple(prefix_embeds.shape)}")
        B, S, _ = prefix_embeds.shape
        if tuple(prefix_mask.shape) != (B, S):
            raise ValueError(f"score: prefix_mask must be [{B}, {S}], got {tuple(prefix_mask.shape)}")
        if cont_ids.dim() != 2 or cont_ids.shape[0] != B:
            raise ValueError(f"score: cont_ids must be [{B}, T], got {tuple(cont_ids.shape)}")
        T = cont_ids.shape[1]
        if T < 1 or S < 1:
            raise ValueError("score: needs at least one prefix slot and one continuation token")
        if cont_mask is not None and tuple(cont_mask.shape) != (B, T):
            raise ValueError(f"score: cont_mask must be [{B}, {T}], got {tuple(cont_mask.shape)}")
        if S + T > self.cfg.max_position_embeddings:
            raise ValueError(f"score: prefix + continuation = {S + T} exceeds max_position_embeddings "
                             f"{self.cfg.max_position_embeddings}")
        if via == "decode" and B > self.SCORE_MAX_ROWS:
            raise ValueError(f"score: via='decode' steps at most {self.SCORE_MAX_ROWS} rows at a time, got {B}; use via='prefill'")
        if reference_logits is not None and tuple(reference_logits.shape) != (B, T, self.vocab):
            raise ValueError(f"score: reference_logits must be [{B}, {T}, {self.vocab}], got {tuple(reference_logits.shape)}")
        return B, S, T

    @torch.no_grad()
    def score(self, prefix_embeds: torch.Tensor, prefix_mask: torch.Tensor, cont_ids: torch.Tensor,
              cont_mask: Optional[torch.Tensor] = None, via: str = "decode", use_graph: bool = False,
              reference_logits: Optional[torch.Tensor] = None, return_logits: bool = False) -> Dict[str, torch.Tensor]:
        """How probable is a GIVEN continuation: per-token log-probabilities of ``cont_ids`` [B, T] (right padded) behind the prefix
        ``prefix_embeds`` [B, S, hidden] / ``prefix_mask`` [B, S] (left padded, images already scattered in, as for ``generate``).
        The reference has this only as the loss of ``lm(..., labels=...)`` (Emu1/models/modeling_llama.py:110-116) behind ``predict``
        (prediction_mixin.py:36-131); what is computed per row is specified in ``emu_amd/scoring.py``.

        ``cont_mask`` false, or an id outside the vocabulary, means IGNORED: ``lp = 0``, ``counted`` false, and id 0 is fed in its
        place.  ``lp[b, 0]`` is read from the prefix's last row, ``lp[b, t]`` from the row fed ``cont_ids[b, t - 1]``.  Returns
        ``lp`` / ``lse`` [B, T] fp32, ``counted`` [B, T] bool, ``top1`` [B, T] int64; with ``reference_logits`` [B, T, vocab] bf16
        also ``kl`` (KL(reference || this run) per token) and ``agree`` (bool); with ``return_logits`` the ``logits`` [B, T, vocab].

        ``via="decode"``: one teacher-forced ``emu_llama_score_step`` per token (a captured graph with ``use_graph``), i.e. the
        kernels generation runs -- whatever weight stream is active (bf16, e4m3, MXFP4 narrow or wide) is the one that is scored.
        ``via="prefill"``: ONE forward of the T - 1 fed tokens per row on top of the prefix's cache, then the head in chunks of
        ``SCORE_CHUNK_ROWS`` rows: 256 rows keep the [rows, vocab] buffer at 16.5 MB for the 32 274-token vocabulary and are a whole
        tile of the head's GEMM, so lm_head is streamed once per 256 rows at full matrix-core rate.  Arguments are checked before any
        device work (ValueError)."""
        B, S, T = self._score_args(prefix_embeds, prefix_mask, cont_ids, cont_mask, via, reference_logits)
        s_max = self.kv_capacity(S + T)
        targets = self._score_targets(cont_ids, cont_mask)
        hidden, kstart, next_pos = self.prefill(prefix_embeds, prefix_mask, s_max)
        first_logits = self.logits(hidden[:, -1, :])
        return self._score_on_cache(first_logits, S, kstart, next_pos, targets, via, use_graph, reference_logits, return_logits)

    def _score_targets(self, cont_ids: torch.Tensor, cont_mask: Optional[torch.Tensor]) -> torch.Tensor:
        """[B, T] int32 on the device, the ignored ones as scoring.IGNORE_INDEX."""
        t = cont_ids.to(device=self.device, dtype=torch.int64)
        ignored = (t < 0) | (t >= self.vocab)
        if cont_mask is not None:
            ignored = ignored | ~cont_mask.to(device=self.device, dtype=torch.bool)
        return t.masked_fill(ignored, IGNORE_INDEX).to(torch.int32).contiguous()

    def _score_on_cache(self, first_logits: torch.Tensor, S: int, kstart: torch.Tensor, next_pos: torch.Tensor,
                        targets: torch.Tensor, via: str, use_graph: bool, reference_logits: Optional[torch.Tensor],
                        return_logits: bool) -> Dict[str, torch.Tensor]:
        """``score`` after the prefill: the engine's current cache holds the S prefix slots of ``targets.shape[0]`` rows,
        ``first_logits`` [B, vocab] are the logits of the prefix's last rows."""
        dev = self.device
        B, T = targets.shape
        tgt = torch.empty(T, B, device=dev, dtype=torch.int32).copy_(targets.t())     # [T, B]: a step's targets are one row
        res = {"lp": torch.zeros(T, B, device=dev, dtype=torch.float32), "lse": torch.zeros(T, B, device=dev, dtype=torch.float32),
               "top1": torch.zeros(T, B, device=dev, dtype=torch.int32)}
        keep = return_logits or reference_logits is not None
        all_logits = torch.empty(T, B, self.vocab, device=dev, dtype=BF16) if keep else None
        step0 = torch.zeros(1, device=dev, dtype=torch.int32)
        ops.token_logprob(first_logits, tgt, step_dev=step0, out=res)
        if keep:
            all_logits[0] = first_logits
        fed = tgt.clamp(min=0)                                           # an ignored target feeds id 0: the row is padding from there on
        if T > 1 and via == "decode":
            st = ScoreState(self, B, fed[0], next_pos, S, kstart, tgt, res)

            def one(i):
                st.step_graph() if use_graph else st.step()
                if keep:
                    all_logits[i + 1].copy_(st.logits)

            run_polled(one, T - 1, T - 1, lambda: False)                 # nothing to poll for: the tokens are given
        elif T > 1:
            n = T - 1
            hid = self.embed_tokens(fed[:n].t().contiguous()).reshape(B * n, self.cfg.hidden_size).contiguous()
            ar = torch.arange(n, device=dev, dtype=torch.int32)
            pos = (next_pos.to(torch.int32)[:, None] + ar[None]).reshape(-1).contiguous()
            slot = (S + ar)[None].expand(B, -1).reshape(-1).contiguous()
            self.forward(hid, B, n, pos, slot, kstart, ctx=S + n)        # no slot-order promise: T != ctx keeps the unfused sequence
            tg = targets[:, 1:].contiguous().reshape(-1)                 # rows of `hid` are row-major [B, n]
            flat = {k: torch.empty(B * n, device=dev, dtype=v.dtype) for k, v in res.items()}
            buf = torch.empty(min(self.SCORE_CHUNK_ROWS, B * n), self.vocab, device=dev, dtype=BF16)
            for r0 in range(0, B * n, self.SCORE_CHUNK_ROWS):
                r1 = min(r0 + self.SCORE_CHUNK_ROWS, B * n)
                lg = self.logits(hid[r0:r1], out=buf[: r1 - r0])
                ops.token_logprob(lg, tg[r0:r1], out={k: v[r0:r1] for k, v in flat.items()})
                if keep:
                    rows = torch.arange(r0, r1, device=dev)
                    all_logits[1 + rows % n, rows // n] = lg
            for k in res:
                res[k][1:] = flat[k].view(B, n).t()
        self.ctx.check_p2p()
        out = {"lp": res["lp"].t().contiguous(), "counted": targets >= 0, "lse": res["lse"].t().contiguous(),
               "top1": res["top1"].t().to(torch.int64)}
        if reference_logits is not None:
            ref = reference_logits.to(device=dev, dtype=BF16).transpose(0, 1).reshape(T * B, self.vocab).contiguous()
            kl = ops.token_logprob(all_logits.view(T * B, self.vocab), tgt.view(-1), ref_logits=ref)
            out["kl"] = kl["kl"].view(T, B).t().contiguous()
            out["agree"] = kl["agree"].view(T, B).t().to(torch.bool)
        if return_logits:
            out["logits"] = all_logits.transpose(0, 1).contiguous()
        return out

    @torch.no_grad()
    def score_continuations(self, prefix_embeds: torch.Tensor, prefix_mask: torch.Tensor, cand_ids: torch.Tensor,
                            cand_mask: Optional[torch.Tensor] = None, n_segments: int = 1, via: str = "prefill",
                            hf_generate_positions: bool = True, share_prefix: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """Per-token log-probabilities of N candidate continuations ``cand_ids`` [N, Tc] (right padded, ``cand_mask`` [N, Tc]) of
        ONE prefix ``prefix_embeds`` [1, S, hidden]: what prediction_mixin.py:36-131 ranks candidate answers by.  The reference runs
        prompt + candidate through the model for every candidate; here the prompt is prefilled once, its K / V slots are copied to
        the rows of a segment (``fan_out_kv``'s copy), and ``score`` runs the candidates on top.  The segments are the reference's
        (``scoring.split_segments``); each is scored to the width of its own longest candidate.  ``hf_generate_positions``: as
        ``prefill``'s (False = arange positions, the bare ``lm(...)`` call of the reference's ``predict``).  Returns (lp [N, Tc]
        fp32, counted [N, Tc] bool).

        ``share_prefix=True`` (opt-in; ``via="prefill"``, one rank, head_dim 128): no copy.  The prompt's K / V stay in the main
        cache, a segment's candidates write their own few slots into the small "suffix" cache (``scoring.shared_prefix_plan`` has
        the shapes and bytes of both routes) and the two-segment flash kernel attends both (``set_kv_prefix``).  With S a multiple of
        64 the result is bit-identical to the copying route's, else it agrees to bf16 rounding (another tile partition)."""
        if prefix_embeds.dim() != 3 or prefix_embeds.shape[0] != 1:
            raise ValueError(f"score_continuations: prefix_embeds must be [1, S, hidden], got {tuple(prefix_embeds.shape)}")
        if cand_ids.dim() != 2 or cand_ids.shape[0] < 1:
            raise ValueError(f"score_continuations: cand_ids must be [N, Tc], got {tuple(cand_ids.shape)}")
        N, Tc = cand_ids.shape
        segments = split_segments(N, n_segments)
        if share_prefix and via != "prefill":
            raise ValueError("score_continuations: share_prefix=True runs via='prefill' only (a one-token step has no two-segment form)")
        if share_prefix and tp_size_of(self) > 1:
            raise ValueError("score_continuations: share_prefix=True has no tensor-parallel form (no multi-rank run of it exists)")
        if share_prefix and self.cfg.head_dim != 128:
            raise ValueError(f"score_continuations: share_prefix=True needs head_dim 128, got {self.cfg.head_dim}")
        for a, b in segments:                                            # every refusal before any device work
            self._score_args(prefix_embeds.expand(b - a, -1, -1), prefix_mask.expand(b - a, -1), cand_ids[a:b],
                             None if cand_mask is None else cand_mask[a:b], via, None)
        S = prefix_embeds.shape[1]
        targets = self._score_targets(cand_ids, cand_mask)
        width = (targets >= 0).int().mul(torch.arange(1, Tc + 1, device=self.device, dtype=torch.int32)[None]).amax(dim=1)
        widths = [max(1, int(width[a:b].max())) for a, b in segments]
        s_max = self.kv_capacity(S + max(widths))
        hidden, kstart, next_pos = self.prefill(prefix_embeds, prefix_mask, s_max, hf_generate_positions)
        first_logits = self.logits(hidden[:, -1, :])
        lp = torch.zeros(N, Tc, device=self.device, dtype=torch.float32)
        if share_prefix:
            plan = shared_prefix_plan(N, S, widths, self.cfg.num_hidden_layers, self.plan.heads_local, self.cfg.head_dim, self.kv_capacity)
            kmain, vmain = self.kcache, self.vcache                      # the prompt's cache: the prefix segment, read only from here on
            try:
                for (a, b), w, seg in zip(segments, widths, plan["segments"]):
                    self.alloc_kv(b - a, seg["suffix_capacity"], zero=False, which="suffix")     # every slot read was written first
                    self.set_kv_prefix(kmain, vmain, s_max, S)
                    # the rows' own slots start at 0 (S = 0 below).  The engine runs T > 1 rows behind a prefix, so a segment of
                    # width 2 (ONE fed token) feeds one more, ignored, token: causal attention keeps it out of the rows before it
                    tg = targets[a:b, :w]
                    if w == 2:
                        tg = torch.cat([tg, torch.full_like(tg[:, :1], IGNORE_INDEX)], dim=1)
                    r = self._score_on_cache(first_logits.expand(b - a, -1).contiguous(), 0, kstart.expand(b - a).contiguous(),
                                             next_pos.expand(b - a).contiguous(), tg.contiguous(), via, False, None, False)
                    lp[a:b, :w] = r["lp"][:, :w]
            finally:
                self.set_kv_prefix(None, None, 0, 0)
            return lp, targets >= 0
        for (a, b), w in zip(segments, widths):
            self.alloc_kv(1, s_max)                                      # back to the prefix's cache: the source of the copy
            self.fan_out_kv(1, b - a, S, s_max, share=False)
            r = self._score_on_cache(first_logits.expand(b - a, -1).contiguous(), S, kstart.expand(b - a).contiguous(),
                                     next_pos.expand(b - a).contiguous(), targets[a:b, :w].contiguous(), via, False, None, False)
            lp[a:b, :w] = r["lp"]
        return lp, targets >= 0

    # ------------------------------------------------------------------ contrastive search
    @torch.no_grad()
    def contrastive_generate(self, embeds: torch.Tensor, attention_mask: torch.Tensor, max_new_tokens: int,
                             penalty_alpha: float, top_k: int, min_len: int = 1, repetition_penalty: float = 1.0,
                             eos_id: int = 2, pad_id: int = 32000, trace: Optional[dict] = None,
                             force_ids: Optional[torch.Tensor] = None, device_contrastive: bool = False,
                             use_graph: bool = False) -> torch.Tensor:
        """``lm.generate(inputs_embeds=..., penalty_alpha=a, top_k=k)`` -- contrastive search as the reference's pinned
        transformers 4.31 runs it (Emu2/emu/emu.py:167,223 forwards both arguments): per step the k most probable tokens
        are each run one step further, and the one maximising (1 - a) * p(token) - a * max_j cos(h_token, h_j) over the
        final-norm hidden states h_j of everything before it is kept.  The k candidates are k extra rows of one decoder
        step that share the prompt's KV rows (as beams do); the kept candidate's KV slot is then copied to its siblings.
        a = 0 or k = 1 degenerate to greedy search (tested against the real reference's greedy ids).  Deviation: hidden
        states of left-padding positions are left out of the similarity (the library includes whatever the masked rows
        hold).  Parity beyond those invariants is unpinned: the transformers in this image no longer ships the mode.

        Diagnostics for the tests: ``trace`` receives ``margin`` (smallest winner / runner-up score gap) and ``steps`` (per
        step the candidate ids, their probabilities, their degeneration penalties and the selection, on the host);
        ``force_ids`` [B, n] replays a given token path (each forced token must be one of the step's k candidates) so two
        engines can be compared number by number along the same path.

        ``device_contrastive=True`` (opt-in) keeps the token loop on the device: ``_contrastive_device`` (csrc/contrastive.hip,
        specified in ``emu_amd/sampling.py``: ``contrastive_reference_*``), replayed from one hipGraph with ``use_graph``.  The loop
        above stays the default and the fallback; the device's sums are fp32 in a fixed order, so a choice this loop decides by less
        than the rounding of either may fall the other way.  What is refused (a ValueError before any device work) and where the
        host loop takes over with one warning per process: ``genroute.contrastive_route``."""
        route = genroute.contrastive_route(self.vocab, tp_size_of(self), int(top_k), device_contrastive, trace is not None,
                                           force_ids is not None)
        if route.warning is not None:
            warn_once(LlamaEngine, *route.warning)
        if route.device:
            return self._contrastive_device(embeds, attention_mask, int(max_new_tokens), float(penalty_alpha), int(top_k),
                                            int(min_len), float(repetition_penalty), int(eos_id), int(pad_id), bool(use_graph))
        B, S, H = embeds.shape
        k, V, dev = int(top_k), self.vocab, self.device
        s_max = self.kv_capacity(S + max_new_tokens)
        hidden, kstart, next_pos = self.prefill(embeds, attention_mask, s_max)
        ctx_h = self.final_norm_rows(hidden.reshape(B * S, H).contiguous()).view(B, S, H).float()
        ctx_ok = torch.arange(S, device=dev)[None, :] >= kstart[:, None].to(dev)
        logit = self.logits(hidden[:, -1, :]).float()
        self.fan_out_kv(B, k, S, s_max)
        kstart_k = kstart.repeat_interleave(k).contiguous()
        pos = next_pos.repeat_interleave(k).contiguous()
        out = torch.full((B, max_new_tokens), pad_id, dtype=torch.int64, device=dev)
        unfinished = torch.ones(B, dtype=torch.int64, device=dev)
        hid = torch.empty(B * k, H, device=dev, dtype=BF16)
        ar = torch.arange(B, device=dev)
        n = 0
        for step in range(max_new_tokens):
            scores = process_logits(logit, out[:, :step], step < min_len, eos_id, False, repetition_penalty=repetition_penalty)
            top_p_, top_ids = torch.topk(torch.softmax(scores, dim=-1), k=k, dim=-1)          # [B, k]
            ops.embed_gather(top_ids.reshape(-1).to(torch.int32).contiguous(), self.embed, out=hid)
            slot = torch.full((B * k,), S + step, device=dev, dtype=torch.int32)
            self.forward(hid, B * k, 1, pos, slot, kstart_k, ctx=S + step + 1)
            nh = self.final_norm_rows(hid).float().view(B, k, H)
            cand_logits = self.logits(hid).float().view(B, k, V)
            cn = ctx_h / ctx_h.norm(dim=2, keepdim=True)
            nn_ = nh / nh.norm(dim=2, keepdim=True)
            cos = torch.einsum("bld,bkd->bkl", cn, nn_).masked_fill(~ctx_ok[:, None, :], -float("inf"))
            pen = cos.max(dim=-1)[0]
            score = (1.0 - penalty_alpha) * top_p_ - penalty_alpha * pen
            sel = score.argmax(dim=-1)                                                                    # [B]
            if force_ids is not None:
                hit = top_ids == force_ids[:, step, None].to(dev)
                if not bool((hit.any(dim=1) | ~unfinished.bool()).all()):
                    raise ValueError(f"contrastive_generate: forced token of step {step} is not among the {k} candidates")
                sel = torch.where(unfinished.bool(), hit.float().argmax(dim=1), sel)
            if trace is not None:
                t2 = torch.topk(score, k=2, dim=-1)[0]
                gap = torch.where(unfinished.bool(), t2[:, 0] - t2[:, 1], torch.full_like(t2[:, 0], float("inf")))
                trace["margin"] = min(trace.get("margin", float("inf")), float(gap.min()))
                trace.setdefault("steps", []).append(dict(ids=top_ids.cpu(), p=top_p_.float().cpu(), pen=pen.float().cpu(),
                                                          sel=sel.cpu(), live=unfinished.bool().cpu()))
            nxt = top_ids[ar, sel]
            nxt = nxt * unfinished + pad_id * (1 - unfinished)
            out[:, step] = nxt
            n = step + 1
            unfinished = unfinished * (nxt != eos_id).long()
            if int(unfinished.max().item()) == 0 or n == max_new_tokens:
                break
            # the kept candidate's KV slot goes to its k - 1 siblings; its hidden state joins the context
            src = (ar * k + sel).repeat_interleave(k)
            self.kcache[:, :, :, S + step] = self.kcache[:, src, :, S + step]
            self.vcache[:, :, :, S + step] = self.vcache[:, src, :, S + step]
            ctx_h = torch.cat((ctx_h, nh[ar, sel][:, None, :]), dim=1)
            ctx_ok = torch.cat((ctx_ok, torch.ones(B, 1, dtype=torch.bool, device=dev)), dim=1)
            logit = cand_logits[ar, sel]
            pos = pos + 1
        self.set_kv_share(0, 0)
        self.ctx.check_p2p()
        return out[:, :n]

    _warned_contrastive = False            # one warning per process (contrastive_generate(device_contrastive=True))

    def _contrastive_device(self, embeds: torch.Tensor, attention_mask: torch.Tensor, L_new: int, alpha: float, k: int, min_len: int,
                            repetition_penalty: float, eos_id: int, pad_id: int, use_graph: bool) -> torch.Tensor:
        """The loop of ``contrastive_generate`` with nothing left on the host but the replay of a hipGraph.  After the prefill the
        prompt's final-normed rows are divided by their norms ONCE into ``ctx_n`` [B, S + max_new_tokens, H] fp32 (every kept
        token's row joins it normalised; nothing is re-normalised per step), the prefill's logits go to row b * k of the step's
        [B * k, V] logits and ``sel`` starts at 0.  One step = {``emu_contrastive_advance`` phase 0 (slot / position from the device
        step counter) -> ``emu_contrastive_pick_bf16`` (the k candidates of the row the previous step kept) -> embedding gather ->
        the decoder step on B * k rows that share the prompt's KV rows -> final norm, logits -> ``emu_contrastive_score`` (penalty,
        selection, token / EOS / PAD bookkeeping, the kept row appended) -> ``emu_llama_contrastive_keep_kv`` (the kept KV slot to
        its siblings) -> counter + 1}: captured once per (B, k, S, cache, limits, options) with buffers the graph owns and replayed
        ``BEAM_POLL`` steps at a time between two reads of the ``unfinished`` flags; ``use_graph=False`` runs the same launches
        eagerly.  Steps replayed beyond the end change nothing (a finished prompt writes PAD; from the length limit on every kernel
        returns at once)."""
        if not hasattr(self, "handle"):
            raise RuntimeError("device_contrastive needs the HIP engine")
        B, S, H = embeds.shape
        V, dev, rows = self.vocab, self.device, B * k
        Lb = lib()
        s_max = self.kv_capacity(S + L_new)
        hidden, kstart, next_pos = self.prefill(embeds, attention_mask, s_max)
        ctx0 = self.final_norm_rows(hidden.reshape(B * S, H).contiguous()).view(B, S, H).double()
        logit0 = self.logits(hidden[:, -1, :])                                          # [B, V] bf16
        self.fan_out_kv(B, k, S, s_max)
        Lc = S + L_new
        key = (B, k, S, self.s_max, L_new, min_len, alpha, repetition_penalty, eos_id, pad_id, self.kcache.data_ptr(), self.mode_epoch)

        def build():
            i32 = dict(dtype=torch.int32, device=dev)
            return dict(ctx_n=torch.zeros(B, Lc, H, dtype=torch.float32, device=dev), lg=torch.zeros(rows, V, device=dev, dtype=BF16),
                        hid=torch.empty(rows, H, device=dev, dtype=BF16), normed=torch.empty(rows, H, device=dev, dtype=BF16),
                        cand_ids=torch.zeros(rows, **i32), cand_p=torch.zeros(rows, dtype=torch.float32, device=dev),
                        sel=torch.zeros(B, **i32), unfinished=torch.ones(B, **i32), out_ids=torch.empty(L_new, B, **i32),
                        step=torch.zeros(1, **i32), slot=torch.empty(rows, **i32), pos=torch.empty(rows, **i32),
                        pos0=torch.empty(rows, **i32), kstart=torch.empty(B, **i32), kstart_k=torch.empty(rows, **i32),
                        ws=torch.empty(int(Lb.emu_contrastive_workspace_bytes(B, k, Lc)), dtype=torch.uint8, device=dev))

        st = self._loop_state("contrastive", key, rows, build)
        st["ctx_n"][:, :S] = (ctx0 / ctx0.norm(dim=2, keepdim=True)).float()
        st["lg"].view(B, k, V)[:, 0] = logit0
        st["sel"].zero_(); st["step"].zero_(); st["unfinished"].fill_(1); st["out_ids"].fill_(pad_id)
        st["kstart"].copy_(kstart); st["kstart_k"].copy_(kstart.repeat_interleave(k))
        st["pos0"].copy_(next_pos.repeat_interleave(k))
        stream = lambda: ops.stream(self.device)           # (inside a capture the current stream is the capturing one)
        p = lambda name: st[name].data_ptr()

        def body():
            """One step, every index read on the device."""
            sm = stream()
            check(Lb.emu_contrastive_advance(p("step"), p("pos"), p("slot"), p("pos0"), S, rows, L_new, 0, sm), "emu_contrastive_advance")
            check(Lb.emu_contrastive_pick_bf16(p("lg"), st["lg"].stride(0), V, B, k, L_new, p("sel"), p("out_ids"), B, p("step"),
                                               repetition_penalty, eos_id, min_len, p("cand_ids"), p("cand_p"), sm),
                  "emu_contrastive_pick_bf16")
            ops.embed_gather(st["cand_ids"], self.embed, out=st["hid"])
            check(Lb.emu_llama_forward(self.handle, p("hid"), rows, 1, p("pos"), p("slot"), p("kstart_k"), None,
                                       min(S + L_new, self.s_max), p("fws"), st["fws"].numel(), sm), "emu_llama_forward", self.ctx.handle)
            check(Lb.emu_llama_final_norm(self.handle, p("hid"), p("normed"), rows, sm), "emu_llama_final_norm")
            check(Lb.emu_llama_logits(self.handle, p("hid"), st["hid"].stride(0), rows, p("lg"), st["lg"].stride(0), p("fws"),
                                      st["fws"].numel(), sm), "emu_llama_logits", self.ctx.handle)
            check(Lb.emu_contrastive_score(p("ctx_n"), p("normed"), p("cand_ids"), p("cand_p"), p("kstart"), p("step"), B, k, H, S, L_new,
                                           Lc, alpha, 1.0 - alpha, eos_id, pad_id, p("out_ids"), p("unfinished"), p("sel"), None,
                                           p("ws"), st["ws"].numel(), sm), "emu_contrastive_score")
            check(Lb.emu_llama_contrastive_keep_kv(self.handle, p("sel"), p("step"), k, S, L_new, sm), "emu_llama_contrastive_keep_kv",
                  self.ctx.handle)
            check(Lb.emu_contrastive_advance(p("step"), None, None, None, S, rows, L_new, 1, sm), "emu_contrastive_advance")

        run_polled(lambda i: st["captured"].step(body, use_graph, key), L_new, self.BEAM_POLL, lambda: not bool(st["unfinished"].any()))
        ids = st["out_ids"].t().to(torch.int64)
        self.set_kv_share(0, 0)
        self.ctx.check_p2p()
        # a finished prompt emitted PAD on the device; steps between the last prompt's EOS and the poll that saw it are cut off
        # here: the width is one past the last step at which any prompt was still unfinished, the host loop's rule
        return apply_eos_padding(ids, eos_id, pad_id)

    # ------------------------------------------------------------------ beam search
    @torch.no_grad()
    def beam_search_generate(self, embeds: torch.Tensor, attention_mask: torch.Tensor, num_beams: int,
                             max_new_tokens: int, min_len: int = 1, length_penalty: float = -1.0, eos_id: int = 2,
                             pad_id: int = 32000, do_sample: bool = False, temperature: Optional[float] = None,
                             top_k: Optional[int] = None, top_p: Optional[float] = None,
                             repetition_penalty: float = 1.0, hf_semantics: str = "4.31",
                             trace: Optional[dict] = None, no_repeat_ngram_size: int = 0,
                             num_return_sequences: int = 1, uniforms: Optional[torch.Tensor] = None,
                             device_beam_sampler: bool = False, constraint=None, device_ngram_ban: bool = False) -> torch.Tensor:
        """``lm.generate(inputs_embeds=..., num_beams=N, do_sample=False, early_stopping=False)`` -- the reference's
        DEFAULT decoding mode (num_beams=5, length_penalty=-1, Emu2/emu/emu.py:163-172,213-229).  Restates
        transformers' vectorised beam search: per step keep the 2N best continuations over beams x vocab, the N best
        non-finished ones keep running, finished ones (EOS, or the length limit) compete for the N result slots with
        score / len**length_penalty, and the loop ends when no running beam can beat the worst kept result.
        One prefill for the B prompts; every beam then gets a cache row, of which only the GENERATED slots are its own
        (the prompt's stay in one row per prompt, ``fan_out_kv``) and are re-ordered by beam index each step (gathered on
        the device).  Returns the best sequence per prompt [B, <= max_new_tokens].

        ``do_sample=True`` is the library's *beam-search multinomial sampling*: the per-beam log-probabilities go through
        the logits pipeline (repetition penalty, min length, temperature / top-k / top-p with min_tokens_to_keep = 2)
        BEFORE the beam scores are added, and the 2N continuations are drawn without replacement from
        softmax(accumulated scores) instead of taken by top-k.  ``repetition_penalty`` alone gives penalised beam search.

        ``hf_semantics`` selects the ORDER of the sampling pipeline, which changed between the transformers the reference
        pins (4.31, ``Emu2/requirements.txt:2``) and the one installed here (5.x, the only one that can be run, so the
        only one the golden fixture pins): "4.31" = ``beam_sample`` of that release -- logits processors, THEN the running
        beam scores are added, THEN the warpers (temperature / top-k / top-p) act on the accumulated rows, and the 2N
        draws are sorted by score before the beam bookkeeping (so "only the first N candidates may finish" is by rank, not
        by draw order), and all N beams start at score 0 instead of (0, -1e9, ...); "5.x" = processors and warpers on the per-beam log-probabilities, scores added afterwards, draws
        kept in draw order.  With temperature 1 and no top-k / top-p the two differ only in the sort.
        It also selects the SCORER conventions, in every mode (do_sample or not): "5.x" = the vectorised search of the installed
        library, which the golden fixtures pin (a hypothesis that ends, by EOS or at the length limit, is scored over cur + 1
        tokens; only the first N candidates may end; the early-stopping heuristic looks at the best running beam); "4.31" =
        ``BeamSearchScorer`` / ``BeamHypotheses`` of the pinned release: ``add`` divides an EOS hypothesis by
        ``hyp.shape[-1] ** length_penalty`` where the hypothesis excludes the EOS (cur tokens: with ``inputs_embeds`` the ids
        start empty), ``is_done`` compares the best of ALL 2N candidates at (cur + 1) ** length_penalty with the worst kept
        score, and at the length limit ``finalize`` adds every running beam at L ** length_penalty unless the prompt is done.
        With the reference's default length_penalty = -1 the two rank hypotheses of different lengths differently.  The 4.31
        conventions are restated from that release (it cannot be installed here): UNPINNED beyond a per-hypothesis restatement
        in tests/test_host_logic.py.

        ``no_repeat_ngram_size`` adds the library's NoRepeatNGramLogitsProcessor to the pipeline; ``num_return_sequences`` = n
        returns the n best results of every prompt ([B * n, len], prompt-major: what Emu1's ``num_captions`` asks for,
        Emu1/models/modeling_emu.py:110,173).

        ``uniforms`` [max_new_tokens, B, 2 * num_beams] fp32 in [0, 1) (sampling only): the 2N continuations of step ``cur`` are
        drawn from row ``cur`` of this table by the rule of ``emu_amd/sampling.py::beam_reference_select`` (masses in fp64) instead of
        ``torch.multinomial`` -- another random stream, and the reference of the device loop below.  None (the default): the
        multinomial draw from torch's global generator, as ever.  With a table, ties between candidate scores go to the first in
        candidate order (stable top-k, the device kernels' rule; ``torch.topk`` leaves them open), so that the table alone decides.

        ``device_beam_sampler=True`` / ``device_ngram_ban=True`` (opt-ins): beam-search sampling and penalised beam search, and the ban
        of ``no_repeat_ngram_size``, keep the token loop on the device (``_beam_search_device``).  The sampler's draws come from
        ``uniforms``, by default ONE ``torch.rand(max_new_tokens, B, 2 * num_beams)`` from the global generator up front: seed-stable,
        but a different random stream from ``multinomial``, which is why this is an option.  Which call runs on the device, in which
        variant of the step, what is refused (a ValueError before any device work) and where the host loop takes over, with or
        without a warning: ``genroute.beam_route``.

        ``trace`` (a dict, diagnostics for the tests): receives ``margin`` = the smallest gap seen between the N-th and the
        (N+1)-th running candidate at a pruning step and between the two best final results, and, with a table of uniforms,
        ``draw_margin`` = the smallest distance seen of a draw's ``u * R`` from a boundary between two entries
        (``sampling.beam_draw_margin``).

        ``constraint`` (``emu_amd.constrain.TokenTrie`` or a callable (batch_id, ids generated so far) -> allowed ids, the library's
        ``prefix_allowed_tokens_fn``; Emu1/mm_eval/models/emu.py:96-109 runs it with 5 beams): the per-beam log-probabilities of every
        id that is not allowed become -inf after the processors and ahead of the warpers (the log-softmax is over the whole row).
        Fewer than 2N candidates may then be finite, so every selection goes by the device kernels' rule -- ties, those among -inf
        included, to the lower index (stable top-k) -- and the ``trace`` margins leave out exact ties and non-finite gaps (-inf minus
        -inf)."""
        trie, allow_fn = resolve_constraint(constraint, self.vocab, eos_id, min_len, num_return_sequences)
        kind = genroute.constraint_kind(constraint)
        if genroute.constraint_drops_beam_sampler(kind, device_beam_sampler, do_sample, repetition_penalty):
            warn_once(LlamaEngine, *genroute.BEAM_CONSTRAINT_WARNING)
            device_beam_sampler = False
        ngram = int(no_repeat_ngram_size or 0)
        route = genroute.beam_route(self.vocab, tp_size_of(self), max_new_tokens, num_beams, do_sample, repetition_penalty, ngram,
                                    device_beam_sampler, device_ngram_ban, kind, trace is not None, hasattr(self, "handle"),
                                    hf_semantics, num_return_sequences, embeds.shape[0], None if uniforms is None else uniforms.shape)
        if route.warning is not None:
            warn_once(LlamaEngine, *route.warning)
        B, S, H = embeds.shape
        nb, V, dev = num_beams, self.vocab, self.device
        s_max = self.kv_capacity(S + max_new_tokens)
        hidden, kstart, next_pos = self.prefill(embeds, attention_mask, s_max)
        logits = self.logits(hidden[:, -1, :])                                          # [B, V]
        # rows b*nb .. b*nb + nb - 1 are the beams of prompt b; its keys / values stay in the first of them (fan_out_kv)
        self.fan_out_kv(B, nb, S, s_max)
        kstart_b = kstart.repeat_interleave(nb).contiguous()
        pos = next_pos.repeat_interleave(nb).contiguous()

        max_len = max_new_tokens
        # The deterministic mode (the reference's default) runs each step's selection and bookkeeping in ONE kernel (emu_beam_step_bf16
        # or a variant of it); whatever the route leaves to the host, and any logits but the HIP engine's bf16, keep the torch pipeline
        # below.
        if route.device and not route.sampler and logits.dtype == BF16:
            return self._beam_search_device(logits, B, S, nb, max_len, min_len, length_penalty, eos_id, pad_id, kstart_b, pos,
                                            int(num_return_sequences), hf_semantics == "4.31", trie=trie, **route.device_kw)
        if route.sampler:
            if not hasattr(self, "handle") or logits.dtype != BF16:
                raise RuntimeError("device_beam_sampler needs the HIP engine and its bf16 logits")
            return self._beam_search_device(logits, B, S, nb, max_len, min_len, length_penalty, eos_id, pad_id, kstart_b, pos,
                                            int(num_return_sequences), hf_semantics == "4.31",
                                            sampler=(sample_params(do_sample, temperature, top_k, top_p, repetition_penalty, eos_id,
                                                                   min_len, eos_id, pad_id, min_keep=2), uniforms), **route.device_kw)
        logits = logits.float()
        v431 = hf_semantics == "4.31"
        old = do_sample and v431
        st = beam_start_state(B, nb, max_len, pad_id, dev, equal_start=old)     # (4.31's beam_sample starts EVERY beam at 0)
        hid = torch.empty(B * nb, H, device=dev, dtype=BF16)

        cur = 0
        lp_rows = logits[:, None, :].expand(B, nb, V)                                   # step 0: every beam = the prompt
        margin = draw_margin = float("inf")
        table = uniforms is not None and do_sample
        # with a table the result has to be a function of the table alone, so ties between candidates (the rule, not the exception:
        # at step 0 every beam holds the same hypothesis) go to the first in candidate order, the device kernels' rule
        # ... and so does a constraint: it leaves fewer than 2N finite candidates, and which -inf entry a dead beam is fed must not
        # be left to torch.topk
        stable = table or allow_fn is not None
        # (such exact ties are decided alike on both sides and do not count as a margin; nor does -inf minus -inf)
        gap = (lambda d: float(d.min())) if not stable else \
            (lambda d: float(d.masked_fill((d == 0) | ~torch.isfinite(d), float("inf")).min()))
        while True:
            acc = beam_host_scores(lp_rows, st["running_scores"], st["running_seq"], cur, min_len, eos_id, do_sample, old, temperature,
                                   top_k, top_p, repetition_penalty, ngram, allow_fn).reshape(B, nb * V)
            if do_sample:
                if table:                              # the draws of step cur from row cur of the table (emu_amd/sampling.py)
                    u = uniforms[cur].to(torch.float32)
                    top_idx = beam_reference_select(acc.view(B, nb, V), nb, u, True, "5.x", torch.float64)[1]
                    if trace is not None:
                        draw_margin = min(draw_margin, float(beam_draw_margin(acc.view(B, nb, V), nb, u, top_idx).min()))
                else:
                    top_idx = torch.multinomial(torch.softmax(acc, dim=-1), num_samples=2 * nb)
                top_lp = torch.gather(acc, 1, top_idx)
                if old:                                # ... and its draws are ranked before the beam scorer sees them
                    top_lp, order = torch.sort(top_lp, descending=True, dim=1, stable=table)
                    top_idx = torch.gather(top_idx, 1, order)
            else:
                top_lp, top_idx = beam_topk(acc, 2 * nb, stable)
            toks, flat, _, run_lp = beam_scorer_step(st, top_lp, top_idx, V, cur, max_len, length_penalty, eos_id, v431, stable)
            cur += 1
            if trace is not None and cur < max_len:
                srt = torch.sort(run_lp, dim=1, descending=True)[0]
                margin = min(margin, gap(srt[:, nb - 1] - srt[:, nb]))
            # (every candidate is a hit exactly when the length limit is reached: a beam contributes EOS at most once, so the 2N
            # candidates are never all EOS -- known on the host, one device read per step instead of two)
            if cur >= max_len or not bool(st["open"].any()):
                break
            # advance the model: reorder the cache rows by beam, feed the chosen tokens
            ctx = S + cur - 1
            # beams of one prompt share the prompt's KV slots, so only the generated slots [S, ctx) move with the beam
            # permutation -- a few KB per layer instead of the whole live cache
            if ctx > S:
                self.kcache[:, :, :, S:ctx] = self.kcache[:, flat, :, S:ctx]
                self.vcache[:, :, :, S:ctx] = self.vcache[:, flat, :, S:ctx]
            ops.embed_gather(toks.to(torch.int32).contiguous(), self.embed, out=hid)
            slot = torch.full((B * nb,), ctx, device=dev, dtype=torch.int32)
            self.forward(hid, B * nb, 1, pos, slot, kstart_b, ctx=ctx + 1)
            pos = pos + 1
            lp_rows = self.logits(hid).float().view(B, nb, V)
        sequences, beam_scores, seq_len = st["sequences"], st["beam_scores"], st["seq_len"]
        self.set_kv_share(0, 0)
        nret = int(num_return_sequences)
        out_len = int(seq_len[:, :nret].max().item())
        if trace is not None:
            trace["margin"] = min(margin, gap(beam_scores[:, 0] - beam_scores[:, 1]))
            if table:
                trace["draw_margin"] = draw_margin
        self.ctx.check_p2p()
        if nret == 1:
            return sequences[:, 0, :out_len]
        return sequences[:, :nret, :out_len].reshape(B * nret, out_len)

    BEAM_POLL = 4          # graph-replayed beam steps between two looks at the done flags
    _warned_beam_sampler = False           # one warning per process (beam_search_generate(device_beam_sampler=True))
    _warned_beam_constraint = False        # ... and for a constraint that makes it ignore that flag

    def _beam_search_device(self, logits0: torch.Tensor, B: int, S: int, nb: int, max_len: int, min_len: int,
                            length_penalty: float, eos_id: int, pad_id: int, kstart_b: torch.Tensor, pos: torch.Tensor,
                            nret: int, v431: bool = True, sampler: Optional[tuple] = None,
                            trie: Optional[TokenTrie] = None, ngram: int = 0) -> torch.Tensor:
        """The loop of ``beam_search_generate`` for the deterministic mode, with nothing left on the host but the replay of a
        hipGraph: per step {``emu_beam_advance`` (slot / position of the token to feed from the device-side step counter) ->
        ``emu_llama_beam_reorder_kv`` (the generated KV slots follow the beam permutation) -> embedding gather -> the decoder
        step on prompts x beams rows -> logits -> ``emu_beam_step_bf16`` (log-softmax, 2N-best selection and the scorer's
        bookkeeping, csrc/beam.hip: the same statements as the torch pipeline, which stays the specification and the fallback) ->
        counter + 1}.  The first step (every beam continues the prompt) runs eagerly on the prefill's logits; the graph is
        captured once per (prompt length, batch, beams, limits) on the persistent beam cache and replayed ``BEAM_POLL`` steps at
        a time between two reads of the done flags -- steps replayed beyond the end of the search change nothing (kept results
        are frozen once a prompt is done, and the kernels do nothing from the length limit on).  ``self.beam_graph = False``
        runs the same launches eagerly.

        ``sampler`` = (options, table of uniforms or None) (``beam_search_generate(device_beam_sampler=True)``): the same loop with
        ``emu_beam_sample_step_bf16`` (csrc/beam_sample.hip: beam-search sampling, penalised beam search) as its step.  The table
        is copied into a buffer the captured graph owns, so a call with another table replays the same graph; under the "4.31"
        order with sampling all N running scores start at 0, as on the host.

        ``trie`` (deterministic mode only): the same loop with the step's "trie" variant (``ops.SELECT_ENTRY``).  The beams' nodes
        live in the state and start at the root; the state keeps the trie's tables alive, and their addresses are part of the key,
        so a call with another trie captures anew.

        ``ngram`` > 0 (``device_ngram_ban``; not together with a trie): the "ngram" variant of the step, with or without ``sampler``.
        The n is a scalar of the launch, so it is part of the key."""
        dev, V, rows = self.device, self.vocab, B * nb
        ngram = int(ngram)
        if ngram and trie is not None:
            raise ValueError("the n-gram ban together with a constraint is not built on the device")
        tables = None if trie is None else trie.tables(dev)
        L = lib()
        params = sampler[0] if sampler is not None else None
        sampling = params is not None and bool(params.do_sample)
        opts = None if params is None else (sampling, params.repetition_penalty, params.temperature, params.top_k, params.top_p)
        key = (B, nb, S, self.s_max, max_len, int(min_len), float(length_penalty), int(eos_id), bool(v431), self.kcache.data_ptr(),
               self.mode_epoch, opts, None if tables is None else tuple((t.data_ptr(), t.numel()) for t in tables), ngram)

        def build():
            i32 = dict(dtype=torch.int32, device=dev)
            st = dict(running_seq=torch.empty(B, nb, max_len, **i32), sequences=torch.empty(B, nb, max_len, **i32),
                      running_scores=torch.empty(B, nb, device=dev), beam_scores=torch.empty(B, nb, device=dev),
                      finished=torch.empty(B, nb, dtype=torch.uint8, device=dev), seq_len=torch.empty(B, nb, **i32),
                      still_open=torch.empty(B, dtype=torch.uint8, device=dev), next_tok=torch.empty(rows, **i32),
                      beam_flat=torch.empty(rows, dtype=torch.int64, device=dev),
                      hid=torch.empty(rows, self.cfg.hidden_size, device=dev, dtype=BF16), slot=torch.empty(rows, **i32),
                      pos=torch.empty(rows, **i32), pos0=torch.empty(rows, **i32), kstart=torch.empty(rows, **i32),
                      cur=torch.empty(1, **i32), lg=torch.empty(rows, V, device=dev, dtype=BF16),
                      ws=torch.empty((L.emu_beam_step_workspace_bytes if params is None else L.emu_beam_sample_workspace_bytes)(B, nb, V),
                                     dtype=torch.uint8, device=dev))
            if sampling:
                st["uni"] = torch.empty(max_len, B, 2 * nb, dtype=torch.float32, device=dev)
            if tables is not None:
                st.update(tables=tables, trie=ops.trie_tables(tables), node=torch.empty(rows, **i32))
            return st

        st = self._loop_state("beam", key, rows, build)
        st["running_seq"].fill_(pad_id); st["sequences"].fill_(pad_id)
        st["running_scores"].zero_()
        if not (sampling and v431):
            st["running_scores"][:, 1:] = -1.0e9           # 4.31's beam_sample starts EVERY beam at 0 (the draws tell them apart)
        if sampling:
            table = sampler[1]
            st["uni"].copy_(torch.rand(max_len, B, 2 * nb, dtype=torch.float32, device=dev) if table is None else table)
        st["beam_scores"].fill_(-1.0e9); st["finished"].zero_(); st["seq_len"].zero_(); st["still_open"].fill_(1)
        st["pos0"].copy_(pos); st["kstart"].copy_(kstart_b)
        if tables is not None:
            st["node"].zero_()                             # every beam starts at the root
        stream = lambda: ops.stream(self.device)           # (inside a capture the current stream is the capturing one)

        def beam_step(lg, ld_prompt, ld_beam, cur, cur_dev):
            state = (lg.data_ptr(), ld_prompt, ld_beam, V, B, nb, max_len, cur, cur_dev, int(min_len), eos_id,
                     float(length_penalty), int(v431), st["running_seq"].data_ptr(), st["sequences"].data_ptr(),
                     st["running_scores"].data_ptr(), st["beam_scores"].data_ptr(), st["finished"].data_ptr(),
                     st["seq_len"].data_ptr(), st["still_open"].data_ptr(), st["next_tok"].data_ptr(),
                     st["beam_flat"].data_ptr(), st["ws"].data_ptr(), st["ws"].numel())
            variant = "trie" if tables is not None else "ngram" if ngram else "plain"
            if params is None or tables is not None:
                ops.select_call(L, "beam_step", variant, state, stream(), self.ctx.handle, st.get("trie"), st.get("node"), ngram)
            else:
                draw = (params, int(sampling and v431), st["uni"].data_ptr() if sampling else None, max_len, None, None, 0)
                ops.select_call(L, "beam_sample_step", variant, state + draw, stream(), self.ctx.handle, ngram=ngram)

        def body():
            """One step, every index read on the device."""
            sm = stream()
            check(L.emu_beam_advance(st["cur"].data_ptr(), st["pos"].data_ptr(), st["slot"].data_ptr(), st["pos0"].data_ptr(), S, rows,
                                     max_len, 0, sm), "emu_beam_advance")
            check(L.emu_llama_beam_reorder_kv(self.handle, st["beam_flat"].data_ptr(), st["cur"].data_ptr(), nb, S, max_len, sm),
                  "emu_llama_beam_reorder_kv", self.ctx.handle)
            ops.embed_gather(st["next_tok"], self.embed, out=st["hid"])
            check(L.emu_llama_forward(self.handle, st["hid"].data_ptr(), rows, 1, st["pos"].data_ptr(), st["slot"].data_ptr(),
                                      st["kstart"].data_ptr(), None, min(S + max_len, self.s_max), st["fws"].data_ptr(),
                                      st["fws"].numel(), sm), "emu_llama_forward", self.ctx.handle)
            check(L.emu_llama_logits(self.handle, st["hid"].data_ptr(), st["hid"].stride(0), rows, st["lg"].data_ptr(),
                                     st["lg"].stride(0), st["fws"].data_ptr(), st["fws"].numel(), sm), "emu_llama_logits",
                  self.ctx.handle)
            beam_step(st["lg"], nb * st["lg"].stride(0), st["lg"].stride(0), 0, st["cur"].data_ptr())
            check(L.emu_beam_advance(st["cur"].data_ptr(), None, None, None, S, rows, max_len, 1, sm), "emu_beam_advance")

        beam_step(logits0, logits0.stride(0), 0, 0, None)     # step 0: every beam continues the prompt
        st["cur"].fill_(1)
        use_graph = getattr(self, "beam_graph", True)
        run_polled(lambda i: st["captured"].step(body, use_graph, key), max_len - 1, self.BEAM_POLL,
                   lambda: not bool(st["still_open"].any()))
        self.set_kv_share(0, 0)
        out_len = int(st["seq_len"][:, :nret].max().item())
        self.ctx.check_p2p()
        seqs = st["sequences"].long()
        if nret == 1:
            return seqs[:, 0, :out_len].clone()
        return seqs[:, :nret, :out_len].reshape(B * nret, out_len)


def process_logits(scores: torch.Tensor, generated: torch.Tensor, suppress_eos: bool, eos_id: int, do_sample: bool,
                   temperature: Optional[float] = None, top_k: Optional[int] = None, top_p: Optional[float] = None,
                   repetition_penalty: float = 1.0, min_keep: int = 1, no_repeat_ngram_size: int = 0,
                   allowed: Optional[torch.Tensor] = None) -> torch.Tensor:
    """transformers' logits pipeline for ``generate(inputs_embeds=...)`` in its order: RepetitionPenaltyLogitsProcessor over
    the ids generated so far (with inputs_embeds the prompt contributes no ids), MinLengthLogitsProcessor (EOS -> -inf),
    PrefixConstrainedLogitsProcessor (``allowed`` bool [B, V]: everything else -> -inf; None = no constraint),
    then -- only when sampling -- TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper.  ``scores`` [B, V] fp32,
    ``generated`` [B, n] int64.  ``min_keep`` is the warpers' min_tokens_to_keep (2 under beam search: one EOS id + 1).
    Pure torch: pinned against the library's own processors in tests/test_host_logic.py and tests/test_constrain_host.py."""
    if repetition_penalty != 1.0 and generated.shape[1] > 0:
        g = torch.gather(scores, 1, generated)
        g = torch.where(g < 0, g * repetition_penalty, g / repetition_penalty)
        scores = scores.scatter(1, generated, g)
    if no_repeat_ngram_size and no_repeat_ngram_size > 0:
        scores = ban_repeated_ngrams(scores, generated, int(no_repeat_ngram_size))
    if suppress_eos:
        scores = scores.clone()
        scores[:, eos_id] = -float("inf")
    if allowed is not None:
        scores = scores.masked_fill(~allowed, -float("inf"))
    if do_sample:
        scores = warp_logits(scores, temperature, top_k, top_p, min_keep)
    return scores


def beam_host_scores(lp_rows: torch.Tensor, running_scores: torch.Tensor, running_seq: torch.Tensor, cur: int, min_len: int,
                     eos_id: int, do_sample: bool = False, old: bool = False, temperature: Optional[float] = None,
                     top_k: Optional[int] = None, top_p: Optional[float] = None, repetition_penalty: float = 1.0, ngram: int = 0,
                     allow_fn=None) -> torch.Tensor:
    """The score half of a beam-search step on the host, ``acc`` [B, nb, V] fp32: log-softmax of the beams' logit rows ``lp_rows``
    [B, nb, V], ``process_logits`` (min_keep = 2) over the ``cur`` ids every beam has generated (``running_seq`` [B, nb, >= cur]), the
    running scores added.  ``old`` (4.31's ``beam_sample``): the warpers act on the ACCUMULATED scores instead of the log-probabilities.
    With no processor on, the pipeline is skipped and only the min-length suppress of EOS remains.  ``allow_fn``: the constraint as
    a callable (batch_id, ids) -> allowed ids, ``resolve_constraint``'s."""
    B, nb, V = lp_rows.shape
    log_probs = torch.log_softmax(lp_rows, dim=-1)
    if do_sample or repetition_penalty != 1.0 or ngram or allow_fn is not None:
        gen = running_seq[:, :, :cur].reshape(B * nb, cur)
        log_probs = process_logits(log_probs.reshape(B * nb, V), gen, cur < min_len,
                                   eos_id, do_sample and not old, temperature, top_k, top_p, repetition_penalty,
                                   min_keep=2, no_repeat_ngram_size=ngram,
                                   allowed=None if allow_fn is None else allowed_mask(allow_fn, gen, nb, V)).view(B, nb, V)
    elif cur < min_len:
        log_probs = log_probs.clone()
        log_probs[..., eos_id] = -float("inf")
    acc = log_probs + running_scores[:, :, None]
    if old:                                    # 4.31 beam_sample: the warpers see the ACCUMULATED scores
        acc = warp_logits(acc.reshape(B * nb, V), temperature, top_k, top_p, min_keep=2).view(B, nb, V)
    return acc


def tp_size_of(engine) -> int:
    """The ranks an engine is sharded over (the CPU stand-in of the tests has a context without the field: one)."""
    return getattr(engine.ctx, "tp_size", 1)


def resolve_constraint(constraint, vocab: int, eos_id: int, min_len: int, num_return_sequences: int = 1):
    """``constraint`` of the generate loops -> (trie or None, callable or None).  A ``TokenTrie`` is checked against the call (a
    ValueError before any device work) and may run on the device; a callable with the library's ``prefix_allowed_tokens_fn``
    signature (batch_id, ids generated so far) -> list always keeps the host loop."""
    if constraint is None:
        return None, None
    if isinstance(constraint, TokenTrie):
        if constraint.vocab != int(vocab) or constraint.eos_id != int(eos_id):
            raise ValueError(f"constraint: the trie was built for vocabulary {constraint.vocab} and EOS {constraint.eos_id}, the call "
                             f"has vocabulary {vocab} and EOS {eos_id}")
        if int(min_len) > constraint.min_depth:
            raise ValueError(f"constraint: min_len {min_len} is above the trie's shortest sequence ({constraint.min_depth} tokens "
                             "ahead of its EOS): with EOS suppressed nothing would be allowed there")
        if int(num_return_sequences) > constraint.count:
            raise ValueError(f"constraint: num_return_sequences {num_return_sequences} is above the trie's {constraint.count} sequences")
        return constraint, constraint.as_callable()
    if callable(constraint):
        return None, constraint
    raise TypeError("constraint must be an emu_amd.constrain.TokenTrie or a callable (batch_id, ids) -> list of allowed ids")


def allowed_mask(fn, generated: torch.Tensor, rows_per_prompt: int, vocab: int) -> torch.Tensor:
    """[rows, vocab] bool from ``fn(batch_id, ids)`` over the rows of ``generated`` [rows, n] (the ids generated so far; batch_id =
    row // rows_per_prompt, as the library's PrefixConstrainedLogitsProcessor numbers the beams of a prompt).  An empty answer is
    the library's ValueError."""
    mask = torch.zeros(generated.shape[0], vocab, dtype=torch.bool)
    for r, ids in enumerate(generated.cpu()):
        ok = fn(r // rows_per_prompt, ids)
        if len(ok) == 0:
            raise ValueError(f"`prefix_allowed_tokens_fn` returned an empty list for batch ID {r // rows_per_prompt}. This means that "
                             "the constraint is unsatisfiable. Please check your implementation of `prefix_allowed_tokens_fn`")
        mask[r, torch.as_tensor(list(ok), dtype=torch.int64)] = True
    return mask.to(generated.device)


def ban_repeated_ngrams(scores: torch.Tensor, generated: torch.Tensor, n: int) -> torch.Tensor:
    """transformers' NoRepeatNGramLogitsProcessor (after the repetition penalty, ahead of MinLength in the library's processor
    list): a token that would complete an n-gram already present in the row's generated ids gets -inf.  ``generated`` [B, cur]
    (with inputs_embeds the prompt contributes no ids).  Host loop: rows x cur is a few hundred at most."""
    B, cur = generated.shape
    if cur + 1 < n:
        return scores
    scores = scores.clone()
    gen = generated.tolist()
    for b in range(B):
        row = gen[b]
        prefix = tuple(row[cur - (n - 1):]) if n > 1 else ()
        for i in range(cur - n + 1):
            if tuple(row[i:i + n - 1]) == prefix:
                scores[b, row[i + n - 1]] = -float("inf")
    return scores


def warp_logits(scores: torch.Tensor, temperature: Optional[float] = None, top_k: Optional[int] = None,
                top_p: Optional[float] = None, min_keep: int = 1) -> torch.Tensor:
    """transformers' sampling warpers in their order: TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper."""
    if temperature is not None and temperature != 1.0:
        scores = scores / temperature
    if top_k is not None and top_k > 0:
        kth = torch.topk(scores, min(max(top_k, min_keep), scores.shape[-1]))[0][..., -1, None]
        scores = scores.masked_fill(scores < kth, -float("inf"))
    if top_p is not None and top_p < 1.0:
        srt, idx = torch.sort(scores, descending=False)
        cum = srt.softmax(dim=-1).cumsum(dim=-1)
        remove = cum <= (1 - top_p)
        remove[..., -min_keep:] = False
        scores = scores.masked_fill(remove.scatter(1, idx, remove), -float("inf"))
    return scores


def apply_eos_padding(ids: torch.Tensor, eos_id: int, pad_id: int) -> torch.Tensor:
    """HF greedy bookkeeping: after a row emits EOS it emits PAD; generation stops once every row is finished."""
    ids = ids.clone()
    B, n = ids.shape
    is_eos = ids == eos_id
    first = torch.where(is_eos.any(dim=1), is_eos.float().argmax(dim=1), torch.full((B,), n, device=ids.device))
    ar = torch.arange(n, device=ids.device)[None]
    ids[ar > first[:, None]] = pad_id
    keep = int(min(n, int(first.max().item()) + 1))
    return ids[:, :keep]


def sample_params(do_sample: bool, temperature, top_k, top_p, repetition_penalty: float, suppress_id: Optional[int], min_len: int,
                  eos_id: int, pad_id: int, min_keep: int = 1) -> SampleParamsC:
    """The options of ``emu_sample_bf16`` / ``emu_llama_sample_step`` (include/emu_hip.h: emu_sample_params) from generate's."""
    return SampleParamsC(float(repetition_penalty), -1 if suppress_id is None else int(suppress_id), int(min_len), int(bool(do_sample)),
                         1.0 if temperature is None else float(temperature), 0 if top_k is None else int(top_k),
                         1.0 if top_p is None else float(top_p), int(min_keep), int(eos_id), int(pad_id))


class GreedyState:
    """Device-resident state of the greedy token loop (see emu_llama_greedy_step)."""

    def __init__(self, eng: LlamaEngine, B: int, first_ids: torch.Tensor, next_pos: torch.Tensor, S: int,
                 kstart: torch.Tensor, out_ids: torch.Tensor):
        self.eng, self.B = eng, B
        dev = eng.device
        self.cur = first_ids.to(torch.int32).clone()
        self.pos = next_pos.to(torch.int32).clone()
        self.slot = torch.full((B,), S, device=dev, dtype=torch.int32)
        self.ctx = torch.tensor([S + 1], device=dev, dtype=torch.int32)
        self.step_idx = torch.tensor([1], device=dev, dtype=torch.int32)   # out_ids[0] already holds first_ids
        self.kstart = kstart
        self.out_ids = out_ids
        self.hidden = torch.empty(B, eng.cfg.hidden_size, device=dev, dtype=BF16)
        self.logits = torch.empty(B, eng.vocab, device=dev, dtype=BF16)
        self.ws = eng._workspace(B, 1)
        self.captured = CapturedStep()

    def reset(self, first_ids: torch.Tensor, next_pos: torch.Tensor, S: int) -> None:
        """Rewind the device-side state to the end of the prompt, in place (a captured graph stays valid)."""
        self.cur.copy_(first_ids.to(torch.int32))
        self.pos.copy_(next_pos.to(torch.int32))
        self.slot.fill_(S)
        self.ctx.fill_(S + 1)
        self.step_idx.fill_(1)

    def step(self) -> None:
        e = self.eng
        check(lib().emu_llama_greedy_step(e.handle, self.B, self.cur.data_ptr(), self.pos.data_ptr(),
                                          self.slot.data_ptr(), self.kstart.data_ptr(), self.ctx.data_ptr(),
                                          self.step_idx.data_ptr(), self.out_ids.data_ptr(), e.s_max,
                                          self.hidden.data_ptr(), self.logits.data_ptr(), self.logits.stride(0),
                                          self.ws.data_ptr(), self.ws.numel(), ops.stream(e.device)),
              "emu_llama_greedy_step", e.ctx.handle)

    def step_graph(self) -> None:
        """One step from a hipGraph captured on first use and anew after a mode switch (launch-bound at TP>1: ~550 launches/token).
        The kernels read the step index from the device, so the one captured step serves every token."""
        self.captured.step(self.step, True, self.eng.mode_epoch)

    def step_eager_suppress(self, suppress: int) -> None:
        """A step with a suppressed id (min_length > 1): same as step() but argmax masks ``suppress``."""
        e = self.eng
        ops.embed_gather(self.cur, e.embed, out=self.hidden)
        e.forward(self.hidden, self.B, 1, self.pos, self.slot, self.kstart, ctx=e.s_max, ctx_dev=self.ctx)
        e.logits(self.hidden, out=self.logits)
        ops.argmax(self.logits, suppress_id=suppress, out=self.cur)
        st = int(self.step_idx.item())
        self.out_ids[st] = self.cur
        self.pos += 1
        self.slot += 1
        self.ctx += 1
        self.step_idx += 1


class SampleState(GreedyState):
    """Device-resident state of the sampling / penalised-greedy token loop (see emu_llama_sample_step): GreedyState's arrays, the
    rows' ``unfinished`` flags, the table of uniforms and the options.  ``out_ids`` [max_new, B] is also the penalty's history.
    ``step_graph`` is GreedyState's: the min-length suppress and the history length, too, come from the device-side step index."""

    def __init__(self, eng: "LlamaEngine", B: int, next_pos: torch.Tensor, S: int, kstart: torch.Tensor, out_ids: torch.Tensor,
                 uniforms: Optional[torch.Tensor], params: SampleParamsC, trie_tables: Optional[tuple] = None, ngram: int = 0):
        super().__init__(eng, B, torch.zeros(B, device=eng.device, dtype=torch.int32), next_pos, S, kstart, out_ids)
        # constraint: the tables (kept alive here for as long as a captured graph holds their addresses), their C view, and the rows'
        # nodes, every row at the root
        self.trie_tables = trie_tables
        self.trie = None if trie_tables is None else ops.trie_tables(trie_tables)
        self.node = None if trie_tables is None else torch.zeros(B, device=eng.device, dtype=torch.int32)
        # no-repeat n-gram ban (0 = off): a scalar of the step's launch, so a captured step holds it -- it is part of the graph's key
        self.ngram = int(ngram)
        if self.ngram and trie_tables is not None:
            raise ValueError("the n-gram ban together with a constraint is not built on the device")
        self.step_idx.zero_()                              # no token yet: first() draws it
        self.unfinished = torch.ones(B, device=eng.device, dtype=torch.int32)
        self.uniforms, self.params = uniforms, params
        self.max_new = out_ids.shape[0]

    def first(self) -> None:
        """The first token, from ``self.logits`` (the prefill's last rows): step 0 of the table."""
        ops.sample(self.logits, self.step_idx, self.params, self.cur, hist=self.out_ids, uniforms=self.uniforms,
                   unfinished=self.unfinished, trie=self.trie, node=self.node, ngram=self.ngram or None)
        self.out_ids[0] = self.cur
        self.step_idx.fill_(1)

    def step(self) -> None:
        e = self.eng
        args = (e.handle, self.B, self.cur.data_ptr(), self.pos.data_ptr(), self.slot.data_ptr(), self.kstart.data_ptr(),
                self.ctx.data_ptr(), self.step_idx.data_ptr(), self.out_ids.data_ptr(), self.max_new, e.s_max, self.hidden.data_ptr(),
                self.logits.data_ptr(), self.logits.stride(0), self.ws.data_ptr(), self.ws.numel(), ops._p(self.uniforms),
                self.unfinished.data_ptr(), C.byref(self.params))
        variant = "ngram" if self.ngram else "plain" if self.trie is None else "trie"
        ops.select_call(lib(), "sample_step", variant, args, ops.stream(e.device), e.ctx.handle, self.trie, self.node, self.ngram)

    def step_graph(self) -> None:
        """GreedyState's, the n of the ban beside the mode epoch in the key: the captured launch holds that scalar."""
        self.captured.step(self.step, True, (self.eng.mode_epoch, self.ngram))


class ScoreState(GreedyState):
    """Device-resident state of the teacher-forced loop (see emu_llama_score_step): GreedyState's arrays without ``out_ids`` -- the
    tokens are given: ``targets`` int32 [T, B], the ignored ones negative -- and the results ``lp`` / ``lse`` / ``top1`` [T, B], row 0
    of which the caller filled from the prefill's logits.  ``step_graph`` is GreedyState's: the step index, and with it the row of
    targets and results, comes from the device."""

    def __init__(self, eng: "LlamaEngine", B: int, first_ids: torch.Tensor, next_pos: torch.Tensor, S: int, kstart: torch.Tensor,
                 targets: torch.Tensor, res: Dict[str, torch.Tensor]):
        super().__init__(eng, B, first_ids, next_pos, S, kstart, None)
        self.targets, self.res, self.T = targets, res, targets.shape[0]

    def step(self) -> None:
        e = self.eng
        check(lib().emu_llama_score_step(e.handle, self.B, self.cur.data_ptr(), self.pos.data_ptr(), self.slot.data_ptr(),
                                         self.kstart.data_ptr(), self.ctx.data_ptr(), self.step_idx.data_ptr(),
                                         self.targets.data_ptr(), self.T, e.s_max, self.hidden.data_ptr(), self.logits.data_ptr(),
                                         self.logits.stride(0), self.ws.data_ptr(), self.ws.numel(), self.res["lp"].data_ptr(),
                                         self.res["lse"].data_ptr(), self.res["top1"].data_ptr(), ops.stream(e.device)),
              "emu_llama_score_step", e.ctx.handle)
