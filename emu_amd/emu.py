"""``EmuModel`` -- drop-in for the reference's ``Emu2/emu/emu.py:19-235`` on MI355X.

Same constructor configs, attribute names, method names, keyword arguments, defaults and return types
(``encode_image`` / ``generate`` / ``generate_image``), and the same state-dict keys
(``visual.*``, ``decoder.lm.model.*``, ``decoder.lm.lm_head.weight``, ``project_up.weight``,
``project_down.weight``).  All arithmetic runs in libemu_hip.so (hand-written gfx950 kernels); this file is
host orchestration only.  ``generate_image`` uses the KV-cached formulation (1 prefill + n_query-1 cached steps)
that is mathematically identical to the reference's 64 uncached forwards.
"""
from __future__ import annotations

import os
from typing import Dict, Iterable, List, Optional, Tuple

import torch

from . import genroute, ops
from .conf.emu_conf import CLIPVisionCfg, LlamaCfg, TextDecoderCfg
from .constants import *  # noqa: F401,F403  (re-exported like the reference module does)
from .constants import (DEFAULT_gIMG_TOKEN, DEFAULT_IMAGE_TOKEN, DEFAULT_IMG_END_TOKEN, DEFAULT_IMG_PLACEHOLDER,
                        DEFAULT_IMG_TOKEN, DEFAULT_VID_PLACEHOLDER, EOS_TOKEN_ID, IMAGE_TOKEN_ID, IMG_TOKEN_ID,
                        PAD_TOKEN_ID, VOCAB_EMU2, VOCAB_EMU2_CHAT, gIMG_TOKEN_ID, special_tokens_list)
from .constrain import pop_constraint
from .device_loop import CapturedStep, option_or_env
from .llama import EmuHipContext, LlamaEngine, tp_size_of

BF16 = torch.bfloat16


def build_tokenizer(llama_config_path: str, instruct: bool):
    """LlamaTokenizer + the Emu special tokens, exactly as the reference builds it (Emu2/emu/lm.py:40-63).
    Pure host logic; needs ``tokenizer.model`` in ``llama_config_path`` (ship it with the checkpoint)."""
    import transformers
    from .constants import DEFAULT_BOS_TOKEN, DEFAULT_EOS_TOKEN, DEFAULT_PAD_TOKEN
    if not os.path.exists(os.path.join(llama_config_path, "tokenizer.model")):
        raise FileNotFoundError(
            f"no tokenizer.model under {llama_config_path!r}: point TextDecoderCfg.llama_config_path (or the "
            "EMU_LLAMA_CONFIG environment variable) at the checkpoint's llama_config directory")
    tok = transformers.LlamaTokenizer.from_pretrained(llama_config_path)
    tok.add_special_tokens(dict(pad_token=DEFAULT_PAD_TOKEN, bos_token=DEFAULT_BOS_TOKEN, eos_token=DEFAULT_EOS_TOKEN,
                                additional_special_tokens=special_tokens_list(instruct)))
    tok.truncation_side = tok.padding_side = "left"          # emu.py:58
    return tok


class _Decoder:
    """Stand-in for ``EmuForClsAndRegression`` (Emu2/emu/lm.py:30-102): exposes ``.lm`` and ``.tokenizer``."""

    def __init__(self, lm: LlamaEngine, cfg: TextDecoderCfg):
        self.lm = lm
        self.args = cfg
        self._tokenizer = None
        self.image_token_id = IMAGE_TOKEN_ID
        self.img_token_id = IMG_TOKEN_ID

    @property
    def tokenizer(self):
        if self._tokenizer is None:
            path = os.environ.get("EMU_LLAMA_CONFIG", self.args.llama_config_path)
            self._tokenizer = build_tokenizer(path, self.args.instruct)
        return self._tokenizer

    @tokenizer.setter
    def tokenizer(self, tok):
        self._tokenizer = tok

    def get_num_layers(self):
        return self.lm.cfg.num_hidden_layers


class EmuModel:
    def __init__(self, vision_cfg: CLIPVisionCfg = CLIPVisionCfg(), text_decoder_cfg: TextDecoderCfg = TextDecoderCfg(),
                 *, llama_cfg: Optional[LlamaCfg] = None, device="cuda", tp_rank: int = 0, tp_size: int = 1,
                 ctx: Optional[EmuHipContext] = None, vit_token_parallel: Optional[bool] = None,
                 device_sampler: Optional[bool] = None, device_beam_sampler: Optional[bool] = None,
                 device_contrastive: Optional[bool] = None, device_ngram_ban: Optional[bool] = None):
        """``device_sampler`` (default: the ``EMU_DEVICE_SAMPLER`` environment variable, off unless "1"): sampling and penalised
        greedy generation (one beam) keep their token loop on the device (``LlamaEngine.sample_generate(device_sampler=True)``:
        uniforms drawn once up front, so a different random stream from the default's ``torch.multinomial``).

        ``device_beam_sampler`` (default: the ``EMU_DEVICE_BEAM_SAMPLER`` environment variable, off unless "1"; an option of its
        own, ``device_sampler`` does not switch it on): beam search with ``do_sample`` or a repetition penalty keeps its token loop
        on the device too (``LlamaEngine.beam_search_generate(device_beam_sampler=True)``: one table of uniforms up front, again
        another random stream than ``torch.multinomial``).

        ``device_contrastive`` (default: the ``EMU_DEVICE_CONTRASTIVE`` environment variable, off unless "1"; an option of its own
        beside the two above): contrastive search (``penalty_alpha``, ``top_k``) keeps its token loop on the device
        (``LlamaEngine.contrastive_generate(device_contrastive=True)``: candidates, degeneration penalty, selection and the KV copy
        in kernels of csrc/contrastive.hip, replayed from one hipGraph with ``use_graph``).  Its sums are fp32 in a fixed order, so
        a choice the host loop decides by less than its own rounding may fall the other way.

        ``device_ngram_ban`` (default: the ``EMU_DEVICE_NGRAM_BAN`` environment variable, off unless "1"): with
        ``no_repeat_ngram_size > 0`` the two device samplers above stay on instead of handing the call to the host loop, and the
        deterministic beam search keeps its device loop: the ban runs inside the selection kernels
        (``LlamaEngine.sample_generate`` / ``beam_search_generate(device_ngram_ban=True)``).  It switches no sampler on by itself.

        ``vit_token_parallel`` (default: the ``EMU_VIT_TOKEN_PARALLEL`` environment variable, off unless "1"): under tensor
        parallelism a prompt with ONE image splits its ViT encode across the ranks by token rows (``encode_image``) instead of every
        rank encoding the whole image.  Opt-in until a multi-GPU node has measured it."""
        from .vit import VitEngine
        self.vision_cfg, self.text_decoder_cfg = vision_cfg, text_decoder_cfg
        if llama_cfg is None:
            llama_cfg = LlamaCfg.from_json(text_decoder_cfg.llama_config_path)
        self.llama_cfg = llama_cfg
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.ctx = ctx or EmuHipContext(dev, tp_rank, tp_size)
        self.vocab = VOCAB_EMU2_CHAT if text_decoder_cfg.instruct else VOCAB_EMU2
        self.visual = VitEngine(vision_cfg, self.ctx)
        self.decoder = _Decoder(LlamaEngine(llama_cfg, self.vocab, self.ctx), text_decoder_cfg)
        self.project_up: Optional[torch.Tensor] = None       # [hidden, width]   EVA -> LM   (emu.py:53)
        self.project_down: Optional[torch.Tensor] = None     # [width, hidden]   LM -> EVA   (emu.py:55)
        self.n_query = vision_cfg.n_query
        self.v_query = vision_cfg.v_query
        self.image_placeholder = DEFAULT_IMG_TOKEN + DEFAULT_IMAGE_TOKEN * self.n_query + DEFAULT_IMG_END_TOKEN
        self.video_placeholder = DEFAULT_IMG_TOKEN + DEFAULT_gIMG_TOKEN * self.v_query + DEFAULT_IMG_END_TOKEN
        self.use_graph = False
        self.vit_token_parallel = option_or_env(vit_token_parallel, "EMU_VIT_TOKEN_PARALLEL")
        self._vit_tp_ready = False
        self.device_sampler = option_or_env(device_sampler, "EMU_DEVICE_SAMPLER")
        self.device_beam_sampler = option_or_env(device_beam_sampler, "EMU_DEVICE_BEAM_SAMPLER")
        self.device_contrastive = option_or_env(device_contrastive, "EMU_DEVICE_CONTRASTIVE")
        self.device_ngram_ban = option_or_env(device_ngram_ban, "EMU_DEVICE_NGRAM_BAN")
        # beam-search conventions: the transformers release the reference pins (Emu2/requirements.txt:2); "5.x" = the installed
        # library's vectorised search, the one the golden fixtures can pin (LlamaEngine.beam_search_generate)
        self.hf_semantics = "4.31"

    _warned_431 = False          # one warning per process: the default beam mode has no library vector (generate_ids)

    # ------------------------------------------------------------------ nn.Module-like surface
    def device(self, module=None):
        return self.ctx.device

    def dtype(self, module=None):
        return BF16

    def eval(self):
        return self

    def load_state_dict(self, state_dict, strict: bool = True):
        return self.load_weights(state_dict.items(), strict=strict)

    def load_weights(self, items: Iterable[Tuple[str, torch.Tensor]], strict: bool = True):
        """Streaming loader (reference key names); tensors may live on CPU or GPU, any float dtype."""
        unexpected = []
        for name, t in items:
            if name.startswith("visual."):
                used = self.visual.load_tensor(name[len("visual."):], t)
            elif name.startswith("decoder.lm."):
                used = self.decoder.lm.load_tensor(name[len("decoder.lm."):], t)
            elif name == "project_up.weight":
                self.project_up, used = t.to(self.ctx.device, BF16).contiguous(), True
            elif name == "project_down.weight":
                self.project_down, used = t.to(self.ctx.device, BF16).contiguous(), True
            else:
                used = False
            if not used and not name.endswith("rotary_emb.inv_freq"):
                unexpected.append(name)
        missing = []
        if not self.visual.ready:
            missing.append("visual.*")
        if not self.decoder.lm.ready:
            missing.append("decoder.lm.*")
        else:
            self.decoder.lm.pack_bf16_default()                # the 13-bit sets of qkv, gate/up and lm_head (bf16pack.default_pack)
        if self.project_up is None:
            missing.append("project_up.weight")
        if self.project_down is None:
            missing.append("project_down.weight")
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for EmuModel: missing {missing}, unexpected {unexpected}")
        return missing, unexpected

    # ------------------------------------------------------------------ encode_image (emu.py:77-90)
    @torch.no_grad()
    def encode_image(self, image: torch.Tensor, *, n_query=None):
        n_query = n_query if n_query is not None else self.n_query
        g = self.vision_cfg.grid
        stride = int(g // (n_query ** 0.5))

        def enc(img):
            return ops.avgpool_tokens(self.visual(img), g, stride)    # [k, 1+g*g, C] -> [k, n_query, C]
        # opt-in: ONE image is split across the tensor-parallel ranks by token rows (every rank returns the same tokens)
        if self.ctx.tp_size > 1 and image.shape[0] == 1 and self.vit_token_parallel and self._image_parallel_ok():
            self._init_vit_token_parallel()
            tokens = self.visual.forward_token_parallel(image)
            self.visual.check_exchange()
            return ops.avgpool_tokens(tokens, g, stride)
        # tensor-parallel ranks split the IMAGES of a prompt between them (the ViT is replicated) and all-gather the pooled tokens
        if self.ctx.tp_size > 1 and image.shape[0] >= 2 and self._image_parallel_ok():
            from .tp import image_parallel_encode
            return image_parallel_encode(image, enc, self.ctx.tp_rank, self.ctx.tp_size, self._all_gather)
        return enc(image)

    def _init_vit_token_parallel(self) -> None:
        """First token-parallel encode (collective, like the encode itself): the exchange regions' IPC handles go round through
        torch.distributed; the exchange takes the form the decoder's P2P all-reduce cleared (fence-free only after its soak)."""
        if self._vit_tp_ready:
            return
        import torch.distributed as dist

        def allgather(b):
            box = [None] * dist.get_world_size()
            dist.all_gather_object(box, b)
            return box
        self.visual.init_token_parallel(self.ctx.tp_rank, self.ctx.tp_size, allgather, fenced=not self.ctx.p2p_fence_free)
        self._vit_tp_ready = True

    def _image_parallel_ok(self) -> bool:
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized() and dist.get_world_size() == self.ctx.tp_size

    @staticmethod
    def _all_gather(t: torch.Tensor):
        """torch.distributed.all_gather of a device tensor: RCCL over xGMI; under a gloo group (ranks sharing one GPU in the
        validation runs) the exchange goes through the host."""
        import torch.distributed as dist
        if dist.get_backend() == "gloo":
            parts = [torch.empty_like(t, device="cpu") for _ in range(dist.get_world_size())]
            dist.all_gather(parts, t.cpu())
            return [p.to(t.device) for p in parts]
        parts = [torch.empty_like(t) for _ in range(dist.get_world_size())]
        dist.all_gather(parts, t)
        return parts

    def _project(self, x2d: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        return ops.linear(x2d.contiguous(), w)

    def _prompt_embeds(self, input_ids: torch.Tensor, image: Optional[torch.Tensor], n_query: Optional[int],
                       token_id: int = IMAGE_TOKEN_ID, embeds: Optional[torch.Tensor] = None) -> torch.Tensor:
        """embed_tokens + masked overwrite of the <image> rows with project_up(encode_image) (emu.py:193-203)."""
        lm = self.decoder.lm
        B, S = input_ids.shape
        x = lm.embed_tokens(input_ids).view(B * S, -1) if embeds is None else embeds
        if image is not None:
            e = self.encode_image(image, n_query=n_query)
            e = self._project(e.view(-1, e.shape[-1]), self.project_up)
            rows = torch.nonzero(input_ids.reshape(-1).to(self.ctx.device) == token_id).reshape(-1).to(torch.int32)
            if rows.numel() != e.shape[0]:
                raise ValueError(f"shape mismatch: {rows.numel()} image slots in the prompt cannot take "
                                 f"{e.shape[0]} image embedding rows")
            ops.scatter_rows(e, rows.contiguous(), x)
        return x

    # ------------------------------------------------------------------ generate (emu.py:155-235)
    @torch.no_grad()
    def generate_ids(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, image: Optional[torch.Tensor] = None,
                     video: Optional[torch.Tensor] = None, max_new_tokens: int = 10, min_len: int = 1,
                     stop_on_eos: bool = True, num_beams: int = 1, length_penalty: float = -1.0, do_sample: bool = False,
                     temperature=None, top_k=None, top_p=None, repetition_penalty: float = 1.0,
                     penalty_alpha: Optional[float] = None, no_repeat_ngram_size: int = 0,
                     num_return_sequences: int = 1, hf_semantics: Optional[str] = None,
                     eos_token_id: Optional[int] = None, min_new_tokens: Optional[int] = None,
                     constraint=None, prompt_lookup_num_tokens: int = 0, max_matching_ngram_size: int = 2) -> torch.Tensor:
        """``generate`` at the token-id level: returns the NEW ids [B, n] (what HF returns for inputs_embeds).  Which engine
        method runs, and with which of this model's opt-ins: ``genroute.model_route``.
        ``hf_semantics`` (default: ``self.hf_semantics`` = "4.31", the transformers release the reference pins): beam-search
        conventions, see ``LlamaEngine.beam_search_generate``; "5.x" = the installed library the golden fixtures come from.
        The two releases also differ in what ``min_length=min_len`` (emu.py:220) enforces when generation is driven by
        ``inputs_embeds``: 4.31 compares against the EMPTY id sequence (min_len new tokens), 5.x subtracts the prompt length first
        (``_prepare_generated_length``: the default min_len = 1 then enforces nothing and EOS may be the first token -- pinned by
        the real reference's ids in tests/golden/generate_beam_eos_tiny.npz).  ``eos_token_id`` / ``min_new_tokens``: the options
        of that name the reference forwards to ``lm.generate`` through ``**kwargs`` (emu.py:175,228).  ``constraint``: an
        ``emu_amd.constrain.TokenTrie`` or a callable with the library's ``prefix_allowed_tokens_fn`` signature.
        ``prompt_lookup_num_tokens`` = k > 0 (with ``max_matching_ngram_size``; the library's options of these names, off by default):
        prompt-lookup speculative greedy decoding, ``LlamaEngine.lookup_generate`` -- one prompt, plain greedy search, 1 <= k <= 7, no
        tensor parallelism; anything else is ``genroute.lookup_route``'s ValueError, before any device work.  On a model made with
        ``device_sampler=True`` it also takes one beam that samples or carries a repetition penalty (``speculate.row_select``)."""
        B, S = input_ids.shape
        lookup = dict(prompt_lookup_num_tokens=int(prompt_lookup_num_tokens), max_matching_ngram_size=int(max_matching_ngram_size)) \
            if prompt_lookup_num_tokens else {}
        if lookup:
            genroute.lookup_route(int(prompt_lookup_num_tokens), B, tp_size_of(self.decoder.lm), num_beams, do_sample, top_k, penalty_alpha,
                                  repetition_penalty, int(no_repeat_ngram_size or 0), int(num_return_sequences), constraint,
                                  device_sampler=genroute.model_flags(self)["device_sampler"])
        sem = hf_semantics or getattr(self, "hf_semantics", "4.31")
        eos = EOS_TOKEN_ID if eos_token_id is None else int(eos_token_id)
        if min_new_tokens is not None:
            min_len = max(int(min_len), int(min_new_tokens)) if sem == "4.31" else int(min_new_tokens)
        elif sem != "4.31":
            min_len = max(int(min_len) - S, 0)
        if num_beams > 1 and sem == "4.31" and min_len < 1:
            # 4.31's BeamHypotheses.add scores an EOS hypothesis over hyp.shape[-1] ** length_penalty with the EOS excluded: a
            # hypothesis that ends at the first step (cur == 0) has length 0 (0 ** lp), a case that release only avoids through its
            # min_length = 1 default; the restatement here does not define it either (checked before any device work)
            raise ValueError("beam search under hf_semantics='4.31' needs min_len >= 1 (an EOS hypothesis of length 0 is scored over "
                             "0 ** length_penalty in that release); pass min_len >= 1 or hf_semantics='5.x'")
        x = self._prompt_embeds(input_ids, image, self.n_query, IMAGE_TOKEN_ID)
        if video is not None:
            x = self._prompt_embeds(input_ids, video, self.v_query, gIMG_TOKEN_ID, embeds=x)
        ngram, nret = int(no_repeat_ngram_size or 0), int(num_return_sequences)
        method, routing = genroute.model_route(genroute.model_flags(self), num_beams, do_sample, top_k, penalty_alpha,
                                               repetition_penalty, ngram, nret, constraint, **lookup)
        lm, x = self.decoder.lm, x.view(B, S, -1)
        if method == "lookup_generate":
            if "do_sample" in routing:                         # one beam that samples or penalises (device_sampler): the warpers' values
                routing.update(temperature=temperature, top_k=top_k, top_p=top_p)
            return lm.lookup_generate(x, attention_mask, input_ids, max_new_tokens, min_len=min_len, eos_id=eos, pad_id=PAD_TOKEN_ID,
                                      stop_on_eos=stop_on_eos, **routing)
        if method == "contrastive_generate":
            return lm.contrastive_generate(x, attention_mask, max_new_tokens, float(penalty_alpha), int(top_k), min_len,
                                           repetition_penalty, eos_id=eos, pad_id=PAD_TOKEN_ID, **routing)
        if method == "beam_search_generate":
            if sem == "4.31" and not EmuModel._warned_431:
                # honesty in code, not only in INTEGRATION.md: this is the DEFAULT mode (emu.py:163-172: 5 beams, length_penalty -1)
                EmuModel._warned_431 = True
                import warnings
                warnings.warn("emu_amd: beam search under hf_semantics='4.31' (the transformers release the reference pins) follows a "
                              "RESTATEMENT of that release's BeamSearchScorer: no vector from the 4.31 library itself exists in "
                              "tests/golden/ (the library is not installable offline).  hf_semantics='5.x' is the mode pinned to the "
                              "installed library's ids; the two differ only where a hypothesis ends on EOS (INTEGRATION.md).",
                              stacklevel=2)
            return lm.beam_search_generate(x, attention_mask, num_beams, max_new_tokens, min_len, length_penalty, eos_id=eos,
                                           pad_id=PAD_TOKEN_ID, do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p,
                                           repetition_penalty=repetition_penalty, no_repeat_ngram_size=ngram,
                                           num_return_sequences=nret, hf_semantics=sem, **routing)
        if method == "sample_generate":
            return lm.sample_generate(x, attention_mask, max_new_tokens, min_len, do_sample, temperature, top_k, top_p,
                                      repetition_penalty, eos_id=eos, pad_id=PAD_TOKEN_ID, no_repeat_ngram_size=ngram,
                                      num_return_sequences=nret, use_graph=self.use_graph, **routing)
        return lm.greedy_generate(x, attention_mask, max_new_tokens, min_len, eos_id=eos, pad_id=PAD_TOKEN_ID,
                                  use_graph=self.use_graph, stop_on_eos=stop_on_eos)

    @torch.no_grad()
    def generate(self, text: List[str], image: Optional[torch.Tensor] = None, video: Optional[torch.Tensor] = None,
                 image_placeholder: str = DEFAULT_IMG_PLACEHOLDER, video_placeholder: str = DEFAULT_VID_PLACEHOLDER,
                 num_beams=5, max_new_tokens=10, min_len=1, do_sample=False, penalty_alpha=None, top_p=None,
                 top_k=None, temperature=None, length_penalty=-1, repetition_penalty=1.0, synced_gpus=False,
                 skip_special_tokens=True, **kwargs):
        # the reference forwards **kwargs to transformers' generate (emu.py:175,228); the options this engine honours
        # are mapped, anything else is refused rather than silently ignored
        min_new = int(kwargs.pop("min_new_tokens")) if "min_new_tokens" in kwargs else None
        if "min_length" in kwargs:
            min_len = max(int(min_len), int(kwargs.pop("min_length")))
        eos_override = kwargs.pop("eos_token_id", None)
        kwargs.pop("use_cache", None)                   # always cached
        ngram = int(kwargs.pop("no_repeat_ngram_size", 0) or 0)
        nret = int(kwargs.pop("num_return_sequences", 1) or 1)
        constraint = pop_constraint(kwargs)
        lookup = {name: int(kwargs.pop(name)) for name in ("prompt_lookup_num_tokens", "max_matching_ngram_size") if name in kwargs}
        if kwargs:
            raise TypeError(f"EmuModel.generate: unsupported generation options {sorted(kwargs)} "
                            "(the HIP engine implements greedy / beam / sampling / contrastive search with the arguments of the signature)")
        tok = self.decoder.tokenizer
        text = [t.replace(image_placeholder, self.image_placeholder).replace(video_placeholder, self.video_placeholder)
                for t in text]
        inputs = tok(text, padding="longest", return_tensors="pt")
        ids = self.generate_ids(inputs.input_ids, inputs.attention_mask, image, video, max_new_tokens, min_len,
                                num_beams=num_beams, length_penalty=length_penalty, do_sample=do_sample,
                                temperature=temperature, top_k=top_k, top_p=top_p, repetition_penalty=repetition_penalty,
                                penalty_alpha=penalty_alpha, no_repeat_ngram_size=ngram, num_return_sequences=nret,
                                eos_token_id=eos_override, min_new_tokens=min_new, constraint=constraint, **lookup)
        return tok.batch_decode(ids.cpu(), skip_special_tokens=skip_special_tokens)

    # ------------------------------------------------------------------ scoring given text (no counterpart in the reference)
    @torch.no_grad()
    def score_ids(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, image: Optional[torch.Tensor] = None,
                  video: Optional[torch.Tensor] = None, cont_ids: Optional[torch.Tensor] = None,
                  cont_mask: Optional[torch.Tensor] = None, via: str = "decode", use_graph: Optional[bool] = None,
                  reference_logits: Optional[torch.Tensor] = None, return_logits: bool = False):
        """How probable is the continuation ``cont_ids`` [B, T] (right padded, ``cont_mask``) behind the prompt ``input_ids`` /
        ``attention_mask`` [B, S] (left padded, as for ``generate_ids``; ``image`` / ``video`` are scattered into its placeholder
        slots the same way): ``LlamaEngine.score``'s dict.  The reference's Emu2 has no such call."""
        if cont_ids is None:
            raise ValueError("score_ids: cont_ids is required")
        B, S = input_ids.shape
        x = self._prompt_embeds(input_ids, image, self.n_query, IMAGE_TOKEN_ID)
        if video is not None:
            x = self._prompt_embeds(input_ids, video, self.v_query, gIMG_TOKEN_ID, embeds=x)
        return self.decoder.lm.score(x.view(B, S, -1), attention_mask, cont_ids, cont_mask, via=via,
                                     use_graph=self.use_graph if use_graph is None else bool(use_graph),
                                     reference_logits=reference_logits, return_logits=return_logits)

    @torch.no_grad()
    def score(self, text: List[str], continuation: List[str], image: Optional[torch.Tensor] = None,
              video: Optional[torch.Tensor] = None, image_placeholder: str = DEFAULT_IMG_PLACEHOLDER,
              video_placeholder: str = DEFAULT_VID_PLACEHOLDER, via: str = "decode", use_graph: Optional[bool] = None,
              reference_logits: Optional[torch.Tensor] = None, return_logits: bool = False):
        """``score_ids`` on text: the prompts are tokenised as ``generate`` tokenises them (left padded, special tokens), the
        continuations right padded without special tokens."""
        if len(text) != len(continuation):
            raise ValueError(f"score: {len(text)} prompts but {len(continuation)} continuations")
        tok = self.decoder.tokenizer
        text = [t.replace(image_placeholder, self.image_placeholder).replace(video_placeholder, self.video_placeholder)
                for t in text]
        inputs = tok(text, padding="longest", return_tensors="pt")
        side, tok.padding_side = tok.padding_side, "right"
        try:
            cont = tok(list(continuation), padding="longest", return_tensors="pt", add_special_tokens=False)
        finally:
            tok.padding_side = side
        return self.score_ids(inputs.input_ids, inputs.attention_mask, image, video, cont.input_ids, cont.attention_mask.bool(),
                              via=via, use_graph=use_graph, reference_logits=reference_logits, return_logits=return_logits)

    @torch.no_grad()
    def score_candidates_ids(self, input_ids: torch.Tensor, attention_mask: torch.Tensor, image: Optional[torch.Tensor] = None,
                             video: Optional[torch.Tensor] = None, cand_ids: Optional[torch.Tensor] = None,
                             cand_mask: Optional[torch.Tensor] = None, n_segments: int = 1, via: str = "prefill",
                             share_prefix: bool = False):
        """Rank N candidate continuations ``cand_ids`` / ``cand_mask`` [N, Tc] (right padded) of ONE prompt ``input_ids`` /
        ``attention_mask`` [1, S] (``image`` / ``video`` scattered into its placeholder slots as for ``generate_ids``): the
        per-token log-probabilities of ``LlamaEngine.score_continuations`` with ``generate``'s positions.  The prompt is prefilled
        once; ``share_prefix=True`` also keeps its cache in one place (no copy per candidate).  Returns (lp [N, Tc] fp32, counted
        [N, Tc] bool).  The reference's Emu2 has no ranking call (Emu1's is prediction_mixin.py:36-131)."""
        if cand_ids is None:
            raise ValueError("score_candidates_ids: cand_ids is required")
        if input_ids.dim() != 2 or input_ids.shape[0] != 1:
            raise ValueError(f"score_candidates_ids: one prompt at a time, input_ids must be [1, S], got {tuple(input_ids.shape)}")
        S = input_ids.shape[1]
        x = self._prompt_embeds(input_ids, image, self.n_query, IMAGE_TOKEN_ID)
        if video is not None:
            x = self._prompt_embeds(input_ids, video, self.v_query, gIMG_TOKEN_ID, embeds=x)
        return self.decoder.lm.score_continuations(x.view(1, S, -1), attention_mask, cand_ids, cand_mask, n_segments=n_segments,
                                                   via=via, hf_generate_positions=True, share_prefix=share_prefix)

    @torch.no_grad()
    def score_candidates(self, text: str, candidates: List[str], image: Optional[torch.Tensor] = None,
                         video: Optional[torch.Tensor] = None, image_placeholder: str = DEFAULT_IMG_PLACEHOLDER,
                         video_placeholder: str = DEFAULT_VID_PLACEHOLDER, n_segments: int = 1, via: str = "prefill",
                         share_prefix: bool = False):
        """``score_candidates_ids`` on text: the prompt is tokenised as ``score`` tokenises its prompts, the candidates right padded
        without special tokens.  Returns a dict of ``lp`` / ``counted`` [N, Tc] and, per candidate, ``sum`` (the log-probability of
        the whole candidate) and ``mean`` (per counted token) [N]."""
        tok = self.decoder.tokenizer
        text = text.replace(image_placeholder, self.image_placeholder).replace(video_placeholder, self.video_placeholder)
        inputs = tok([text], padding="longest", return_tensors="pt")
        side, tok.padding_side = tok.padding_side, "right"
        try:
            cand = tok(list(candidates), padding="longest", return_tensors="pt", add_special_tokens=False)
        finally:
            tok.padding_side = side
        lp, counted = self.score_candidates_ids(inputs.input_ids, inputs.attention_mask, image, video, cand.input_ids,
                                                cand.attention_mask.bool(), n_segments=n_segments, via=via, share_prefix=share_prefix)
        total = torch.where(counted, lp, torch.zeros_like(lp)).sum(dim=-1)
        return {"lp": lp, "counted": counted, "sum": total, "mean": total / counted.sum(dim=-1).clamp(min=1)}

    # ------------------------------------------------------------------ generate_image (emu.py:92-153)
    @torch.no_grad()
    def generate_image_ids(self, prompt_ids: torch.Tensor, image: Optional[torch.Tensor] = None,
                           attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Visual-embedding regression at the token-id level: prompt + [IMG] prefill, then n_query-1 cached steps with input
        project_up(project_down(h_prev)).  Rows of different length arrive LEFT-padded with ``attention_mask``; every row then
        sees the positions 0..len-1 of its own tokens (pads are masked out of the attention), i.e. exactly what it computes
        alone -- the rows share one weight stream per step instead of being run one by one."""
        lm = self.decoder.lm
        B, S0 = prompt_ids.shape
        ids = torch.cat((prompt_ids.to(torch.int64), torch.full((B, 1), IMG_TOKEN_ID, dtype=torch.int64)), dim=1)
        S = S0 + 1
        if S + self.n_query > lm.cfg.max_position_embeddings:
            raise ValueError("prompt too long for generate_image")
        x = self._prompt_embeds(ids, image, self.n_query, IMAGE_TOKEN_ID)
        mask = torch.ones(B, S, dtype=torch.int64)
        if attention_mask is not None:
            mask[:, :S0] = attention_mask.to(torch.int64)
        # positions from the mask: arange(S) for an unpadded row (what the reference's lm.model call uses), the row's own
        # 0..len-1 behind left padding
        hidden, kstart, pos = lm.prefill(x.view(B, S, -1), mask, hf_generate_positions=True)
        h = lm.final_norm_rows(hidden[:, -1, :].contiguous())
        first = self._project(h, self.project_down)                                # [B, width]
        if self.n_query == 1:
            return first[:, None, :]
        # replayed from a hipGraph where the host would bound the loop (tensor-parallel shards: a step is ~2.7 ms of small
        # launches at TP = 8); at TP = 1 the eager loop stays ahead of the GPU and measured 2 % FASTER than the replay
        # (10.25 vs 10.48 ms per step: profiles/r04_bench_tp1_*.json), so it is the default there
        if not getattr(self, "regress_graph", self.ctx.tp_size > 1):
            outs = [first]
            for j in range(self.n_query - 1):
                xin = self._project(outs[-1], self.project_up)                    # [B, hidden]
                hj = lm.decode_embeds(xin, pos, S + j, kstart)
                pos = pos + 1
                outs.append(self._project(lm.final_norm_rows(hj), self.project_down))
            return torch.stack(outs, dim=1)                                        # [B, n_query, width]
        return self._regress_replayed(first, pos, S, kstart)

    def _regress_replayed(self, first: torch.Tensor, pos: torch.Tensor, S: int, kstart: torch.Tensor) -> torch.Tensor:
        """The n_query - 1 cached steps of ``generate_image`` with the loop state on the device: one step -- project_up, the decoder
        step on the persistent KV cache, final norm, project_down, ``emu_regress_advance_bf16`` (stores the embedding at the
        device-side step index, makes it the next input, advances positions and slots) -- is captured into a hipGraph once per
        (batch, cache) and replayed; nothing returns to the host before the last step (at TP = 8 a shard's step is 2.7 ms of small
        launches: an eager Python loop would bound it)."""
        from ._lib import check, lib
        lm = self.decoder.lm
        B, width, hidden, dev = first.shape[0], first.shape[1], lm.cfg.hidden_size, self.ctx.device
        L = lib()
        key = (B, lm.s_max, self.n_query, lm.kcache.data_ptr(), lm.mode_epoch)
        st = getattr(self, "_regress_state", None)
        if st is None or st["key"] != key:
            i32 = dict(dtype=torch.int32, device=dev)
            st = dict(key=key, prev=torch.empty(B, width, device=dev, dtype=BF16), xin=torch.empty(B, hidden, device=dev, dtype=BF16),
                      normed=torch.empty(B, hidden, device=dev, dtype=BF16), cur=torch.empty(B, width, device=dev, dtype=BF16),
                      out_all=torch.empty(self.n_query, B, width, device=dev, dtype=BF16), pos=torch.empty(B, **i32),
                      slot=torch.empty(B, **i32), step=torch.empty(1, **i32), kstart=torch.empty(B, **i32),
                      captured=CapturedStep(),
                      ws=torch.empty(max(int(L.emu_llama_workspace_bytes(lm.handle, B, 1)), B * hidden * 2), dtype=torch.uint8, device=dev))
            self._regress_state = st
        st["prev"].copy_(first); st["out_all"][0].copy_(first)
        st["pos"].copy_(pos); st["slot"].fill_(S); st["step"].fill_(1); st["kstart"].copy_(kstart)

        def body():
            sm = ops.stream(dev)
            ops.linear(st["prev"], self.project_up, out=st["xin"])
            check(L.emu_llama_forward(lm.handle, st["xin"].data_ptr(), B, 1, st["pos"].data_ptr(), st["slot"].data_ptr(),
                                      st["kstart"].data_ptr(), None, lm.s_max, st["ws"].data_ptr(), st["ws"].numel(), sm),
                  "emu_llama_forward", self.ctx.handle)
            check(L.emu_llama_final_norm(lm.handle, st["xin"].data_ptr(), st["normed"].data_ptr(), B, sm), "emu_llama_final_norm")
            ops.linear(st["normed"], self.project_down, out=st["cur"])
            check(L.emu_regress_advance_bf16(st["cur"].data_ptr(), st["out_all"].data_ptr(), st["prev"].data_ptr(), st["pos"].data_ptr(),
                                             st["slot"].data_ptr(), st["step"].data_ptr(), B, width, sm), "emu_regress_advance_bf16")

        for _ in range(self.n_query - 1):
            st["captured"].step(body, True, key)
        lm.ctx.check_p2p()
        lm.check_decode_fused()
        return st["out_all"].permute(1, 0, 2).clone()                               # [B, n_query, width] (never a view of the state)

    @torch.no_grad()
    def generate_image(self, text: List[str], image: Optional[torch.Tensor] = None,
                       placeholder: str = DEFAULT_IMG_PLACEHOLDER, warn_ragged: bool = True):
        tok = self.decoder.tokenizer
        text = [t.replace(placeholder, self.image_placeholder) for t in text]
        inputs = tok(text, padding="longest", return_tensors="pt")
        if not bool(inputs.attention_mask.all()):
            # the reference re-pads every iteration and calls lm.model without position_ids, so its
            # left-padded rows see RoPE positions shifted by their pad count; here every row keeps the positions of its own
            # tokens, which is what the same rows compute un-padded (= the reference at batch size 1).
            import warnings
            if warn_ragged:
                warnings.warn("generate_image: prompts of different token lengths are computed as at batch size 1 (each row on "
                              "its own positions); the reference's batched call shifts the RoPE positions of its left-padded "
                              "rows and returns different embeddings for them", stacklevel=2)
            if tok.padding_side != "left":
                tok.padding_side, side = "left", tok.padding_side
                try:
                    inputs = tok(text, padding="longest", return_tensors="pt")
                finally:
                    tok.padding_side = side
            return self.generate_image_ids(inputs.input_ids, image, inputs.attention_mask)
        return self.generate_image_ids(inputs.input_ids, image)
