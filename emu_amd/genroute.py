"""Where a generation runs, decided in one place and on the host alone: which engine method a model's ``generate_ids`` calls and with
which routing keywords (``model_route``), and, inside the engine, whether the token loop of that method stays on the host or runs on
the device, in which selection variant, with which warning or refusal (``sample_route`` / ``beam_route`` / ``contrastive_route``).
Pure functions of scalars known before any device work: no tensor, no engine, no warning is touched here, so a CPU test can enumerate
them (tests/test_generation_routes.py).  The callers give the warning (once per process), prefill, and branch on the answer."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional, Tuple

from ._lib import BEAM_MAX_BEAMS, BEAM_MAX_NEW_TOKENS, CONTRASTIVE_MAX_K, SAMPLE_MAX_VOCAB
from .constrain import TokenTrie

# ------------------------------------------------------------------------------------------------ model level
MODEL_FLAGS = ("device_sampler", "device_beam_sampler", "device_contrastive", "device_ngram_ban", "use_graph")


def model_flags(model) -> dict:
    """The opt-ins of an ``EmuModel`` / ``Emu`` (their constructors' options of these names); a model made with ``__new__`` lacks
    some or all of them: off."""
    return {name: bool(getattr(model, name, False)) for name in MODEL_FLAGS}


def model_route(flags: dict, num_beams: int, do_sample: bool, top_k, penalty_alpha, repetition_penalty: float, ngram: int,
                num_return_sequences: int, constraint, prompt_lookup_num_tokens: int = 0,
                max_matching_ngram_size: int = 2) -> Tuple[str, dict]:
    """Mode selection as transformers does it -> (the ``LlamaEngine`` method, its routing keywords): contrastive search, beam
    search / beam sampling, ``sample_generate`` (whatever one beam needs logits processing for), else plain greedy.  An option that is
    off adds no keyword: the call is then the one made before the option existed.  An n-gram ban takes the device samplers out
    unless ``device_ngram_ban`` is on, which alone switches no sampler on.  A ``constraint`` is handed on as it is.
    ``prompt_lookup_num_tokens`` > 0 (the library's option of that name; 0 = every call is what it was): ``lookup_generate``, for a
    call that is otherwise plain greedy and, with ``device_sampler`` on, for one beam that samples or penalises (then with the
    keywords ``do_sample`` and ``repetition_penalty``; the caller adds the warpers' values) -- anything else is ``lookup_route``'s
    ValueError."""
    if prompt_lookup_num_tokens:
        lookup_route(prompt_lookup_num_tokens, 1, 1, num_beams, do_sample, top_k, penalty_alpha, repetition_penalty, ngram,
                     num_return_sequences, constraint, device_sampler=flags["device_sampler"])
        selection = dict(do_sample=bool(do_sample), repetition_penalty=float(repetition_penalty)) \
            if do_sample or repetition_penalty != 1.0 else {}
        return "lookup_generate", dict(num_tokens=int(prompt_lookup_num_tokens), max_ngram=int(max_matching_ngram_size),
                                       use_graph=flags["use_graph"], **selection)
    if penalty_alpha is not None and penalty_alpha > 0 and top_k is not None and top_k > 1 and num_beams == 1 and not do_sample:
        if ngram or num_return_sequences != 1:
            raise NotImplementedError("contrastive search with no_repeat_ngram_size / several returned sequences is not built")
        if constraint is not None:
            raise NotImplementedError("contrastive search with a constraint is not built")
        return "contrastive_generate", dict(device_contrastive=True, use_graph=flags["use_graph"]) if flags["device_contrastive"] else {}
    ban = bool(ngram) and flags["device_ngram_ban"]
    extra = dict(device_ngram_ban=True) if ban else {}
    if constraint is not None:
        extra["constraint"] = constraint
    if num_beams > 1:
        if flags["device_beam_sampler"] and (not ngram or ban):
            extra["device_beam_sampler"] = True
        return "beam_search_generate", extra
    if do_sample or repetition_penalty != 1.0 or ngram or num_return_sequences != 1 or constraint is not None:
        return "sample_generate", dict(device_sampler=flags["device_sampler"] and (not ngram or ban), **extra)
    return "greedy_generate", {}


# ------------------------------------------------------------------------------------------------ engine level
@dataclass(frozen=True)
class Route:
    """Where one call's token loop runs: on the ``device`` or the host; the selection ``variant`` ("plain", "trie", "ngram"); beam
    search's ``sampler`` step or the deterministic one; the ``warning`` to give first (``LlamaEngine``'s once-per-process flag, the
    text); ``device_kw``, the extra keywords of ``_sample_device`` / ``_beam_search_device``."""
    device: bool
    variant: str = "plain"
    sampler: bool = False
    warning: Optional[Tuple[str, str]] = None
    device_kw: dict = field(default_factory=dict)


def constraint_kind(constraint) -> Optional[str]:
    """None, "trie" (may run on the device) or "callable" (a Python function cannot run inside a captured step: the host loop)."""
    return None if constraint is None else "trie" if isinstance(constraint, TokenTrie) else "callable"


# the one statement of the rule; the two loops word what follows from it
BAN_WITH_CONSTRAINT = "a TokenTrie together with the ban is not built on the device"


def _on_device(ngram: int, constraint: Optional[str] = None, sampler: bool = False) -> Route:
    variant = "ngram" if ngram > 0 else "trie" if constraint == "trie" else "plain"
    return Route(True, variant, sampler, device_kw=dict(ngram=ngram) if ngram > 0 else {})


def sample_route(vocab: int, tp_size: int, max_new_tokens: int, device_sampler: bool, ngram: int, device_ngram_ban: bool,
                 constraint: Optional[str]) -> Route:
    """``sample_generate``.  The host loop unless ``device_sampler``; with it, the host loop still takes a callable constraint (without
    a word) and, with one warning per process, a trie together with the ban, a ban with a vocabulary below ``max_new_tokens + 2``
    (the ban, at most one id per generated token, and the EOS suppress could leave a row without a finite score, which the draw does
    not define) and a vocabulary above ``SAMPLE_MAX_VOCAB``.  Refused: a ban without ``device_ngram_ban``, tensor parallelism."""
    if not device_sampler or constraint == "callable":
        return Route(False)
    if ngram > 0 and device_ngram_ban:
        why = (BAN_WITH_CONSTRAINT if constraint is not None else
               f"vocabulary {vocab} is below max_new_tokens + 2 = {max_new_tokens + 2} (the ban and the EOS suppress could "
               "leave a row without a finite score)" if vocab < max_new_tokens + 2 else None)
        if why is not None:
            return Route(False, warning=("_warned_ngram_ban", f"emu_amd: device_ngram_ban: {why}; staying on the host path"))
    elif ngram > 0:
        raise ValueError("device_sampler: no_repeat_ngram_size > 0 is not built on the device; it keeps the host path "
                         "(device_sampler=False)")
    if tp_size > 1:
        raise ValueError("device_sampler: not built for tensor parallelism (the ranks would need one shared table of "
                         "uniforms); use device_sampler=False")
    if vocab > SAMPLE_MAX_VOCAB:
        return Route(False, warning=("_warned_sampler_vocab", f"emu_amd: device_sampler: vocabulary {vocab} is above the sample kernel's "
                                     f"bound {SAMPLE_MAX_VOCAB} (emu_sample_bf16 answers -22); staying on the host path"))
    return _on_device(ngram, constraint)


BEAM_CONSTRAINT_WARNING = ("_warned_beam_constraint", "emu_amd: device_beam_sampler: a constraint is not built into the device beam "
                           "sampler (emu_beam_sample_step_bf16); staying on the host path")


def constraint_drops_beam_sampler(constraint: Optional[str], device_beam_sampler: bool, do_sample: bool,
                                  repetition_penalty: float) -> bool:
    """Beam search, ahead of everything else: a constraint of either kind where the sampler step would run (sampling or a penalty)
    takes ``device_beam_sampler`` out, with ``BEAM_CONSTRAINT_WARNING``."""
    return constraint is not None and bool(device_beam_sampler) and (do_sample or repetition_penalty != 1.0)


def beam_route(vocab: int, tp_size: int, max_new_tokens: int, num_beams: int, do_sample: bool, repetition_penalty: float, ngram: int,
               device_beam_sampler: bool, device_ngram_ban: bool, constraint: Optional[str], trace: bool, device_engine: bool,
               hf_semantics: str, num_return_sequences: int, prompts: int, uniforms_shape: Optional[tuple]) -> Route:
    """``beam_search_generate``, after ``constraint_drops_beam_sampler``: the argument checks, then two device loops, both within the
    step kernels' bounds (``BEAM_MAX_BEAMS``, ``BEAM_MAX_NEW_TOKENS``, 2N <= vocabulary) and without a ``trace``.  The deterministic,
    unpenalised search runs on the device engine whatever the flags say (a trie in its "trie" variant; a callable keeps the host loop)
    and silently keeps the host loop otherwise.  Sampling or a penalty run there with ``device_beam_sampler``, also bounded by
    ``SAMPLE_MAX_VOCAB``: outside the bounds the host loop takes over with one warning per process; tensor parallelism is refused.
    An n-gram ban keeps the host loop -- under ``device_beam_sampler`` it is refused -- unless ``device_ngram_ban`` is on: then both
    loops run their "ngram" variant, except with a constraint, a ``trace`` or a vocabulary below ``max_new_tokens + 1 + 2 *
    num_beams`` (the ban takes at most one id per generated token from a beam's row, and 2N finite continuations must remain beside
    the EOS suppress): there the host loop takes over, with one warning where ``device_beam_sampler`` is thereby ignored.  The
    deterministic search with the ban is not refused under tensor parallelism: nothing is random and every rank holds the same ids;
    no multi-rank run of it has been made."""
    if hf_semantics not in ("4.31", "5.x"):
        raise ValueError("hf_semantics must be '4.31' or '5.x'")
    if not 1 <= num_return_sequences <= num_beams:
        raise ValueError("`num_return_sequences` has to be smaller or equal to `num_beams`")       # the library's own check
    if uniforms_shape is not None and tuple(uniforms_shape) != (max_new_tokens, prompts, 2 * num_beams):
        raise ValueError(f"uniforms must be [max_new_tokens, prompts, 2 * num_beams] = "
                         f"[{max_new_tokens}, {prompts}, {2 * num_beams}], got {tuple(uniforms_shape)}")
    plain = not do_sample and repetition_penalty == 1.0
    sampler = bool(device_beam_sampler) and not plain
    ban_why = None
    if ngram > 0 and device_ngram_ban:
        ban_why = (BAN_WITH_CONSTRAINT if constraint is not None else
                   "a trace is asked for" if trace else
                   f"vocabulary {vocab} is below max_new_tokens + 1 + 2 * num_beams = {max_new_tokens + 1 + 2 * num_beams} "
                   "(a beam could be left with fewer than 2N finite continuations)"
                   if vocab < max_new_tokens + 1 + 2 * num_beams else None)
    device_ban = ngram > 0 and bool(device_ngram_ban) and ban_why is None
    if sampler and ban_why is not None:
        return Route(False, warning=("_warned_ngram_ban", f"emu_amd: device_ngram_ban: {ban_why}; device_beam_sampler is ignored, "
                                     "staying on the host path"))
    within = num_beams <= BEAM_MAX_BEAMS and max_new_tokens <= BEAM_MAX_NEW_TOKENS and vocab >= 2 * num_beams and not trace
    if sampler:
        if ngram > 0 and not device_ban:
            raise ValueError("device_beam_sampler: no_repeat_ngram_size > 0 is not built on the device; it keeps the host path "
                             "(device_beam_sampler=False)")
        if tp_size > 1:
            raise ValueError("device_beam_sampler: not built for tensor parallelism (the ranks would need one shared table of "
                             "uniforms); use device_beam_sampler=False")
        why = (f"{num_beams} beams (the kernel takes {BEAM_MAX_BEAMS})" if num_beams > BEAM_MAX_BEAMS else
               f"{max_new_tokens} new tokens (the kernel takes {BEAM_MAX_NEW_TOKENS})" if max_new_tokens > BEAM_MAX_NEW_TOKENS else
               f"vocabulary {vocab} above the kernel's bound {SAMPLE_MAX_VOCAB}" if vocab > SAMPLE_MAX_VOCAB else
               f"vocabulary {vocab} below 2 * num_beams" if vocab < 2 * num_beams else
               "a trace is asked for" if trace else None)
        if why is not None:
            return Route(False, warning=("_warned_beam_sampler", f"emu_amd: device_beam_sampler: {why} (emu_beam_sample_step_bf16 answers "
                                         "-22 outside its range); staying on the host path"))
        return _on_device(ngram, sampler=True)
    if plain and (not ngram or device_ban) and within and device_engine and constraint != "callable":
        return _on_device(ngram if device_ban else 0, constraint)
    return Route(False)


def contrastive_route(vocab: int, tp_size: int, top_k: int, device_contrastive: bool, trace: bool, forced: bool) -> Route:
    """``contrastive_generate``.  The host loop unless ``device_contrastive``; with it, tensor parallelism is refused (the ranks would
    have to agree on every selection), and the host loop takes over, with one warning per process, for ``top_k`` above
    ``CONTRASTIVE_MAX_K``, a vocabulary above ``SAMPLE_MAX_VOCAB`` or below ``top_k``, a ``trace`` or a forced token path."""
    if not device_contrastive:
        return Route(False)
    if tp_size > 1:
        raise ValueError("device_contrastive: not built for tensor parallelism (the ranks would have to agree on every "
                         "selection); use device_contrastive=False")
    why = (f"top_k {top_k} (the kernels take {CONTRASTIVE_MAX_K})" if top_k > CONTRASTIVE_MAX_K else
           f"vocabulary {vocab} above the kernel's bound {SAMPLE_MAX_VOCAB}" if vocab > SAMPLE_MAX_VOCAB else
           f"vocabulary {vocab} below top_k" if vocab < top_k else
           "a trace is asked for" if trace else
           "a forced token path is given" if forced else None)
    if why is None:
        return Route(True)
    return Route(False, warning=("_warned_contrastive", f"emu_amd: device_contrastive: {why} (the kernels answer -22 outside their "
                                 "range); staying on the host path"))


LOOKUP_MAX_TOKENS = 7          # a chunk step has 1 + k <= 8 rows (the chunk attention kernel's DECODE_CHUNK_MAX)


def lookup_route(k: int, prompts: int, tp_size: int, num_beams: int = 1, do_sample: bool = False, top_k=None, penalty_alpha=None,
                 repetition_penalty: float = 1.0, ngram: int = 0, num_return_sequences: int = 1, constraint=None,
                 device_sampler: bool = False) -> Route:
    """``prompt_lookup_num_tokens = k``.  k == 0: off, nothing is decided here.  Else the device loop of ``lookup_generate`` runs when
    the call is otherwise plain greedy, one prompt (the library refuses assisted decoding for a batch, and so does this), 1 <= k <=
    ``LOOKUP_MAX_TOKENS`` and no tensor parallelism; together with contrastive search, beams, sampling, a repetition penalty, an
    n-gram ban, several returned sequences or a constraint it is a ValueError that names the mode, before any device work.
    ``device_sampler`` on: one beam that samples or carries a repetition penalty runs on the device too (the chunk rows are picked
    by the sampler's kernel, ``speculate.row_select``); every other refusal stands."""
    k = int(k)
    if k == 0:
        return Route(False)
    contrastive = penalty_alpha is not None and penalty_alpha > 0 and top_k is not None and top_k > 1 and num_beams == 1 and not do_sample
    mode = ("contrastive search (penalty_alpha with top_k)" if contrastive else
            f"beam search (num_beams = {num_beams})" if num_beams > 1 else
            "sampling (do_sample)" if do_sample and not device_sampler else
            f"a repetition penalty ({repetition_penalty})" if repetition_penalty != 1.0 and not device_sampler else
            f"an n-gram ban (no_repeat_ngram_size = {ngram})" if ngram else
            f"num_return_sequences = {num_return_sequences}" if num_return_sequences != 1 else
            "a constraint" if constraint is not None else None)
    if mode is not None:
        unless = " unless device_sampler is on" if mode.startswith(("sampling", "a repetition penalty")) else ""
        raise ValueError(f"prompt_lookup_num_tokens: speculative decoding is built for plain greedy search only, not together with "
                         f"{mode}{unless}")
    if not 1 <= k <= LOOKUP_MAX_TOKENS:
        raise ValueError(f"prompt_lookup_num_tokens must be in 1..{LOOKUP_MAX_TOKENS} (a step verifies at most {LOOKUP_MAX_TOKENS + 1} "
                         f"rows), got {k}")
    if prompts != 1:
        raise ValueError(f"prompt_lookup_num_tokens: assisted generate is only supported for batch_size = 1, got {prompts} prompts")
    if tp_size > 1:
        raise ValueError("prompt_lookup_num_tokens: not built for tensor parallelism (the chunk step has no multi-rank form)")
    return Route(True)
