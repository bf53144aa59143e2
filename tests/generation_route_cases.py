"""Where a generation runs: the grid of calls behind tests/test_generation_routes.py and the recorder of its truth table.

Everything goes through the public surface -- ``EmuModel.generate_ids`` / ``Emu.generate_ids`` on models made with ``__new__`` around a
recording ``lm``, and ``LlamaEngine.sample_generate`` / ``beam_search_generate`` / ``contrastive_generate`` on a stand-in engine whose
``prefill`` and device loops are spies -- so this file runs unchanged on the commit BEFORE the routing moved into
``emu_amd/genroute.py``.  That is how tests/golden/generation_routes.json was made: with this file copied into a checkout of that
commit,

    git worktree add ../parent 067cf99 && cp tests/generation_route_cases.py ../parent/tests/ &&
        (cd ../parent && python -m tests.generation_route_cases --record $OLDPWD/tests/golden/generation_routes.json)

The outcome of a case: the calls that were reached, in order, with their routing arguments (tensors by shape, the case's trie and
callable by name); the exception that ended it (type and full text), if any; the texts of the warnings given; the once-per-process warning flags
it set (all are cleared before every case).  The table stores each distinct outcome once and, per case in grid order, its index; a
digest of the case ids ties the table to the grid.  ``check_coverage`` asserts on a table that every device loop, every warning flag
and every refusal text of the routing occurs in it: a grid that never reaches a branch proves nothing."""
import ctypes
import hashlib
import itertools
import json
import sys
import types
import warnings

import torch

from emu_amd._lib import SAMPLE_MAX_VOCAB
from emu_amd.constrain import TokenTrie
from emu_amd.emu import EmuModel
from emu_amd.emu1 import Emu
from emu_amd.llama import LlamaEngine

EOS, PAD, HID = 2, 32000, 8
MISSING = "missing"
VOCABS = (5, 12, 13, 64, SAMPLE_MAX_VOCAB + 1)


class Reached(Exception):
    """Raised by a spy: the call got this far."""


class PrefillLogits:
    """What the engine stand-in's ``logits`` returns: the routing reads its dtype; the host loops convert it first thing."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), dtype

    def float(self):
        raise Reached("host loop")


def _callable(batch_id, ids):
    return [3, 4, EOS]


def make_trie(vocab):
    return TokenTrie([[3, 4], [4]], EOS, vocab)               # two sequences, the shortest one token ahead of its EOS


def encode(v, trie=None):
    """A value as JSON: a tensor by shape, the case's trie / callable by name, a C struct by its fields."""
    if isinstance(v, torch.Tensor):
        return {"tensor": list(v.shape)}
    if isinstance(v, PrefillLogits):
        return {"logits": list(v.shape), "dtype": str(v.dtype)}
    if isinstance(v, TokenTrie):
        return "<the case's trie>" if v is trie else "<another trie>"
    if isinstance(v, ctypes.Structure):
        return {name: getattr(v, name) for name, _ in v._fields_}
    if isinstance(v, (list, tuple)):
        return [encode(x, trie) for x in v]
    if isinstance(v, dict):
        return {str(k): encode(x, trie) for k, x in v.items()}
    if callable(v):
        return "<the case's callable>" if v is _callable else "<another callable>"
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    raise TypeError(f"cannot record {type(v)}")


def _reset_flags():
    for cls in (LlamaEngine, EmuModel, Emu):
        for name in list(vars(cls)):
            if name.startswith("_warned"):
                setattr(cls, name, False)


def _flags_set():
    return sorted(f"{cls.__name__}.{name}" for cls in (LlamaEngine, EmuModel, Emu) for name in vars(cls)
                  if name.startswith("_warned") and getattr(cls, name))


def _run(call, events):
    _reset_flags()
    raised = None
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        try:
            call()
        except Reached as e:
            events.append([str(e)])
        except AssertionError:                                 # a check of this module's own: never an outcome
            raise
        except Exception as e:                                 # the refusals, whatever their type
            raised = [type(e).__name__, str(e)]
    out = dict(events=events, raised=raised, warnings=[str(m.message) for m in w], flags=_flags_set())
    _reset_flags()
    return json.loads(json.dumps(out))


# ------------------------------------------------------------------------------------------------ model level
FLAGS = ("device_sampler", "device_beam_sampler", "device_contrastive", "device_ngram_ban", "use_graph")


def _flag_sets():
    """Every flag in {missing, False, True} while the others are all True; every flag alone True, the others missing; all of them
    missing; all of them False."""
    sets = [dict.fromkeys(FLAGS, False), dict.fromkeys(FLAGS, MISSING)]
    for flag, state in itertools.product(FLAGS, (MISSING, False, True)):
        sets.append(dict(dict.fromkeys(FLAGS, True), **{flag: state}))
    for flag in FLAGS:
        sets.append(dict(dict.fromkeys(FLAGS, MISSING), **{flag: True}))
    return [s for i, s in enumerate(sets) if s not in sets[:i]]


def model_cases():
    opts = []
    for beams, sample, ngram, nret, cons in itertools.product((1, 3), (False, True), (0, 2), (1, 2), ("none", "trie", "callable")):
        for pen in (1.0, 1.2):
            opts.append(dict(num_beams=beams, do_sample=sample, repetition_penalty=pen, ngram=ngram, nret=nret, constraint=cons,
                             contrastive=False))
        opts.append(dict(num_beams=beams, do_sample=sample, repetition_penalty=1.0, ngram=ngram, nret=nret, constraint=cons,
                         contrastive=True))
    cases = [dict(level="model", model=model, flags=flags, sem="5.x", min_len=1, **o)
             for model in ("emu2", "emu1") for flags in _flag_sets() for o in opts]
    # Emu2 alone: the "4.31" conventions (the warning, once; min_len < 1 under beams is refused before the embeddings)
    for beams, min_len, contrastive in itertools.product((1, 3), (0, 1), (False, True)):
        cases.append(dict(level="model", model="emu2", flags=dict.fromkeys(FLAGS, True), sem="4.31", min_len=min_len, num_beams=beams,
                          do_sample=False, repetition_penalty=1.0, ngram=0, nret=1, constraint="none", contrastive=contrastive))
    return cases


ROUTING_KEYWORDS = ("device_sampler", "device_beam_sampler", "device_contrastive", "device_ngram_ban", "use_graph", "constraint")


class _RecordingLM:
    """Records of a call its name, its routing keywords with their values, and the names of the others; what the others and the
    positional arguments hold does not depend on the routing and is asserted right here (``passed_through``), not recorded."""

    def __init__(self, case, events, trie):
        self.case, self.events, self.trie = case, events, trie

    def embed_tokens(self, ids):
        return torch.zeros(*ids.shape, HID)

    def __getattr__(self, name):
        def f(*a, **k):
            routing = {n: v for n, v in k.items() if n in ROUTING_KEYWORDS}
            rest = {n: v for n, v in k.items() if n not in ROUTING_KEYWORDS}
            assert (encode(a), rest) == passed_through(self.case, name), (name, encode(a), rest)
            self.events.append([name, encode(routing, self.trie), ",".join(sorted(rest))])
            return torch.zeros(1, 1, dtype=torch.int64)
        return f


def passed_through(c, method):
    """(positional arguments, keywords that are no routing keywords) of the engine call of case ``c``: the embeddings, the mask and
    the case's own options, in the engine method's order."""
    emu2 = c["model"] == "emu2"
    x, mask, new = {"tensor": [1, 4, HID]}, {"tensor": [1, 4]}, 6
    min_len = c["min_len"] if not emu2 or c["sem"] == "4.31" else max(c["min_len"] - 4, 0)      # 5.x subtracts the prompt's 4 slots
    top_k, pen = 4 if c["contrastive"] else None, c["repetition_penalty"]
    ends = dict(eos_id=EOS, pad_id=PAD)
    if method == "contrastive_generate":
        return [x, mask, new, 0.6, 4, min_len, pen], ends
    if method == "beam_search_generate":
        return [x, mask, c["num_beams"], new, min_len, -1.0 if emu2 else 0.0], dict(
            ends, do_sample=c["do_sample"], temperature=None, top_k=top_k, top_p=None, repetition_penalty=pen,
            no_repeat_ngram_size=c["ngram"], num_return_sequences=c["nret"], hf_semantics=c["sem"])
    if method == "sample_generate":
        return [x, mask, new, min_len, c["do_sample"], None, top_k, None, pen], dict(ends, no_repeat_ngram_size=c["ngram"],
                                                                                       num_return_sequences=c["nret"])
    assert method == "greedy_generate", method
    return [x, mask, new, min_len], dict(ends, stop_on_eos=True) if emu2 else ends


def run_model_case(c):
    events, trie = [], make_trie(64)
    lm = _RecordingLM(c, events, trie)
    if c["model"] == "emu2":
        m = EmuModel.__new__(EmuModel)
        m.n_query = m.v_query = 1
        m.decoder = types.SimpleNamespace(lm=lm)
        m._prompt_embeds = lambda ids, *a, **k: (events.append(["_prompt_embeds"]), torch.zeros(ids.numel(), HID))[1]
        length = dict(min_len=c["min_len"])
    else:
        m = Emu.__new__(Emu)
        m.lm = lm
        length = dict(min_length=c["min_len"])
    m.hf_semantics = c["sem"]
    for name, state in c["flags"].items():
        if state != MISSING:
            setattr(m, name, state)
    cons = {"none": None, "trie": trie, "callable": _callable}[c["constraint"]]
    ids, mask = torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, 4, dtype=torch.int64)
    kw = dict(penalty_alpha=0.6, top_k=4) if c["contrastive"] else {}
    return _run(lambda: m.generate_ids(ids, mask, max_new_tokens=6, num_beams=c["num_beams"], do_sample=c["do_sample"],
                                       repetition_penalty=c["repetition_penalty"], no_repeat_ngram_size=c["ngram"],
                                       num_return_sequences=c["nret"], constraint=cons, **length, **kw), events)


# ------------------------------------------------------------------------------------------------ engine level
def _engine_case(method, vocab, tp=1, handle=True, dtype="bf16", **args):
    return dict(level="engine", method=method, vocab=vocab, tp=tp, handle=handle, dtype=dtype, args=args)


NGRAM_BAN = ((0, False), (2, False), (2, True))               # (no_repeat_ngram_size, device_ngram_ban)
CONSTRAINTS = ("none", "trie", "callable")
BEAM_MODES = (dict(), dict(repetition_penalty=1.2), dict(do_sample=True))


def sample_cases():
    out = []
    for vocab, tp, new, dev, (ngram, ban), cons, sample in itertools.product(VOCABS, (1, 2), (6, 257), (False, True), NGRAM_BAN,
                                                                             CONSTRAINTS, (False, True)):
        if tp == 2 and vocab not in (64, SAMPLE_MAX_VOCAB + 1):       # (the small vocabularies under one rank only: the grid stays small)
            continue
        out.append(_engine_case("sample", vocab, tp, max_new_tokens=new, device_sampler=dev, no_repeat_ngram_size=ngram,
                                device_ngram_ban=ban, constraint=cons, do_sample=sample))
    for new, dev, (ngram, ban), cons, sample in itertools.product((6, 257), (False, True), NGRAM_BAN, CONSTRAINTS, (False, True)):
        base = dict(max_new_tokens=new, device_sampler=dev, no_repeat_ngram_size=ngram, device_ngram_ban=ban, constraint=cons,
                    do_sample=sample)
        out.append(_engine_case("sample", 64, handle=False, **base))
        out.append(_engine_case("sample", 64, num_return_sequences=2, **base))
        out.append(_engine_case("sample", 64, uniforms="good", **base))
        out.append(_engine_case("sample", 64, uniforms="bad", **base))
        out.append(_engine_case("sample", 64, num_return_sequences=2, uniforms="good", **base))
    return out


def beam_cases():
    out = []
    for vocab, beams, new, mode, dev, (ngram, ban), cons, trace in itertools.product(VOCABS, (3, 9), (6, 257), BEAM_MODES, (False, True),
                                                                                     NGRAM_BAN, CONSTRAINTS, (False, True)):
        if (trace or new == 257) and vocab not in (13, 64):           # (a trace, and the long call, at the two mid vocabularies only)
            continue
        out.append(_engine_case("beam", vocab, num_beams=beams, max_new_tokens=new, device_beam_sampler=dev, no_repeat_ngram_size=ngram,
                                device_ngram_ban=ban, constraint=cons, trace=trace, **mode))
    for vocab, mode, dev, (ngram, ban), cons in itertools.product((13, 64), BEAM_MODES, (False, True), NGRAM_BAN, CONSTRAINTS):
        base = dict(num_beams=3, max_new_tokens=6, device_beam_sampler=dev, no_repeat_ngram_size=ngram, device_ngram_ban=ban,
                    constraint=cons, **mode)
        out.append(_engine_case("beam", vocab, tp=2, **base))
        out.append(_engine_case("beam", vocab, handle=False, **base))
        out.append(_engine_case("beam", vocab, dtype="fp32", **base))
        out.append(_engine_case("beam", vocab, uniforms="good", **base))
        out.append(_engine_case("beam", vocab, uniforms="bad", **base))
        out.append(_engine_case("beam", vocab, hf_semantics="5.x", **base))
        out.append(_engine_case("beam", vocab, hf_semantics="4.30", **base))
        out.append(_engine_case("beam", vocab, num_return_sequences=2, **base))
        out.append(_engine_case("beam", vocab, num_return_sequences=4, **base))
    return out


def contrastive_cases():
    out = []
    for vocab, tp, k, handle, dev, trace, forced in itertools.product(VOCABS, (1, 2), (4, 9), (False, True), (False, True), (False, True),
                                                                      (False, True)):
        out.append(_engine_case("contrastive", vocab, tp, handle, top_k=k, device_contrastive=dev, trace=trace, forced=forced,
                                use_graph=handle))
    return out


def two_fault_cases():
    """Calls with two things wrong: which refusal comes first is behaviour."""
    beam = dict(num_beams=3, max_new_tokens=6)
    return [
        _engine_case("beam", 64, hf_semantics="4.30", constraint="trie", min_len=2, **beam),             # the constraint, then the rest
        _engine_case("beam", 64, hf_semantics="4.30", constraint="bad type", **beam),
        _engine_case("beam", 64, hf_semantics="4.30", num_return_sequences=4, **beam),
        _engine_case("beam", 64, num_return_sequences=4, uniforms="bad", **beam),
        _engine_case("beam", 64, tp=2, uniforms="bad", do_sample=True, device_beam_sampler=True, **beam),
        _engine_case("beam", 64, tp=2, do_sample=True, device_beam_sampler=True, no_repeat_ngram_size=2, **beam),
        _engine_case("beam", 64, tp=2, do_sample=True, device_beam_sampler=True, no_repeat_ngram_size=2, device_ngram_ban=True, trace=True,
                     **beam),                                                                         # the warning, not the refusal
        _engine_case("beam", 64, handle=False, tp=2, do_sample=True, device_beam_sampler=True, **beam),
        _engine_case("beam", 64, constraint="other vocabulary", num_return_sequences=4, **beam),
        _engine_case("beam", 64, constraint="trie", num_return_sequences=3, **beam),                  # the trie holds two sequences
        _engine_case("beam", 64, constraint="trie", eos_id=3, **beam),
        _engine_case("beam", 64, constraint="callable", do_sample=True, device_beam_sampler=True, no_repeat_ngram_size=2, tp=2, **beam),
        _engine_case("sample", 64, tp=2, max_new_tokens=6, device_sampler=True, no_repeat_ngram_size=2),
        _engine_case("sample", 64, tp=2, max_new_tokens=6, device_sampler=True, do_sample=False, num_return_sequences=2),
        _engine_case("sample", SAMPLE_MAX_VOCAB + 1, tp=2, max_new_tokens=6, device_sampler=True),
        _engine_case("sample", 64, max_new_tokens=6, device_sampler=True, do_sample=False, num_return_sequences=2, uniforms="bad"),
        _engine_case("sample", 64, max_new_tokens=6, device_sampler=True, constraint="trie", min_len=2, no_repeat_ngram_size=2),
        _engine_case("sample", 64, max_new_tokens=6, device_sampler=True, constraint="bad type", tp=2),
        _engine_case("sample", 64, max_new_tokens=6, constraint="trie", do_sample=True, num_return_sequences=3),
        _engine_case("contrastive", 64, tp=2, top_k=9, device_contrastive=True, trace=True, forced=False, use_graph=False),
        _engine_case("contrastive", SAMPLE_MAX_VOCAB + 1, top_k=9, device_contrastive=True, trace=True, forced=True, use_graph=False),
        _engine_case("contrastive", 5, top_k=6, device_contrastive=True, trace=True, forced=False, use_graph=True),   # below top_k, then
    ]


def engine_cases():
    return sample_cases() + beam_cases() + contrastive_cases() + two_fault_cases()


def _stand_in_engine(c, events, trie):
    """A LlamaEngine without a library: what the routing reads, and spies where the device work starts."""
    e = LlamaEngine.__new__(LlamaEngine)
    e.ctx = types.SimpleNamespace(tp_size=c["tp"], check_p2p=lambda: None)
    e.vocab, e.device = c["vocab"], torch.device("cpu")
    e.cfg = types.SimpleNamespace(max_position_embeddings=2048, hidden_size=HID)
    if c["handle"]:
        e.handle = 1
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[c["dtype"]]

    def prefill(embeds, mask, s_max, *a):
        events.append(["prefill", encode((embeds, mask, s_max))])
        B, S, _ = embeds.shape
        return torch.zeros(B, S, HID), torch.zeros(B, dtype=torch.int32), torch.full((B,), S, dtype=torch.int32)

    def spy(name):
        def f(*a, **k):
            # the keywords, and of the positional arguments the one that routes: _sample_device takes its trie last
            events.append([name, encode(a[-1:] if name == "_sample_device" else (), trie), encode(k, trie)])
            raise Reached("device loop")
        return f

    def host(*a, **k):
        raise Reached("host loop")

    e.prefill = prefill
    e.logits = lambda rows, out=None: PrefillLogits((rows.shape[0], c["vocab"]), dtype)
    e.fan_out_kv = lambda *a, **k: None
    e.final_norm_rows = host
    for name in ("_sample_device", "_beam_search_device", "_contrastive_device"):
        setattr(e, name, spy(name))
    return e


def run_engine_case(c):
    events, a = [], dict(c["args"])
    trie = make_trie(c["vocab"])
    eng = _stand_in_engine(c, events, trie)
    x, mask = torch.zeros(1, 4, HID, dtype=torch.bfloat16), torch.ones(1, 4, dtype=torch.int64)
    if "constraint" in a:
        a["constraint"] = {"none": None, "trie": trie, "callable": _callable, "bad type": [[5]],
                           "other vocabulary": make_trie(c["vocab"] + 1)}[a["constraint"]]
    if "trace" in a:
        a["trace"] = {} if a["trace"] else None
    new, eos = a.pop("max_new_tokens", 6), a.pop("eos_id", EOS)
    if c["method"] == "sample":
        if "uniforms" in a:
            rows = a.get("num_return_sequences", 1)
            a["uniforms"] = torch.zeros(new, rows) if a["uniforms"] == "good" else torch.zeros(new, rows + 1)
        call = lambda: LlamaEngine.sample_generate(eng, x, mask, new, eos_id=eos, pad_id=PAD, **a)
    elif c["method"] == "beam":
        nb = a.pop("num_beams")
        if "uniforms" in a:
            a["uniforms"] = torch.zeros(new, 1, 2 * nb) if a["uniforms"] == "good" else torch.zeros(new, 1, nb)
        a.setdefault("hf_semantics", "4.31")
        call = lambda: LlamaEngine.beam_search_generate(eng, x, mask, nb, new, eos_id=eos, pad_id=PAD, **a)
    else:
        k = a.pop("top_k")
        if a.pop("forced"):
            a["force_ids"] = torch.zeros(1, new, dtype=torch.int64)
        call = lambda: LlamaEngine.contrastive_generate(eng, x, mask, new, 0.6, k, eos_id=EOS, pad_id=PAD, **a)
    return _run(call, events)


# ------------------------------------------------------------------------------------------------ the table
def all_cases():
    return model_cases() + engine_cases()


def case_id(c):
    return json.dumps(c, sort_keys=True)


def run_case(c):
    return run_model_case(c) if c["level"] == "model" else run_engine_case(c)


def digest(cases):
    return hashlib.sha256("\n".join(case_id(c) for c in cases).encode()).hexdigest()


def record(cases):
    outcomes, index, seen = [], [], {}
    for c in cases:
        o = run_case(c)
        key = json.dumps(o, sort_keys=True)
        if key not in seen:
            seen[key] = len(outcomes)
            outcomes.append(o)
        index.append(seen[key])
    return dict(cases=len(cases), case_ids_sha256=digest(cases), outcomes=outcomes, index=index)


DIGITS, PER_LINE = "0123456789abcdefghijklmnopqrstuvwxyz", 60


def dump(table, path):
    """One outcome per line; the index as two base-36 digits per case, ``PER_LINE`` cases per line."""
    assert len(table["outcomes"]) <= 36 * 36
    packed = "".join(DIGITS[i // 36] + DIGITS[i % 36] for i in table["index"])
    lines = [packed[j:j + 2 * PER_LINE] for j in range(0, len(packed), 2 * PER_LINE)]
    rows = lambda items: ",\n".join(json.dumps(x, separators=(",", ":")) for x in items)
    with open(path, "w") as f:
        f.write('{"cases": %d,\n"case_ids_sha256": "%s",\n"outcomes": [\n%s\n],\n"index": [\n%s\n]}\n'
                % (table["cases"], table["case_ids_sha256"], rows(table["outcomes"]), rows(lines)))


def load(path):
    with open(path) as f:
        table = json.load(f)
    packed = "".join(table["index"])
    table["index"] = [int(packed[j:j + 2], 36) for j in range(0, len(packed), 2)]
    return table


DEVICE_LOOPS = ("_sample_device", "_beam_search_device", "_contrastive_device")
WARNING_FLAGS = ("LlamaEngine._warned_sampler_vocab", "LlamaEngine._warned_ngram_ban", "LlamaEngine._warned_contrastive",
                 "LlamaEngine._warned_beam_sampler", "LlamaEngine._warned_beam_constraint", "EmuModel._warned_431")
# one piece of every refusal of the routing and of every reason a warning gives (the device loops' own argument checks, which need
# the library, are not routing).  Beam search with a constraint AND the ban never warns about the ban: where the beam sampler is asked
# for, the constraint's own warning has already taken it out; the deterministic search keeps the host loop without a word.
REFUSALS = (
    "contrastive search with no_repeat_ngram_size / several returned sequences is not built",
    "contrastive search with a constraint is not built",
    "beam search under hf_semantics='4.31' needs min_len >= 1",
    "constraint: the trie was built for vocabulary",
    "constraint: min_len 2 is above the trie's shortest sequence",
    "constraint: num_return_sequences 3 is above the trie's 2 sequences",
    "constraint must be an emu_amd.constrain.TokenTrie or a callable",
    "device_sampler: no_repeat_ngram_size > 0 is not built on the device",
    "device_sampler: not built for tensor parallelism",
    "Greedy methods without beam search do not support `num_return_sequences` different than 1",
    "uniforms must be [max_new_tokens, rows] = ",
    "device_contrastive: not built for tensor parallelism",
    "hf_semantics must be '4.31' or '5.x'",
    "`num_return_sequences` has to be smaller or equal to `num_beams`",
    "uniforms must be [max_new_tokens, prompts, 2 * num_beams] = ",
    "device_beam_sampler: no_repeat_ngram_size > 0 is not built on the device",
    "device_beam_sampler: not built for tensor parallelism",
    "device_beam_sampler needs the HIP engine and its bf16 logits",
)
WARNING_REASONS = (
    "device_ngram_ban: a TokenTrie together with the ban is not built on the device; staying on the host path",
    "is below max_new_tokens + 2 = 8 (the ban and the EOS suppress",
    "is above the sample kernel's bound",
    "device_contrastive: top_k 9 (the kernels take 8)",
    "device_contrastive: vocabulary 40001 above the kernel's bound 40000",
    "device_contrastive: vocabulary 5 below top_k",
    "device_contrastive: a trace is asked for",
    "device_contrastive: a forced token path is given",
    "device_beam_sampler: a constraint is not built into the device beam sampler",
    "device_ngram_ban: a trace is asked for; device_beam_sampler is ignored",
    "is below max_new_tokens + 1 + 2 * num_beams = 13 (a beam could be left",
    "device_beam_sampler: 9 beams (the kernel takes 8)",
    "device_beam_sampler: 257 new tokens (the kernel takes 256)",
    "device_beam_sampler: vocabulary 40001 above the kernel's bound 40000",
    "device_beam_sampler: vocabulary 5 below 2 * num_beams",
    "device_beam_sampler: a trace is asked for",
    "beam search under hf_semantics='4.31' (the transformers release the reference pins) follows a RESTATEMENT",
)


def check_coverage(table):
    """Every device loop (each in every selection variant it has), every warning flag, every refusal and every reason of a warning
    occurs in the table."""
    outs = table["outcomes"]
    calls = [ev for o in outs for ev in o["events"] if len(ev) == 3]
    reached = {ev[0] for ev in calls}
    for name in DEVICE_LOOPS + ("contrastive_generate", "beam_search_generate", "sample_generate", "greedy_generate"):
        assert name in reached, name
    assert any(o["events"][-1:] == [["host loop"]] for o in outs)
    sample = [ev for ev in calls if ev[0] == "_sample_device"]
    assert any(ev[1][-1] == "<the case's trie>" for ev in sample) and any(ev[2].get("ngram") == 2 for ev in sample)
    assert any(ev[1][-1] is None and "ngram" not in ev[2] for ev in sample)
    beam = [ev for ev in calls if ev[0] == "_beam_search_device"]
    for sampler in (False, True):
        mine = [ev[2] for ev in beam if ("sampler" in ev[2]) == sampler]
        assert any(k.get("ngram") == 2 for k in mine) and any("ngram" not in k and k.get("trie") is None for k in mine), sampler
    assert any(ev[2].get("trie") == "<the case's trie>" for ev in beam)
    flags = {f for o in outs for f in o["flags"]}
    for f in WARNING_FLAGS:
        assert f in flags, f
    raised = [o["raised"][1] for o in outs if o["raised"]]
    for text in REFUSALS:
        assert any(text in r for r in raised), text
    given = [w for o in outs for w in o["warnings"]]
    for text in WARNING_REASONS:
        assert any(text in w for w in given), text
    assert all(len(o["warnings"]) == len(o["flags"]) for o in outs)       # one flag per warning: nothing warns without its flag


if __name__ == "__main__":
    cases = all_cases()
    table = record(cases)
    check_coverage(table)
    print(f"{len(cases)} cases, {len(table['outcomes'])} distinct outcomes")
    if "--record" in sys.argv:
        dump(table, sys.argv[sys.argv.index("--record") + 1])
