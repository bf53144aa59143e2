"""Constrained decoding: a token trie over a closed set of answers, as a host object and as the flat tables the selection kernels
read (csrc/sample.hip, csrc/beam.hip; include/emu_hip.h: ``emu_token_trie``).

The reference's evaluation model builds a ``Trie`` over the token ids of "yes." / "no." followed by EOS and hands
``prefix_allowed_tokens_fn=lambda batch_id, ids: trie.get(ids.tolist()[1:])`` to ``lm.generate`` with 5 beams
(Emu1/mm_eval/models/emu.py:96-109, Emu1/mm_eval/models/trie.py:16-79).  A Python callable cannot run inside a captured step, so the
device loops take the trie itself.

Conventions, decided here once:

* The prefix is the ids GENERATED so far and nothing else (with ``inputs_embeds`` that is what the library hands the callable: empty
  at the first step).  A caller porting ``trie.get(ids.tolist()[1:])`` drops the ``[1:]``.
* Every sequence ends in exactly one ``eos_id`` (appended if missing).
* A prefix that is not in the trie, and one that is complete (past its EOS), allows ``{eos_id}``: the library raises on an empty
  list, even for finished rows and for beams whose score is already -inf, and EOS is the idiom.
* Flat form: node 0 is the root; the edges of node n are ``tok[first[n]:first[n + 1]]`` (ascending) and lead to ``child[...]``;
  an EOS edge leads to node -1, "exhausted or off the trie", which allows ``{eos_id}``.

Pure Python / torch, no device code."""
from __future__ import annotations

import bisect
from typing import Callable, Dict, List, Sequence, Tuple

import torch


class TokenTrie:
    """Immutable trie over ``sequences`` (lists of token ids in [0, vocab)), each stored with one trailing ``eos_id``."""

    def __init__(self, sequences: Sequence[Sequence[int]], eos_id: int, vocab: int):
        eos_id, vocab = int(eos_id), int(vocab)
        if vocab < 1 or not 0 <= eos_id < vocab:
            raise ValueError(f"eos_id {eos_id} is outside the vocabulary [0, {vocab})")
        seqs = []
        for s in sequences:
            s = [int(t) for t in (s.tolist() if isinstance(s, torch.Tensor) else s)]
            if s and s[-1] == eos_id:
                s = s[:-1]
            if not s:
                raise ValueError("an empty sequence cannot be a constraint")
            if any(t == eos_id for t in s):
                raise ValueError(f"eos_id {eos_id} inside a sequence")
            if any(not 0 <= t < vocab for t in s):
                raise ValueError(f"token id outside the vocabulary [0, {vocab})")
            seqs.append(tuple(s) + (eos_id,))
        if not seqs:
            raise ValueError("a constraint needs at least one sequence")
        # children[n]: token -> node; nodes are numbered in order of first appearance, the root first; an EOS edge leads to -1
        children: List[Dict[int, int]] = [{}]
        for s in seqs:
            n = 0
            for t in s[:-1]:
                if t not in children[n]:
                    children[n][t] = len(children)
                    children.append({})
                n = children[n][t]
            children[n][eos_id] = -1
        first, tok, child = [0], [], []
        for d in children:
            for t in sorted(d):
                tok.append(t)
                child.append(d[t])
            first.append(len(tok))
        self._eos, self._vocab = eos_id, vocab
        self._first, self._tok, self._child = tuple(first), tuple(tok), tuple(child)
        self._count = len(set(seqs))
        self._min_depth = min(len(s) for s in seqs) - 1
        self._tables: Dict[str, Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = {}

    eos_id = property(lambda self: self._eos)
    vocab = property(lambda self: self._vocab)
    nodes = property(lambda self: len(self._first) - 1)
    edges = property(lambda self: len(self._tok))
    count = property(lambda self: self._count, doc="distinct sequences")
    min_depth = property(lambda self: self._min_depth, doc="tokens ahead of the EOS of the shortest sequence")

    def child(self, node: int, token: int) -> int:
        """The node after ``token`` at ``node``; -1 when ``token`` is no edge of it (an EOS edge included)."""
        if not 0 <= node < self.nodes:
            return -1
        lo, hi = self._first[node], self._first[node + 1]
        e = bisect.bisect_left(self._tok, token, lo, hi)              # the ids of a node ascend
        return self._child[e] if e < hi and self._tok[e] == token else -1

    def walk(self, prefix: Sequence[int]) -> int:
        """The node of ``prefix`` (the ids generated so far), -1 once it has left the trie or passed its EOS."""
        n = 0
        for t in prefix:
            n = self.child(n, int(t))
            if n < 0:
                return -1
        return n

    def allowed_at(self, node: int) -> List[int]:
        if not 0 <= node < self.nodes:
            return [self._eos]
        return list(self._tok[self._first[node]:self._first[node + 1]]) or [self._eos]

    def allowed(self, prefix: Sequence[int]) -> List[int]:
        """The sorted ids that may follow ``prefix``."""
        return self.allowed_at(self.walk(prefix.tolist() if isinstance(prefix, torch.Tensor) else prefix))

    def as_callable(self) -> Callable:
        """``prefix_allowed_tokens_fn`` of ``transformers.generate``: (batch_id, ids generated so far) -> list."""
        return lambda batch_id, ids: self.allowed(ids)

    def tables(self, device="cpu") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(first int32 [nodes + 1], tok int32 [edges], child int32 [edges]) on ``device``; made once per device."""
        key = str(torch.device(device))
        if key not in self._tables:
            self._tables[key] = tuple(torch.tensor(t, dtype=torch.int32, device=device) for t in (self._first, self._tok, self._child))
        return self._tables[key]

    @classmethod
    def sequences_of(cls, first, tok, child) -> List[Tuple[int, ...]]:
        """The sequences a set of flat tables holds (each with its EOS), sorted: the inverse of ``tables``."""
        first, tok, child = ([int(v) for v in t] for t in (first, tok, child))
        out, stack = [], [(0, ())]
        while stack:
            n, pre = stack.pop()
            for e in reversed(range(first[n], first[n + 1])):
                if child[e] < 0:
                    out.append(pre + (tok[e],))
                else:
                    stack.append((child[e], pre + (tok[e],)))
        return sorted(out)


def pop_constraint(kwargs: dict):
    """The constraint among ``generate``'s ``**kwargs``: ``constraint`` (a ``TokenTrie``) or the library's
    ``prefix_allowed_tokens_fn`` (a callable), removed from ``kwargs``; None when neither is given."""
    fn, trie = kwargs.pop("prefix_allowed_tokens_fn", None), kwargs.pop("constraint", None)
    if fn is not None and trie is not None:
        raise ValueError("give either `constraint` or `prefix_allowed_tokens_fn`, not both")
    return trie if trie is not None else fn
