"""Host side of the loops whose state lives on the device: one step captured into a hipGraph and replayed, and the cadence at
which the host looks at the done flags.  Used by llama.py (greedy, sampling, beam, contrastive), emu.py (the regress loop of
``generate_image``) and unet.py (denoise); imports nothing from them."""
from __future__ import annotations

import os
import warnings
from typing import Callable, Optional

import torch


def _capture_graph(body: Callable[[], None]):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    return g


class CapturedStep:
    """The hipGraph of one step of a loop.  ``body()`` launches the step; it reads every index from device memory, so one captured
    step serves every iteration.  ``step(body, use_graph, key)`` advances the device state by EXACTLY one step, eagerly or from the
    graph.

    The accounting that every caller needs and none should restate: on first use (or under another ``key``: a mode switch, another
    buffer) ``body`` runs once outside capture as a real step -- it also does what a capture must not (lazy module loads, weight
    table uploads) -- and is then captured, which records the launches but does NOT execute them.  So that call, too, advanced
    the state by the one warm-up step; every later call is one replay.

    ``body`` comes with every call and is not kept: it is a closure over the loop's state (and its engine), which in turn holds this
    object -- kept here, the cycle would leave a dropped state's buffers and graph to the garbage collector instead of freeing them
    at once.  ``key`` must therefore cover everything ``body`` reads besides the state: under the same key the graph is replayed.

    ``capture(body) -> graph`` (an object with ``replay()``) is there for the CPU tests alone."""

    def __init__(self, capture: Callable = _capture_graph):
        self.capture = capture
        self.graph, self.key = None, None

    def step(self, body: Callable[[], None], use_graph: bool = True, key=None) -> None:
        if not use_graph:
            body()
        elif self.graph is None or self.key != key:
            body()
            self.graph, self.key = self.capture(body), key
        else:
            self.graph.replay()


def run_polled(step: Callable[[int], None], total: int, poll: int, finished: Callable[[], bool]) -> None:
    """``step(i)`` for i = 0 .. total - 1, ``poll`` at a time: ``finished()`` -- the one host read, the launches before it stay
    queued ahead -- is asked before every chunk but the first, and a true answer ends the loop.  (Steps run between the end and
    the look that saw it must change nothing: the loops' kernels see to that.)"""
    for start in range(0, total, poll):
        if start and finished():
            return
        for i in range(start, min(start + poll, total)):
            step(i)


def warn_once(cls, flag: str, message: str) -> None:
    """One warning per process: ``cls.<flag>`` remembers that it was given."""
    if not getattr(cls, flag):
        setattr(cls, flag, True)
        warnings.warn(message, stacklevel=3)


def option_or_env(option: Optional[bool], name: str) -> bool:
    """An opt-in given to a constructor, or (None) the environment variable ``name``: off unless "1"."""
    return os.environ.get(name, "0") == "1" if option is None else bool(option)
