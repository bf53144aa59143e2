"""The host-side runner of the device loops (emu_amd/device_loop.py) without a GPU: the capture accounting with a recording
``capture``, the cadence of the host's look at the done flags, and the one invalidation of the engine's cached loop states."""
import pytest

from emu_amd.device_loop import CapturedStep, option_or_env, run_polled, warn_once
from emu_amd.llama import LlamaEngine


class _Loop:
    """A step that counts, and a capture that -- like a hipGraph capture -- records the step without executing it."""

    def __init__(self):
        self.count = self.bodies = self.captures = self.replays = 0
        self.capturing = False

    def body(self):
        self.bodies += 1
        if not self.capturing:                               # launches issued under capture do not run
            self.count += 1

    def capture(self, body):
        self.captures += 1
        self.capturing = True
        body()
        self.capturing = False
        loop = self

        class Graph:
            def replay(self):
                loop.replays += 1
                loop.count += 1
        return Graph()


@pytest.mark.parametrize("total", [1, 2, 7])
def test_every_call_of_a_captured_step_advances_by_exactly_one(total):
    lp = _Loop()
    cs = CapturedStep(capture=lp.capture)
    for i in range(total):
        cs.step(lp.body, True, "k")
        assert lp.count == i + 1
    # one warm-up that is a real step, one recording that is not, total - 1 replays
    assert (lp.count, lp.bodies, lp.captures, lp.replays) == (total, 2, 1, total - 1)


def test_another_key_warms_up_and_captures_once_more():
    lp = _Loop()
    cs = CapturedStep(capture=lp.capture)
    for _ in range(3):
        cs.step(lp.body, True, 0)
    first = cs.graph
    for _ in range(3):
        cs.step(lp.body, True, 1)
    assert cs.graph is not first and cs.key == 1
    assert (lp.count, lp.bodies, lp.captures, lp.replays) == (6, 4, 2, 4)


def test_the_eager_path_never_captures():
    lp = _Loop()
    cs = CapturedStep(capture=lp.capture)
    for _ in range(5):
        cs.step(lp.body, False, "k")
    assert (lp.count, lp.bodies, lp.captures, lp.replays) == (5, 5, 0, 0) and cs.graph is None


def _polled(total, poll, done_after=None):
    steps, looks = [], []

    def finished():
        looks.append(len(steps))
        return done_after is not None and len(steps) > done_after
    run_polled(steps.append, total, poll, finished)
    return steps, looks


def test_run_polled_looks_before_every_chunk_but_the_first():
    steps, looks = _polled(10, 4)
    assert steps == list(range(10)) and looks == [4, 8]          # before chunks 2 and 3


def test_run_polled_stops_at_the_end_of_the_chunk_that_finished():
    steps, looks = _polled(10, 4, done_after=5)                 # finished from step 5 on: seen by the look after step 7
    assert steps == list(range(8)) and looks == [4, 8]
    steps, looks = _polled(10, 4, done_after=8)                  # never runs past total
    assert steps == list(range(10)) and looks == [4, 8]


@pytest.mark.parametrize("total", [0, 1, 3, 4])
def test_run_polled_within_one_chunk_never_looks(total):
    steps, looks = _polled(total, 4, done_after=-1)
    assert steps == list(range(total)) and looks == []


def test_a_mode_change_drops_every_cached_loop_state():
    eng = LlamaEngine.__new__(LlamaEngine)
    eng.mode_epoch = 3
    eng._loop_states = {"beam": (("key",), {"captured": object()}), "contrastive": (("key",), {"captured": object()})}
    eng._mode_changed()
    assert eng._loop_states == {} and eng.mode_epoch == 4


def test_warn_once_and_option_or_env(monkeypatch):
    class Flags:
        _warned = False
    with pytest.warns(UserWarning, match="staying"):
        warn_once(Flags, "_warned", "staying on the host path")
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        warn_once(Flags, "_warned", "staying on the host path")          # the second time: silent
    monkeypatch.delenv("EMU_X", raising=False)
    assert option_or_env(None, "EMU_X") is False and option_or_env(True, "EMU_X") is True
    monkeypatch.setenv("EMU_X", "1")
    assert option_or_env(None, "EMU_X") is True and option_or_env(False, "EMU_X") is False
    monkeypatch.setenv("EMU_X", "true")                                  # off unless "1"
    assert option_or_env(None, "EMU_X") is False
