"""CPU: which matrices get a 13-bit packed set by default (emu_amd.bf16pack.default_pack), against a literal table.  The rule is a
pure function of five scalars -- the value of EMU_BF16_PACK, the tensor-parallel world size, whether the bf16 weights were released,
the bytes the missing head-form sets need, the free device bytes -- so no model, engine or device is built here."""
import inspect

import pytest

from emu_amd import bf16pack

GiB = 2 ** 30
NEED, FREE = 37 * GiB, 180 * GiB          # the 33B model's head-form sets on an MI355X after the bf16 weights and the plain sets

TABLE = [
    # env,    world, released, need,  free,          answer
    (None,    1, False, NEED, FREE,         "all"),
    ("all",   1, False, NEED, FREE,         "all"),
    ("1",     1, False, NEED, FREE,         "all"),       # (the old spelling of "on": read as unset)
    ("plain", 1, False, NEED, FREE,         "plain"),
    ("0",     1, False, NEED, FREE,         "off"),
    (None,    2, False, NEED, FREE,         "plain"),     # tensor-parallel shards: never timed, not changed
    (None,    8, False, NEED, FREE,         "plain"),
    ("all",   2, False, NEED, FREE,         "plain"),
    ("all",   8, False, NEED, FREE,         "plain"),
    ("plain", 8, False, NEED, FREE,         "plain"),
    ("0",     2, False, NEED, FREE,         "off"),
    ("0",     8, False, NEED, FREE,         "off"),
    (None,    1, True,  0,    FREE,         "off"),       # released: flagged row groups would have nothing to read
    ("all",   1, True,  NEED, FREE,         "off"),
    ("plain", 8, True,  NEED, FREE,         "off"),
    (None,    1, False, NEED, 2 * NEED,     "all"),       # exactly half of what is free: fits
    (None,    1, False, NEED, 2 * NEED - 1, "plain"),     # one byte short
    ("all",   1, False, NEED, 10 * GiB,     "plain"),
    (None,    1, False, NEED, 0,            "plain"),
    (None,    1, False, 0,    0,            "all"),       # nothing missing: nothing to fit
]


@pytest.mark.parametrize("env,world,released,need,free,answer", TABLE)
def test_default_pack_table(env, world, released, need, free, answer):
    assert bf16pack.default_pack(env, world, released, need, free) == answer


def test_rule_is_pure_and_needs_no_model():
    """The unit under test is the rule alone: five scalars in, one of three words out, nothing read from the environment, no tensor,
    engine or model touched -- so no small EmuModel on stubs is built for it."""
    assert list(inspect.signature(bf16pack.default_pack).parameters) == ["env", "world_size", "bf16_released", "need", "free"]
    assert set(bf16pack.default_pack.__code__.co_names) <= {"int"}                # no global, module or attribute is read
    answers = {bf16pack.default_pack(e, w, r, n, f) for e in (None, "0", "plain", "all") for w in (1, 2, 8) for r in (False, True)
               for n in (0, NEED) for f in (0, FREE)}
    assert answers == {"off", "plain", "all"}
