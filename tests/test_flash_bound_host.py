"""Host: the bound of tests/test_gpu_flash_kernel.py can tell right from wrong.  No GPU: the float64 reference, the bound, the CPU
restatement of flash_kernel's algorithm and the input makers are that file's; here the restatement must stay within the bound, and
the same restatement with one deliberate error each -- the mistakes a wave-uniform ``interior`` test, a per-wave ``q0 + off`` or a
``kstart`` comparison can make, a skipped key tile, a mis-addressed V row -- must leave it, on three representative cases.  The
criterion the flash tests of test_gpu_ops.py use, ``|err| <= 2e-2 + 2e-2 |want|``, is restated too and the mutants it lets through
are printed (not asserted): they are why the GPU file exists."""
import functools

import pytest

from tests.test_gpu_flash_kernel import KINDS, Case, _inputs, _ks, _restate, _scale, bound_of, ratio_to_bound, reference

CASES = [Case(128, 1, 2, 130, 333, True), Case(128, 1, 2, 260, 260, True, (65,)), Case(64, 1, 2, 257, 700, False)]
MUTANTS = ["kstart+1", "causal+1", "drop_last", "drop_tile1", "v70"]


def _cid(c):
    return f"D{c.D}-{c.Sq}x{c.Sk}-{'causal' if c.causal else 'full'}" + ("" if c.kstart is None else f"-ks{c.kstart[0]}")


@functools.lru_cache(maxsize=None)
def _ref(c, kind):
    q, k, v = _inputs(c, kind)
    ref, A, live, smax = reference(q, k, v, _ks(c), c.causal, _scale(c.D))
    assert bool(live.any()) and smax <= 40.0
    return ref, bound_of(ref, A), live


def _ratios(c, kind, mutant=None):
    """(max |err| / bound over the rows that see a key -- the others must be zero --, whether the earlier criterion
    2e-2 + 2e-2 |want| passes on every element) of a restatement against the reference."""
    ref, bound, live = _ref(c, kind)
    got = _restate(*_inputs(c, kind), _ks(c), c.causal, _scale(c.D), mutant)
    err = (got.double() - ref).abs()
    return ratio_to_bound(got, ref, bound, live), bool((err <= 2e-2 + 2e-2 * ref.abs()).all())


@pytest.mark.parametrize("c", CASES, ids=_cid)
def test_the_restatement_is_within_the_bound(c):
    for kind in KINDS:
        r, old_ok = _ratios(c, kind)
        print(f"{_cid(c)} {kind}: restatement / bound = {r:.3f}")
        assert r <= 1.0, (kind, r)
        assert old_ok, kind                                                 # the earlier criterion is the wider one


@pytest.mark.parametrize("c,mutant", [(c, m) for c in CASES for m in MUTANTS if c.causal or m != "causal+1"],
                         ids=lambda x: _cid(x) if isinstance(x, Case) else x)
def test_a_mutant_exceeds_the_bound(c, mutant):
    """On at least one input kind of every case the mutant applies to (no causal limit to shift where the case has none)."""
    r = {kind: _ratios(c, kind, mutant) for kind in KINDS}
    for kind, (ratio, old_ok) in r.items():
        print(f"{_cid(c)} {mutant} {kind}: mutant / bound = {ratio:.2f}; 2e-2 + 2e-2 |want| "
              f"{'PASSES it' if old_ok else 'catches it'}")
    assert max(ratio for ratio, _ in r.values()) > 1.0, r
