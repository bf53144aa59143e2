"""Host: the bounds of tests/test_gpu_norm_kernels.py hold for the kernels' algorithms and can tell right from wrong.  No GPU: the
references, bounds, inputs and fp32 restatements are those of tests/norm_cases.py.  Every restatement must stay within its bound on
every case and input kind (its worst ratio per kernel is printed; test_gpu_norm_kernels.py records it as RESTATED_WORST), and the
same restatement with one deliberate error must leave the bound on at least one case.  For each such mutant the earlier criterion
(``close`` of test_gpu_ops.py; relative L2 < 5e-3 for GroupNorm and softmax) is evaluated on the same data and printed, not
asserted: what it lets through is why the GPU file exists.  As printed by this file, (cases, kinds) over the bound / of those the
earlier criterion passes:

    RMSNorm without eps                     20 of 40 / 10 (the all-zero rows: 0 * inf = NaN, and ``close`` lets a NaN through)
    RMSNorm, last vector out of the sum     26 of 40 / 11
    LayerNorm, unbiased variance             7 of 30 /  3
    GroupNorm, ragged rows left out         15 of 24 /  1
    GroupNorm, group index from C / 32      15 of 24 /  0, and no error at all with 32 groups, the only count the suite had
    softmax, maximum of the first 2048       4 of 50 /  0, all of the ``padded`` kind: below exp's overflow the maximum cancels
    softmax, bias read at ld                10 of 50 /  0, every biased case of more than one row; the suite had no bias

GroupNorm's last case (2560 channels x 13200 pixels, 67 MB) is left to the GPU file, which builds its reference on the device; no
other case is left out."""
import functools

import pytest
import torch

from tests import norm_cases as N

GN_HOST = N.GN_CASES[:-1]
assert N.GN_CASES[-1] == N.GN_BIG


def _show(what, worst):
    print(f"RESTATED_WORST[{what}] = {max(worst.values()):.3f}   " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def _gid(c):
    return f"C{c.C}-G{c.G}-HW{c.HW}-B{c.B}"


# ------------------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("c,want,why", N.GN_TABLE, ids=lambda v: _gid(v) if isinstance(v, N.GNCase) else "")
def test_gn_geometry_matches_the_table(c, want, why):
    cs, nv, RG, nchunk, rows, cg = N.gn_geometry(c.C, c.G, c.HW)
    assert (cs, nv, RG, nchunk, rows) == want, why
    assert cg == c.C // c.G and nv == c.C // cs // 8 and nchunk <= 256 and (nchunk - 1) * rows < c.HW <= nchunk * rows
    assert c.G % cs == 0 and (RG * nv <= 256 or RG == 1)


def test_the_gn_table_reaches_what_it_says():
    geo = {c: N.gn_geometry(c.C, c.G, c.HW) for c in N.GN_CASES}
    cs, nv, RG, nchunk, rows, cg = zip(*geo.values())
    assert set(cs) == {1, 2, 4} and min(N.GN_CASES, key=lambda c: c.G).G == 1 and any(c.G not in (1, 32) for c in N.GN_CASES)
    assert any(r == 1 and v > 256 for r, v in zip(RG, nv)) and any(r == 1 and v == 256 for r, v in zip(RG, nv))
    assert any(32 < n <= 64 for n in nchunk)                                 # a second trip of the 32-chunk fold
    # a ragged last chunk whose rows do not fill the row groups, in a single trip of the fold
    c = N.GN_CASES[1]
    _, _, rg, nch, rw, _ = geo[c]
    last = c.HW - (nch - 1) * rw
    assert 1 < nch <= 32 and last < rw and last % rg and rg * geo[c][1] < 256
    assert float(N.gn_group_means(N.GNCase(64, 32, 1, 2)).abs().max()) / 0.5 == 16        # the ``coded`` kind's mu / sigma


# ------------------------------------------------------------------------------------------------------------ RMSNorm
def _rms_ratio(rows, cols, kind, mutant=None):
    x, w = N.rms_inputs(rows, cols, kind)
    ref, bound = N.rms_reference(x, w)
    got = N.rms_restate(x, w, mutant=mutant)
    if kind == "zero_row" and mutant is None:
        assert bool((N.bits(got[rows // 2]) == 0).all())
    return N.ratio_to_bound(got, ref, bound), N.close_passes(got, ref)


def test_rmsnorm_restatement_is_within_the_bound():
    worst = {}
    for kind in N.RMS_KINDS:
        worst[kind] = max(_rms_ratio(rows, cols, kind)[0] for rows in N.RMS_ROWS for cols in N.RMS_COLS)
    _show("rmsnorm", worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("mutant", N.RMS_MUTANTS)
def test_a_wrong_rmsnorm_exceeds_the_bound(mutant):
    r = {(rows, cols, kind): _rms_ratio(rows, cols, kind, mutant) for rows in N.RMS_ROWS for cols in N.RMS_COLS
         for kind in N.RMS_KINDS}
    _report(mutant, r, "close()")


def _report(mutant, r, old):
    """r: {case: (ratio to the bound, whether the earlier criterion passes)}."""
    over = {k: v for k, v in r.items() if v[0] > 1.0}
    missed = [k for k, v in over.items() if v[1]]
    for k, (ratio, old_ok) in over.items():
        print(f"{mutant} {k}: mutant / bound = {ratio:.2f}; {old} {'PASSES it' if old_ok else 'catches it'}")
    print(f"{mutant}: over the bound on {len(over)} of {len(r)} cases; {old} passes {len(missed)} of those")
    assert over, (mutant, r)


# ------------------------------------------------------------------------------------------------------------ LayerNorm
def _ln_ratio(cols, kind, with_res, mutant=None):
    x, w, b, res = N.ln_inputs(cols, kind)
    res = res if with_res else None
    ref, bound = N.ln_reference(x, w, b, res)
    got = N.ln_restate(x, w, b, res, mutant=mutant)
    return N.ratio_to_bound(got, ref, bound), N.close_passes(got, ref)


def test_layernorm_restatement_is_within_the_bound():
    worst = {}
    for kind in N.LN_KINDS:
        worst[kind] = max(_ln_ratio(cols, kind, with_res)[0] for cols in N.LN_COLS for with_res in (False, True))
    _show("layernorm", worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("mutant", N.LN_MUTANTS)
def test_a_wrong_layernorm_exceeds_the_bound(mutant):
    r = {(cols, kind, "res" if wr else "plain"): _ln_ratio(cols, kind, wr, mutant) for cols in N.LN_COLS for kind in N.LN_KINDS
         for wr in (False, True)}
    _report(mutant, r, "close()")


# ------------------------------------------------------------------------------------------------------------ GroupNorm
@functools.lru_cache(maxsize=4)
def _gn_data(c, kind):
    x, gamma, beta = N.gn_inputs(c, kind)
    return (x, gamma, beta) + N.gn_reference(x, gamma, beta, c.G)


def _gn_ratio(c, kind, silu, mutant=None):
    x, gamma, beta, ref, bound, s, bound_s = _gn_data(c, kind)
    got = N.gn_restate(x, gamma, beta, c.G, silu=silu, mutant=mutant)
    want, bd = (s, bound_s) if silu else (ref, bound)
    return N.ratio_to_bound(got, want, bd), N.rel_l2_passes(got, want)


@pytest.mark.parametrize("c", GN_HOST, ids=_gid)
def test_groupnorm_restatement_is_within_the_bound(c):
    worst = {kind: max(_gn_ratio(c, kind, silu)[0] for silu in (False, True)) for kind in N.GN_KINDS}
    _show(f"groupnorm {_gid(c)}", worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("mutant", N.GN_MUTANTS)
def test_a_wrong_groupnorm_exceeds_the_bound(mutant):
    r = {(_gid(c), kind): _gn_ratio(c, kind, False, mutant) for c in GN_HOST for kind in N.GN_KINDS}
    _report(mutant, r, "relative L2 < 5e-3")
    if mutant == "group_of_32":                                             # with 32 groups, all the suite had, it is no error at all
        assert all(v[0] <= 1.0 for (cid, _), v in r.items() if "-G32-" in cid)


# ------------------------------------------------------------------------------------------------------------ softmax
def _sm_strided(rows, cols, kind):
    """x and the bias as rows of wider flat buffers with different leading dimensions."""
    x, bias, scale = N.sm_inputs(rows, cols, kind)
    ld, ld_bias = cols + 8, cols + 16
    xbuf = torch.zeros(rows * ld, dtype=N.BF16)
    xbuf.view(rows, ld)[:, :cols] = x
    bbuf = None
    if bias is not None:
        bbuf = torch.zeros(rows * ld_bias, dtype=N.BF16)
        bbuf.view(rows, ld_bias)[:, :cols] = bias
    return xbuf, ld, bbuf, ld_bias, scale


def _sm_ratio(rows, cols, kind, strided, mutant=None):
    x, bias, scale = N.sm_inputs(rows, cols, kind)
    ref, bound = N.sm_reference(x, bias, scale)
    if strided:
        xbuf, ld, bbuf, ld_bias, _ = _sm_strided(rows, cols, kind)
        got = N.sm_restate(xbuf, rows, cols, ld, scale, bbuf, ld_bias, mutant)
    else:
        got = N.sm_restate(x.flatten(), rows, cols, cols, scale, None if bias is None else bias.flatten(), cols, mutant)
    if kind == "uniform" and cols & (cols - 1) == 0 and mutant is None:
        assert bool((got.float() == 1.0 / cols).all())
    return N.ratio_to_bound(got, ref, bound), N.rel_l2_passes(got, ref)


def test_softmax_restatement_is_within_the_bound():
    worst = {}
    for kind in N.SM_KINDS:
        worst[kind] = max(_sm_ratio(rows, cols, kind, st)[0] for rows in N.SM_ROWS for cols in N.SM_COLS for st in (False, True))
    _show("softmax", worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("mutant", N.SM_MUTANTS)
def test_a_wrong_softmax_exceeds_the_bound(mutant):
    r = {}
    for rows in N.SM_ROWS:
        for cols in N.SM_COLS:
            for kind in N.SM_KINDS:
                x, bias, scale = N.sm_inputs(rows, cols, kind)
                ref, bound = N.sm_reference(x, bias, scale)
                xbuf, ld, bbuf, ld_bias, _ = _sm_strided(rows, cols, kind)
                got = N.sm_restate(xbuf, rows, cols, ld, scale, bbuf, ld_bias, mutant)
                r[(rows, cols, kind)] = (N.ratio_to_bound(got, ref, bound), N.rel_l2_passes(got, ref))
    _report(mutant, r, "relative L2 < 5e-3")
    if mutant == "max_of_first_2048":                                       # below exp's overflow the subtracted maximum cancels
        assert all(v[0] <= 1.0 for (_, _, kind), v in r.items() if kind != "padded")


# ------------------------------------------------------------------------------------------------------------ CFG + Euler
def test_the_two_euler_references_agree_bit_for_bit():
    sig = N.euler_sigmas()
    assert sig.dtype == torch.float32 and len(sig) == N.EULER_STEPS_N + 1 and float(sig[-1]) == 0.0 and bool((sig[:-1] > 0).all())
    for H, W in N.EULER_MAPS:
        for step in N.EULER_STEPS:
            eps, lat = N.euler_inputs(H, W, step)
            for g in N.EULER_GUIDANCE:
                a, b = N.euler_chain(eps, lat, sig, step, g), N.euler_torch(eps, lat, sig, step, g)
                assert N.same_bits(a, b), (H, W, step, g)
                assert not N.same_bits(a, lat) and bool(torch.isfinite(a.float()).all())
