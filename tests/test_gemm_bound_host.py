"""Host: the bounds of tests/test_gpu_gemm_kernels.py hold for the tiles' algorithm and can tell right from wrong, and every case
of tests/gemm_cases.py reaches the kernel form its table says.  No GPU: the references, bounds, inputs and the fp32 restatement are
those of tests/gemm_cases.py; the plans come from emu_gemm_plan, which runs on the CPU.

Every restatement must stay within its bound on every case and kind (the worst ratio per epilogue is printed; the GPU file records
it as RESTATED_WORST), and the same restatement with one deliberate error must leave the bound on at least one listed case.  The
earlier criteria -- ``close`` of tests/test_gpu_ops.py for the GEMM, relative L2 below 1e-2 for the convs -- accept the mutants
named in the tests below on the same data: that is why the per-element bound exists.  As printed by this file:

    truncating_store          over the bound on 91 of 153 (case, kind, epilogue) -- where it is not, later roundings of a GLU or
                              an activation leave room --; ``close`` accepts all 91
    bias_after_rounding       over on 121 of 153 (rand 50, offset 47, coded 24); ``close`` accepts all 121
    ragged_k_chunk_dropped    over on all 36 with K % 64 != 0 (K = 8, 72, 200); ``close`` rejects them too (at these K a whole
                              chunk is a gross error; its weight falls as 8 / K)
    glu_halves                over on all 51 GLU cases; ``close`` rejects them too
    s2_last_tap_inside        over the bound on every listed stride-2 image (each has an odd side) and the tap test differs; an
                              even side has no such tap, so on 32 x 32 the mutant is bit-identical and passes any criterion; on
                              33 x 33 its relative L2 is 0.14 (a whole output row and column read the pixels that follow)
    up2_parity_swapped        over the bound on every upsampled image and the tap test differs.  Its relative L2 on a random
                              32 x 32 image is 0.74: the relative-L2 criterion was expected to accept it, and it does not --
                              half of all output pixels take a wrong source.  What the earlier conv tests lacked is therefore not
                              this mutant but the non-square, odd-sided images per element and the exact tap test.
The GEMM mutants are tried on the M = 65 cases of the 128 x 64 tile's table and the M = 257 cases of the sliced 256 x 256 tile's.
"""
import pytest
import torch

from tests import gemm_cases as G
from tests.test_capi_symbols import _ensure_built


def _cid(c):
    return f"{c.cfg}-{c.M}x{c.N}x{c.K}-e{''.join(map(str, c.epis))}-p{c.pad}"


# ------------------------------------------------------------------------------------------------------------ plans
def test_every_case_reaches_the_form_its_table_records():
    _ensure_built()
    bad = []
    for c in G.CASES:
        force, tune = G.CONFIGS[c.cfg][:2]
        for tn in (tune, tune | G.TUNE_DIRECT):
            st, entries = G.plan_query(c.M, c.N, c.K, G.plan_epi(c.N, c.epis[0]), force, tn)
            want = c.plan if tn == tune else c.plan._replace(stage=c.plan.stage & ~1)
            if st != 0 or len(entries) != 1 or entries[0][0] != want:
                bad.append((_cid(c), tn, st, entries, want))
            elif G.scratch_need(entries[0][0], entries[0][1], c.M, c.N) > G.SCRATCH_FLOATS:
                bad.append((_cid(c), "scratch", entries))
    assert not bad, bad[:10]
    for (cfg, M, N, K), want in G.SLICED_PLANS.items():
        cs = [c for c in G.CASES if (c.cfg, c.M, c.N, c.K) == (cfg, M, N, K)]
        assert cs and all(c.plan == want for c in cs), (cfg, M, N, K)


def test_the_table_reaches_every_form():
    seen = {(c.cfg, c.plan.tile, c.plan.ksplit > 1, c.plan.reduce, c.plan.w4) for c in G.CASES}
    assert ("S", "C", True, G.REDUCE_SPLITK, 0) in seen and ("P", "256", True, G.REDUCE_PP, 0) in seen
    assert ("W", "256", True, G.REDUCE_PP, 1) in seen and ("W", "256", False, 0, 1) in seen and ("Q", "256", False, 0, 0) in seen
    for cfg, (_, _, bm, bn, _) in G.CONFIGS.items():
        mine = [c for c in G.CASES if c.cfg == cfg]
        assert {bm - 1, bm, bm + 1} <= {c.M for c in mine}
        assert any(c.N % 4 == 3 for c in mine) and any(c.N % 4 == 2 and c.epis[0] in G.GLU for c in mine)
        assert any(c.pad % 4 for c in mine) and any(set(c.epis) == set(G.ALL_EPIS) for c in mine)
        assert any(c.K == 192 for c in mine) and all(bn < c.N <= 600 and c.M <= 600 and c.K <= 1100 for c in mine if c.M != 63)
        if cfg in G.LOCKSTEP:
            assert {8, 64, 72, 200} <= {c.K for c in mine}
        if bm == 256:
            assert {272, 273, 288, 289} <= {c.M for c in mine}


def test_the_sliced_forms_start_where_the_docstring_says():
    _ensure_built()
    for force, tune, tile, reduce, w4 in (("S", 0, "C", 1, 0), ("P", 0, "256", 2, 0), ("P", G.TUNE_W4, "256", 2, 1)):
        for K in range(64, 1089, 64):
            st, e = G.plan_query(63, 4, K, 0, force, tune)
            assert st == 0 and len(e) == 1
            p = e[0][0]
            assert (p.tile, p.w4) == (tile, w4) and (p.ksplit, p.reduce) == ((2, reduce) if K >= 1024 else (1, 0)), (force, tune, K, p)
    # unforced, nothing below the cap is sliced: the dispatcher takes the 128 x 64 tile
    for M, N, K in ((63, 4, 1088), (129, 192, 1088), (600, 600, 1088)):
        st, e = G.plan_query(M, N, K)
        assert st == 0 and e[0][0].tile == "K" and e[0][0].ksplit == 1


def test_the_hybrid_split_is_reached_at_the_recorded_shape_and_not_below():
    _ensure_built()
    M, N, K = G.HYBRID
    for force in ("H", "0"):
        st, e = G.plan_query(M, N, K, 0, force)
        assert st == 0 and e == G.HYBRID_PLAN, e
        for epi in (G.EPI_RESID, G.EPI_SWIGLU):
            st, e = G.plan_query(M, N, K, epi, force)
            assert st == 0 and [x[2:] for x in e] == [x[2:] for x in G.HYBRID_PLAN], (epi, e)
    for M, N, K in G.HYBRID_TOO_SMALL:
        st, e = G.plan_query(M, N, K, 0, "H")
        assert st == 0 and len(e) == 1, (M, N, K, e)


def test_conv_plans_and_the_slow_gather():
    _ensure_built()
    B, H, W, Cin, Cout = G.SLOW_GATHER
    assert not G.conv_fast_gather(B, H, W, Cin, 1) and G.conv_fast_gather(B, H, W, 4096, 1)
    geo = lambda c: (1, H, W, H, W, c)
    # gemm256_ok refuses the slow gather: force 'Q' falls back to the dispatcher's choice, the K-sliced 256 x 128 tile
    st, e = G.plan_query(B * H * W, Cout, 9 * Cin, 0, "Q", 0, geo(Cin))
    assert st == 0 and e[0][0] == G.Plan("C", 8, G.REDUCE_SPLITK, 0, 1), e
    assert G.scratch_need(e[0][0], e[0][1], B * H * W, Cout, True) <= G.SCRATCH_FLOATS
    st, e = G.plan_query(B * H * W, Cout, 9 * 4096, 0, "Q", 0, geo(4096))
    assert st == 0 and e[0][0].tile == "256"
    for force, tile in (("0", "C"), ("K", "K"), ("B", "B")):
        st, e = G.plan_query(B * H * W, Cout, 9 * Cin, 0, force, 0, geo(Cin))
        assert st == 0 and e[0][0].tile == tile
    # the small images: every config of CONV_CFGS gives the tile it names; 'P' slices Cin = 128 (18 k tiles)
    for mode in G.CONV_MODES:
        for (h, w) in G.CONV_IMAGES:
            ho, wo = G.conv_out_hw(mode, h, w)
            for cin, cout in G.CONV_CH:
                for cfg in G.CONV_CFGS:
                    force, tune = ("0", 0) if cfg == "0" else G.CONFIGS[cfg][:2]
                    st, e = G.plan_query(G.CONV_B * ho * wo, cout, 9 * cin, 1, force, tune, (mode, h, w, ho, wo, cin))
                    assert st == 0 and len(e) == 1
                    p = e[0][0]
                    assert p.tile == {"0": "K", "B": "B", "C": "C", "K": "K"}.get(cfg, "256"), (cfg, p)
                    assert p.w4 == int(cfg == "W") and p.ksplit == (2 if cfg in ("P", "W") and cin == 128 and cout % 4 == 0 else 1), (cfg, cin, cout, p)
                    assert G.scratch_need(p, e[0][1], G.CONV_B * ho * wo, cout, True) <= G.SCRATCH_FLOATS


def test_refused_shapes_are_refused_by_the_planner():
    _ensure_built()
    assert G.plan_query(129, 136, 100)[0] == -22                             # K % 8 != 0
    assert G.plan_query(129, 135, 128, G.EPI_SWIGLU)[0] == -22               # an odd N under a GLU
    assert G.plan_query(120, 36, 9 * 72, 0, "0", 0, (1, 5, 8, 5, 8, 72))[0] == -22          # Cin % 64 != 0
    for mode, ho, wo in ((1, 6, 8), (2, 2, 4), (2, 3, 5), (3, 5, 8), (3, 10, 15)):          # Hout / Wout against the mode
        assert G.plan_query(ho * wo * 3, 36, 576, 0, "0", 0, (mode, 5, 8, ho, wo, 64))[0] == -22, (mode, ho, wo)
    for mode in G.CONV_MODES:
        ho, wo = G.conv_out_hw(mode, 5, 8)
        assert G.plan_query(ho * wo * 3, 36, 576, 0, "0", 0, (mode, 5, 8, ho, wo, 64))[0] == 0


# ------------------------------------------------------------------------------------------------------------ GEMM bounds
def _ratio(c, kind, epi, mutant=None):
    ref, bound = G.gemm_reference(c.M, c.N, c.K, kind, epi)
    got = G.gemm_restate(c.M, c.N, c.K, kind, epi, c.cfg, c.plan.ksplit, mutant)
    return G.ratio_to_bound(got, ref, bound), got, ref


def test_gemm_restatement_is_within_the_bound_everywhere_and_exact_on_coded():
    worst = {}
    for c in G.CASES:
        for kind in G.KINDS:
            for epi in c.epis:
                r, got, _ = _ratio(c, kind, epi)
                assert r <= 1.0, (_cid(c), kind, epi, r)
                key = G.EPI_NAMES[epi]
                worst[key] = max(worst.get(key, 0.0), r)
                if kind == "coded" and epi in (G.EPI_NONE, G.EPI_RESID):
                    assert G.same_bits(got, G.gemm_exact(c.M, c.N, c.K, epi)), (_cid(c), epi)
    print("RESTATED_WORST = {" + ", ".join(f'"{k}": {v:.3f}' for k, v in worst.items()) + "}")


def _applies(mutant, c, epi):
    if mutant == "ragged_k_chunk_dropped":
        return c.K % 64 != 0
    if mutant == "glu_halves":
        return epi in G.GLU
    return True


@pytest.mark.parametrize("mutant", G.MUTANTS)
def test_gemm_mutants_leave_the_bound(mutant):
    over, tried, close_ok = {}, 0, 0
    for c in G.CASES:
        if c.cfg not in ("K", "P") or c.M not in (65, 257):                  # one lock-step and one 256 x 256 column of the table
            continue
        for kind in G.KINDS:
            for epi in c.epis:
                if not _applies(mutant, c, epi):
                    continue
                r, got, ref = _ratio(c, kind, epi, mutant)
                tried += 1
                if r > 1.0:
                    over[kind] = over.get(kind, 0) + 1
                    close_ok += G.close_passes(got, ref)
    n = sum(over.values())
    print(f"{mutant}: over the bound on {n} of {tried} (case, kind, epilogue); per kind {over}; of those ``close`` accepts {close_ok}")
    assert n > 0
    if mutant in ("ragged_k_chunk_dropped", "glu_halves"):
        assert over.get("rand", 0) == over.get("offset", 0) == tried // 3     # every case it applies to, on both random kinds
    if mutant in ("truncating_store", "bias_after_rounding"):
        assert over.get("rand", 0) > 0 and close_ok == n, "the earlier criterion was expected to let this through"


# ------------------------------------------------------------------------------------------------------------ conv
def _conv_ratio(mode, h, w, cin, cout, kind, mutant=None, B=G.CONV_B):
    x, wt, bias, b2, res = G.conv_inputs(mode, h, w, cin, cout, kind, B)
    b2s = b2[:, 8:8 + cout]
    ref, bound = G.conv_reference(x, wt, mode, bias, b2s, res)
    got = G.conv_restate(x, wt, mode, bias, b2s, res, mutant=mutant)
    return G.ratio_to_bound(got, ref, bound), got, ref


def test_conv_restatement_is_within_the_bound_and_the_reference_is_torchs_convolution():
    worst = 0.0
    for mode in G.CONV_MODES:
        for (h, w) in G.CONV_IMAGES:
            for cin, cout in G.CONV_CH:
                for kind in G.CONV_KINDS:
                    r, _, _ = _conv_ratio(mode, h, w, cin, cout, kind)
                    assert r <= 1.0, (mode, h, w, cin, cout, kind, r)
                    worst = max(worst, r)
                x, wt, _, _, _ = G.conv_inputs(mode, h, w, cin, cout, "rand")
                ref, _ = G.conv_reference(x, wt, mode)
                want = G.conv_f64(x, wt, mode)
                assert ref.shape == want.shape and float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max()), (mode, h, w)
    B, H, W, Cin, Cout = G.SLOW_GATHER
    r, _, _ = _conv_ratio(1, H, W, Cin, Cout, "rand", B=B)
    assert r <= 1.0
    print(f'RESTATED_WORST["conv"] = {worst:.3f}; slow gather {r:.3f}')


def test_tap_expectation_is_the_convolution_with_the_one_hot_weights():
    for mode in G.CONV_MODES:
        for (h, w) in G.CONV_IMAGES:
            x, wt = G.tap_inputs(G.CONV_B, h, w, 64)
            want = G.tap_expected(x, mode)
            assert torch.equal(G.conv_f64(x, wt, mode), want.double()), (mode, h, w)
            assert G.same_bits(G.conv_restate(x, wt, mode), want), (mode, h, w)


@pytest.mark.parametrize("mutant", G.CONV_MUTANTS)
def test_conv_mutants_leave_the_bound_and_what_the_relative_l2_says(mutant):
    mode = 2 if mutant == "s2_last_tap_inside" else 3
    over = 0
    for (h, w) in G.CONV_IMAGES:
        r, _, _ = _conv_ratio(mode, h, w, 64, 36, "rand", mutant)
        over += r > 1.0
        assert r > 1.0, (mutant, h, w, r)                                    # every listed image has an odd side
        x, wt = G.tap_inputs(G.CONV_B, h, w, 64)
        assert not G.same_bits(G.conv_restate(x, wt, mode, mutant=mutant), G.tap_expected(x, mode)), (mutant, h, w)
    for side in (32, 33):
        x, wt, bias, b2, res = G.conv_inputs(mode, side, side, 64, 36, "rand", 2)
        want = G.conv_restate(x, wt, mode, bias)
        got = G.conv_restate(x, wt, mode, bias, mutant=mutant)
        l2 = float((got.double() - want.double()).norm() / want.double().norm())
        ref, bound = G.conv_reference(x, wt, mode, bias)
        print(f"{mutant} on {side} x {side}: relative L2 {l2:.2e} (criterion 1e-2: {'passes' if l2 < 1e-2 else 'fails'}), "
              f"ratio to the bound {G.ratio_to_bound(got, ref, bound):.1f}")
        if mutant == "s2_last_tap_inside":                                    # an even side has no such tap: no criterion can see it there
            assert G.same_bits(got, want) == (side == 32) and (G.ratio_to_bound(got, ref, bound) > 1.0) == (side == 33)
            assert G.rel_l2_passes(got, want) == (side == 32)
        else:                                                                # on random pixels the swap is gross: relative L2 sees it too
            assert not G.rel_l2_passes(got, want) and G.ratio_to_bound(got, ref, bound) > 1.0
