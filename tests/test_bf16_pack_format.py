"""CPU: the 13-bit lossless bf16 weight format as emu_amd/bf16pack.py states it -- round trip, the hb rule, the flag rule on planted
weights, and no flagged row group under the bench's weight law.  Every comparison is on the raw bits."""
import pytest
import torch

from emu_amd import bf16pack

BF16 = torch.bfloat16


def bits(w):
    return w.contiguous().view(torch.int16)


def from_fields(sign, e8, m7=0):
    v = (sign << 15) | (e8 << 7) | m7
    return torch.tensor([v - 65536 if v >= 32768 else v], dtype=torch.int16).view(BF16)[0]


def planted_matrix():
    """[12, 64] N(0, 0.02^2) with one planted weight in rows 0..8 (and two in row 0); returns (W, planted rows that must flag, emax)."""
    g = torch.Generator().manual_seed(11)
    W = (torch.randn(12, 64, generator=g) * 0.02).to(BF16)
    W[W == 0] = 0.01
    emax = 125                                                       # plant the maximum: 2^-2 * 1.x, so the window is e8 94..125
    W = torch.where(((bits(W).to(torch.int32) >> 7) & 0xFF) < 100, torch.full_like(W, 0.01), W)   # no accidental outsiders
    W[11, 5] = from_fields(0, emax, 3)
    top = emax | 1
    plants = {
        0: [(3, from_fields(0, 0)), (40, from_fields(1, 0))],       # +0 and -0
        1: [(0, from_fields(0, 0, 5))],                              # a subnormal
        2: [(63, from_fields(1, emax - 33, 9))],                     # 33 binades below the maximum
        3: [(17, from_fields(0, top - 32, 1))],                      # just below the window's lowest binade
        4: [(9, from_fields(0, 255))],                               # Inf
        5: [(31, from_fields(1, 255, 64))],                          # NaN
    }
    for r, ps in plants.items():
        for c, v in ps:
            W[r, c] = v
    W[6, 8] = from_fields(1, top - 31, 127)                          # exactly at the window's lowest binade: stays packed
    return W, sorted(plants), emax


def test_round_trip_is_exact():
    g = torch.Generator().manual_seed(0)
    W = (torch.randn(8, 64, generator=g) * 0.02).to(BF16)
    W[W == 0] = 0.01
    for rows in (2, 4):
        p = bf16pack.pack(W, rows)
        back, flagged = bf16pack.unpack(p)
        assert not flagged.any()
        assert torch.equal(bits(back), bits(W))
        assert p["lo"].numel() + p["nib"].numel() + p["sign"].numel() == 8 * 64 * 13 // 8
        assert bf16pack.packed_bytes(8, 64, rows) == 8 * 64 * 13 // 8 + 4


@pytest.mark.parametrize("emax", [124, 125, 30, 31, 32, 254])
def test_hb_rule_odd_and_even_maximum(emax):
    W = torch.full((4, 32), 0.0, dtype=BF16)
    W[:] = from_fields(0, max(emax - 3, 1), 1)
    W[2, 7] = from_fields(1, emax, 0)
    top = emax | 1
    assert bf16pack.hb_rule(emax) == max(0, (top - 31) >> 1) == bf16pack.matrix_hb(W)
    hb = bf16pack.matrix_hb(W)
    assert 2 * hb + 31 == max(top, 31)                               # the window's top pair holds emax
    p = bf16pack.pack(W, 4)
    back, flagged = bf16pack.unpack(p)
    assert p["hb"] == hb and not flagged.any() and torch.equal(bits(back), bits(W))


def test_inf_does_not_set_the_window():
    W = torch.full((4, 32), 0.01, dtype=BF16)
    W[1, 1] = float("inf")
    assert bf16pack.matrix_hb(W) == bf16pack.matrix_hb(torch.full((4, 32), 0.01, dtype=BF16))


@pytest.mark.parametrize("rows", [2, 4])
def test_planted_weights_flag_exactly_their_row_groups(rows):
    W, planted_rows, emax = planted_matrix()
    p = bf16pack.pack(W, rows)
    assert p["hb"] == bf16pack.hb_rule(emax)
    want = torch.zeros(12 // rows, dtype=torch.bool)
    for r in planted_rows:
        want[r // rows] = True
    assert torch.equal(bf16pack.flagged_groups(p), want)
    back, flagged = bf16pack.unpack(p)
    assert torch.equal(flagged, want.repeat_interleave(rows))
    assert torch.equal(bits(back)[~flagged], bits(W)[~flagged])
    assert not flagged[6] or rows == 4 and want[6 // 4]              # the weight at the window's edge flags nothing by itself
    bad = bf16pack.flag_rule(W, p["hb"])
    assert sorted(set(bad.nonzero()[:, 0].tolist())) == planted_rows and not bad[6].any()


def test_bench_weight_law_flags_nothing():
    g = torch.Generator().manual_seed(0)
    W = (torch.randn(256, 6656, generator=g) * 0.02).to(BF16)
    for rows in (2, 4):
        assert not bf16pack.flagged_groups(bf16pack.pack(W, rows)).any()
