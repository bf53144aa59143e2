"""CPU: the 12-bit lossless bf16 weight format as emu_amd/bf16pack.py states it (pack12 / unpack12) -- round trip on every kind of bit
pattern and on every (row, element) position of a patch, the window rule on hand-made histograms, the 8-slot limit, the padded last
group and the rule that picks a matrix's format around its break-even.  Every comparison is on the raw bits."""
import inspect

import pytest
import torch

from emu_amd import bf16pack

BF16 = torch.bfloat16
HB = 54
EMPTY = -1                                                            # 0xffffffff as the int32 the record is kept in


def bits(w):
    return w.contiguous().view(torch.int16)


def from_fields(sign, e8, m7=0):
    v = (sign << 15) | (e8 << 7) | m7
    return torch.tensor([v - 65536 if v >= 32768 else v], dtype=torch.int16).view(BF16)[0]


def base_matrix(N, K, seed=0):
    """N(0, 0.02^2) with every weight inside exponent fields 112..123 (codes 56..61): the window is [54, 61], the lowest base that holds
    them all (HB), and nothing misses."""
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, K, generator=g) * 0.02).to(BF16)
    e8 = (bits(W).to(torch.int32) >> 7) & 0xFF
    return torch.where((e8 < 112) | (e8 > 123), torch.full_like(W, 0.01), W)


def slot_fields(s):
    s = int(s) & 0xFFFFFFFF
    return s >> 13, (s >> 11) & 3, (s >> 8) & 7, s & 0xFF            # vi, row in group, element, high byte


# ------------------------------------------------------------------------------------------------ round trip
def test_base_matrix_has_no_miss():
    for rows in (2, 4):
        p = bf16pack.pack12(base_matrix(8, 64), rows)
        assert p["hb"] == HB and p["flagged"] == 0 and int(bf16pack.slots_used(p).sum()) == 0
        assert bool((p["patch"] == EMPTY).all())


@pytest.mark.parametrize("rows", [2, 4])
def test_round_trip_every_kind_of_bit_pattern(rows):
    """+-0, a denormal, Inf, NaN, the smallest and the largest code of the window with both signs, one code below and one above it:
    at most 8 misses per row group, so nothing is flagged and every bit comes back."""
    W = base_matrix(12, 64, seed=1)
    lo_e, hi_e = 2 * HB, 2 * (HB + 7) + 1                            # exponent fields 108 and 123: codes 0 and 7
    plants = {(0, 3): from_fields(0, 0), (0, 40): from_fields(1, 0), (1, 0): from_fields(0, 0, 5), (4, 9): from_fields(0, 255),
              (5, 31): from_fields(1, 255, 64), (8, 1): from_fields(0, lo_e, 0), (8, 2): from_fields(1, lo_e, 127),
              (9, 63): from_fields(0, hi_e, 127), (9, 62): from_fields(1, hi_e, 0), (10, 7): from_fields(1, lo_e - 1, 127),
              (11, 8): from_fields(0, hi_e + 1, 0)}
    for (r, c), v in plants.items():
        W[r, c] = v
    p = bf16pack.pack12(W, rows)
    assert p["hb"] == HB and p["flagged"] == 0 and not bf16pack.flagged_groups(p).any()
    back, flagged = bf16pack.unpack12(p)
    assert not flagged.any() and torch.equal(bits(back), bits(W))
    miss = bf16pack.miss_rule12(W, HB)
    assert sorted(map(tuple, miss.nonzero().tolist())) == sorted(k for k in plants if k[0] not in (8, 9))
    assert int(bf16pack.slots_used(p).sum()) == 7
    n = p["nib"].to(torch.int32)                                     # a missed weight's nibble is 0: row 0, element 3 of vector 0
    assert int(n[0, 0, 0, 3]) & 15 == 0
    assert p["lo"].numel() + p["nib"].numel() == 12 * 64 * 12 // 8
    assert bf16pack.packed_bytes12(12, 64, rows) == 12 * 64 * 12 // 8 + 32 * (12 // rows) + 4


@pytest.mark.parametrize("rows", [2, 4])
def test_a_patch_in_every_row_and_element(rows):
    """One miss per (row in group, element) pair, spread over the row groups 8 to a group, at different vectors: the record names
    each, sorted, and the round trip is exact."""
    G = rows                                                         # rows x 8 positions, 8 per group
    W = base_matrix(G * rows, 2080, seed=2)
    want = {}
    for r in range(rows):
        for j in range(8):
            g, vi = (r * 8 + j) // 8, 7 + 31 * j + r
            v = from_fields(j & 1, 3 + j, 16 * r + j)
            W[g * rows + r, vi * 8 + j] = v
            want.setdefault(g, []).append((vi, r, j, (int(bits(v)) >> 8) & 0xFF))
    p = bf16pack.pack12(W, rows)
    assert p["flagged"] == 0 and bf16pack.slots_used(p).tolist() == [8] * G
    for g in range(G):
        got = [slot_fields(s) for s in p["patch"][g].tolist()]
        assert got == sorted(want[g])
    back, flagged = bf16pack.unpack12(p)
    assert not flagged.any() and torch.equal(bits(back), bits(W))


# ------------------------------------------------------------------------------------------------ the window rule
def hist(**counts):
    h = [0] * 128
    for k, v in counts.items():
        h[int(k[1:])] = v
    return h


@pytest.mark.parametrize("h,hb", [
    ([0] * 128, 0),                                                   # empty: the lowest base
    (hist(b60=10), 53),                                               # one bin: the lowest base whose window holds it
    (hist(b0=5), 0),                                                  # the low end
    (hist(b127=5), 120),                                              # the high end: the last base
    (hist(b126=1, b127=5, b119=5), 119),                              # [119, 126] and [120, 127] both hold 6: the lower base
    (hist(b10=3, b17=3, b18=3), 10),                                  # [10, 17] and [11, 18] both hold 6: the tie goes to the lower base
    (hist(b10=3, b17=3, b18=4), 11),                                  # [11, 18] holds 7
    (hist(b56=100, b57=900, b58=3000, b59=4000, b60=1500, b61=400, b62=90, b63=9, b55=8, b64=1), 56),
    (hist(b56=100, b57=900, b58=3000, b59=4000, b60=1500, b61=400, b62=90, b63=9, b55=9), 55),       # a tie again: the lower base
])
def test_window_rule_on_hand_made_histograms(h, hb):
    assert bf16pack.window_rule(h) == hb
    best = max(sum(h[b:b + 8]) for b in range(121))
    assert sum(h[hb:hb + 8]) == best and all(sum(h[b:b + 8]) < best for b in range(hb))


def test_window_rule_reads_only_the_counts():
    assert list(inspect.signature(bf16pack.window_rule).parameters) == ["hist"]
    assert set(bf16pack.window_rule.__code__.co_names) <= {"int", "len", "range", "sum"}
    W = base_matrix(8, 64)
    assert bf16pack.window_rule(bf16pack.histogram12(W)) == bf16pack.pack12(W, 2)["hb"] == HB
    assert int(bf16pack.histogram12(W).sum()) == W.numel()


# ------------------------------------------------------------------------------------------------ the 8-slot limit
@pytest.mark.parametrize("rows", [2, 4])
def test_eight_misses_fit_and_nine_flag(rows):
    W = base_matrix(3 * rows, 64, seed=3)
    for i in range(8):                                                # group 0: exactly 8
        W[i % rows, 8 * (i % 8) + i // rows % 8] = from_fields(0, 0)
    for i in range(9):                                                # group 1: 9
        W[rows + i % rows, 7 * i % 64] = from_fields(1, 1, i)
    assert bf16pack.miss_rule12(W, HB)[:rows].sum() == 8 and bf16pack.miss_rule12(W, HB)[rows:2 * rows].sum() == 9
    p = bf16pack.pack12(W, rows)
    assert bf16pack.flagged_groups(p).tolist() == [False, True, False] and p["flagged"] == 1
    assert bf16pack.slots_used(p).tolist() == [8, 0, 0]               # a flagged group's record is empty
    assert p["flags"].tolist() == [2]
    back, flagged = bf16pack.unpack12(p)
    assert torch.equal(flagged, torch.tensor([False, True, False]).repeat_interleave(rows))
    assert torch.equal(bits(back)[~flagged], bits(W)[~flagged])


# ------------------------------------------------------------------------------------------------ the padded last group
@pytest.mark.parametrize("rows,N", [(2, 5), (4, 5), (4, 7), (4, 9)])
def test_partial_last_group_is_padded(rows, N):
    """The rows that pad the last group hold zero low bytes and zero nibbles and are no misses, as in the 13-bit set."""
    W = base_matrix(N, 64, seed=N)
    W[N - 1, 13] = from_fields(1, 0)                                  # one real miss in the last group
    p = bf16pack.pack12(W, rows)
    G = (N + rows - 1) // rows
    assert tuple(p["lo"].shape) == (G, rows // 2, 8, 16) and tuple(p["nib"].shape) == (G, 8, rows, 4) and tuple(p["patch"].shape) == (G, 8)
    assert torch.equal(p["lo"], bf16pack.pack(W, rows)["lo"])         # the low plane is the 13-bit set's
    pad = range(N - (G - 1) * rows, rows)
    for r in pad:
        assert not p["nib"][G - 1, :, r].any() and not p["lo"][G - 1, r // 2, :, 8 * (r & 1):8 * (r & 1) + 8].any()
    assert bf16pack.slots_used(p).tolist() == [0] * (G - 1) + [1] and p["flagged"] == 0
    assert slot_fields(p["patch"][G - 1, 0])[:3] == (1, (N - 1) % rows, 5)
    back, flagged = bf16pack.unpack12(p)
    assert back.shape == W.shape and not flagged.any() and torch.equal(bits(back), bits(W))


# ------------------------------------------------------------------------------------------------ which format a matrix takes
@pytest.mark.parametrize("rows,K", [(2, 6656), (2, 17920), (4, 6656), (2, 64), (4, 32)])
def test_set_bits_around_its_break_even(rows, K):
    """12 bits exactly while (12 w + 256) G + 16 w f < 13 w G, w = rows K: enumerated one flagged group either side of the break-even."""
    G = 4096
    w = rows * K
    edge = (w - 256) * G // (16 * w)                                  # the largest f with 16 w f <= (w - 256) G
    for f in range(max(0, edge - 2), edge + 3):
        want = 12 if (12 * w + 256) * G + 16 * w * f < 13 * w * G else 13
        assert bf16pack.set_bits(f, G, rows, K) == want
    assert bf16pack.set_bits(0, G, rows, K) == (12 if w > 256 else 13)            # a 128-weight group's record outweighs its sign bits
    assert bf16pack.set_bits(G, G, rows, K) == 13
    assert bf16pack.set_bits(0, G, rows, K, False) == 13 and bf16pack.set_bits(0, 0, rows, K) == 13
    if w > 256:
        assert bf16pack.set_bits(edge + 1, G, rows, K) == 13 and edge / G < 1 / 16                    # just under one group in 16


def test_heavy_tails_stay_on_13_bits_and_the_bench_law_takes_12():
    g = torch.Generator().manual_seed(4)
    W = (torch.randn(512, 6656, generator=g) * 0.02).to(BF16)
    p = bf16pack.pack12(W, 4)
    assert p["flagged"] == 0 and bf16pack.set_bits(p["flagged"], 128, 4, 6656) == 12
    chi = torch.randn(4, 512, 6656, generator=g).pow(2).sum(0)       # Student-t(4) = N / sqrt(chi2_4 / 4)
    T = (torch.randn(512, 6656, generator=g) / (chi / 4).sqrt() * 0.02).to(BF16)
    pt = bf16pack.pack12(T, 4)
    assert pt["flagged"] > 128 // 16 and bf16pack.set_bits(pt["flagged"], 128, 4, 6656) == 13


def test_default_pack_is_untouched():
    assert list(inspect.signature(bf16pack.default_pack).parameters) == ["env", "world_size", "bf16_released", "need", "free"]
    assert bf16pack.default_pack(None, 1, False, 1, 4) == "all" and bf16pack.default_pack(None, 2, False, 1, 4) == "plain"
