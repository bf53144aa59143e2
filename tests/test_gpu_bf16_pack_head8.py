"""GPU: the packed head form with two 4-row groups (8 rows) per workgroup (csrc/gemv_pack.hip, gemv_pack_head_kernel<EPI, 2>) against
emu_linear_bf16 on the bf16 matrix, on the raw bits with a NaN guard band behind the row: one group, a lone trailing group, a padded
last group and whole pairs; short rows, the 2048 trip boundary, a ragged last trip and the true width; workgroups with neither, one
and both groups flagged; the true shapes once each."""
import pytest
import torch

from tests.test_gpu_bf16_pack import BF16, EPI_NONE, EPI_SWIGLU, HEAD, _case, _matrix

pytestmark = pytest.mark.gpu

KS = [32, 64, 2048, 2080, 6656]


def _planted_groups(order, K):
    """[4 len(order), K]: the planted matrix of tests/test_bf16_pack_format.py cut into its three 4-row groups -- "A" (rows 0..3) and
    "B" (rows 4..7) hold planted weights and flag, "C" (rows 8..11, with the matrix's largest exponent) does not -- and laid out in
    ``order``, in front of K - 64 further columns inside the window."""
    from tests.test_bf16_pack_format import planted_matrix
    P = planted_matrix()[0]
    cut = {"A": P[0:4], "B": P[4:8], "C": P[8:12]}
    W = torch.cat([cut[c] for c in order])
    if K > 64:
        g = torch.Generator().manual_seed(K)
        more = (torch.randn(W.shape[0], K - 64, generator=g) * 0.02).to(BF16)
        more = torch.where(more.float().abs() < 2.0 ** -20, torch.full_like(more, 0.01), more)     # no accidental outsiders
        W = torch.cat([W, more], dim=1)
    return W.contiguous()


# workgroup b owns groups 2b and 2b + 1: (C A) and (B C) one flagged, (A B) both, (C C) neither; then an odd count whose lone last
# group is clean, and one whose lone last group is flagged
ORDERS = ["CABCABCC", "CABCABC", "CABCA"]


def _pairs(fl):
    return {(bool(fl[i]), bool(fl[i + 1]) if i + 1 < len(fl) else None) for i in range(0, len(fl), 2)}


def test_planted_orders_hold_every_kind_of_workgroup():
    """On the CPU, from bf16pack.flagged_groups: neither, one (either side) and both groups of a workgroup flagged all occur."""
    from emu_amd import bf16pack
    got = _pairs(bf16pack.flagged_groups(bf16pack.pack(_planted_groups(ORDERS[0], 64), 4)).tolist())
    assert got == {(False, True), (True, False), (True, True), (False, False)}
    assert (False, None) in _pairs(bf16pack.flagged_groups(bf16pack.pack(_planted_groups(ORDERS[1], 64), 4)).tolist())
    assert (True, None) in _pairs(bf16pack.flagged_groups(bf16pack.pack(_planted_groups(ORDERS[2], 64), 4)).tolist())


@pytest.mark.parametrize("epi", [EPI_NONE, EPI_SWIGLU])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", [4, 6, 8, 10, 12, 16, 20])
def test_head_form_groups_and_tails(N, K, epi):
    _case(_matrix(N, K, seed=N * 7 + K), HEAD, 4, epi, True, seed=K + N + epi)


@pytest.mark.parametrize("epi", [EPI_NONE, EPI_SWIGLU])
@pytest.mark.parametrize("K", [64, 2080, 6656])
@pytest.mark.parametrize("order", ORDERS)
def test_flagged_neither_one_and_both(order, K, epi):
    """The planted Inf / NaN rows give Inf / NaN in both kernels: the comparison is on the bits all the same.  K = 2080 and 6656: a
    flagged workgroup streams the bf16 rows over more than one trip."""
    from emu_amd import bf16pack
    W = _planted_groups(order, K)
    fl = bf16pack.flagged_groups(bf16pack.pack(W, 4)).tolist()
    assert fl == [c != "C" for c in order]
    _case(W, HEAD, 4, epi, True, seed=len(order) * 10 + epi + K, finite=False)


@pytest.mark.parametrize("N,epi", [(19968, EPI_NONE), (35840, EPI_SWIGLU), (32274, EPI_NONE)], ids=["qkv", "gateup", "lm_head"])
def test_true_shapes(N, epi):
    """qkv, gate/up (SwiGLU) and an lm_head of 8069 groups (odd: the last workgroup owns one group), K = 6656."""
    _case(_matrix(N, 6656, seed=N), HEAD, 4, epi, True, seed=N + epi)
