"""CPU: the token-row partition of the token-parallel ViT encode (emu_amd/tp.py::token_rows) and, over gloo worlds of 2 and 3
processes, the row split itself restated on the oracle's ViT blocks: every rank runs the stem and every block on its own token
rows only, all-gathers K and V of every block, and gathers the final rows -- the result equals the unsplit oracle forward."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from emu_amd.tp import token_rows


@pytest.mark.parametrize("N", [17, 1025])
@pytest.mark.parametrize("world", range(1, 9))
def test_token_rows_partition(N, world):
    rr = [token_rows(N, r, world) for r in range(world)]
    assert rr[0][0] == 0 and rr[-1][1] == N                            # covers [0, N)
    assert all(rr[r][1] == rr[r + 1][0] for r in range(world - 1))     # contiguous and disjoint
    assert all(r0 <= r1 for r0, r1 in rr)
    assert rr[0][1] > 0                                                 # CLS (row 0) on rank 0
    assert all(r0 % 8 == 0 for r0, r1 in rr if r1 > r0)                 # the V^T epilogue's 8-key groups
    assert all(r1 % 8 == 0 or r1 == N for _, r1 in rr)
    groups = [(r1 - r0 + 7) // 8 for r0, r1 in rr]
    assert max(groups) - min(groups) <= 1                               # balanced to one 8-row group


def test_token_rows_zero_row_rank_and_true_width():
    assert [token_rows(17, r, 4) for r in range(4)] == [(0, 8), (8, 16), (16, 17), (17, 17)]
    assert [token_rows(1025, r, 8)[1] - token_rows(1025, r, 8)[0] for r in range(8)] == [136] + [128] * 6 + [121]
    with pytest.raises(ValueError):
        token_rows(17, 4, 4)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _all_gather_rows(t, rank, world, rows):
    """Rows [r0, r1) of every rank, concatenated in rank order (gloo all_gather needs equal shapes: padded to the largest)."""
    most = max(r1 - r0 for r0, r1 in rows)
    pad = t.new_zeros((most,) + tuple(t.shape[1:]))
    pad[: t.shape[0]] = t
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad)
    return torch.cat([parts[r][: rows[r][1] - rows[r][0]] for r in range(world)], dim=0)


def _split_forward(image, W, cfg, rank, world):
    """oracle/emu2_ref.vit_forward of one image, this rank's token rows only, K / V all-gathered in every block."""
    from oracle import emu2_ref as R
    rows = [token_rows(cfg.tokens, r, world) for r in range(world)]
    r0, r1 = rows[rank]
    x = torch.cat((W["visual.cls_token"][0], R.vit_patch_embed(image, W)[0]), dim=0) + W["visual.pos_embed"][0]
    x = x[r0:r1]                                                        # own rows of the stem
    H, C = cfg.heads, x.shape[-1]
    for i in range(cfg.layers):
        pre = f"visual.blocks.{i}."
        bias = torch.cat((W[pre + "attn.q_bias"], torch.zeros_like(W[pre + "attn.v_bias"]), W[pre + "attn.v_bias"]))
        qkv = F.linear(x, W[pre + "attn.qkv.weight"], bias).reshape(-1, 3, H, cfg.head_width)
        kv = _all_gather_rows(qkv[:, 1:].contiguous(), rank, world, rows)  # every rank's K and V rows
        q = qkv[:, 0].transpose(0, 1) * (cfg.head_width ** -0.5)
        k, v = kv[:, 0].transpose(0, 1), kv[:, 1].transpose(0, 1)
        o = ((q @ k.transpose(-2, -1)).softmax(dim=-1) @ v).transpose(0, 1).reshape(-1, H * cfg.head_width)
        a = F.linear(o, W[pre + "attn.proj.weight"], W[pre + "attn.proj.bias"])
        x = x + F.layer_norm(a, (C,), W[pre + "norm1.weight"], W[pre + "norm1.bias"], cfg.ln_eps)
        x = x + F.layer_norm(R.vit_mlp(x, W, i), (C,), W[pre + "norm2.weight"], W[pre + "norm2.bias"], cfg.ln_eps)
    return _all_gather_rows(x, rank, world, rows)[None]


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle import emu2_ref as R
        from tests import tiny
        z = tiny.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"), "vit_tiny.npz")
        v, l, vocab, W = tiny.weights_from(z)
        cfg = tiny.oracle_cfg(v, l, vocab).vit
        errs = []
        for j in range(z["image"].shape[0]):
            image = torch.from_numpy(z["image"][j:j + 1]).float()
            got = _split_forward(image, W, cfg, rank, world)
            want = R.vit_forward(image, W, cfg)
            errs.append(float((got - want).norm() / want.norm()))
        q.put((rank, max(errs)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_token_split_gloo_matches_unsplit_oracle(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    [p.start() for p in procs]
    res = [q.get(timeout=180) for _ in procs]
    [p.join(60) for p in procs]
    assert sorted(r for r, _ in res) == list(range(world))
    assert all(err < 1e-5 for _, err in res), res
