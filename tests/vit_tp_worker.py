"""Worker of tests/test_gpu_vit_token_parallel.py: one process per rank (torch.distributed.run), the token-parallel ViT encode of ONE
image (emu_vit_forward_tp: every rank computes its own token rows, K rows and V^T keys exchanged per block over IPC-mapped
regions, csrc/p2p.hip).  Exit code 0 = pass.

EMU_TP_SHARED_GPU=1: every rank uses cuda:0 and the rendezvous is gloo (RCCL refuses two ranks on one device); the exchange uses
the same kernels, flags and IPC mappings a multi-GPU node does, minus the xGMI hop.
  * tiny fixture: every image of vit_tiny.npz encoded alone -- bit-identical tokens on every rank, feats / oracle bounds of
    test_vit_and_encode_image, each rank computed only its own rows, eager == hipGraph replay, no give-up;
  * true width: random weights of the EVA-CLIP-4B shape (1792 wide, 16 heads, 1025 tokens), the first blocks, against the
    replicated (TP = 1) forward of the same engine;
  * end to end (--e2e): EmuModel(vit_token_parallel=True), greedy generate_ids with an image == generate_tiny.npz's ids."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16 = torch.bfloat16


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm())


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    shared = os.environ.get("EMU_TP_SHARED_GPU") == "1"
    local = 0 if shared else int(os.environ["LOCAL_RANK"])
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from emu_amd import CLIPVisionCfg, EmuModel, TextDecoderCfg, synth
    from emu_amd._lib import lib
    from emu_amd.llama import EmuHipContext
    from emu_amd.tp import token_rows
    from emu_amd.vit import VitEngine
    from oracle import emu2_ref as R
    from tests import tiny
    t = lambda a: torch.from_numpy(np.asarray(a))

    def allgather(b):
        box = [None] * world
        dist.all_gather_object(box, b)
        return box

    def same_on_all_ranks(x):
        parts = [torch.empty_like(x.cpu()) for _ in range(world)]
        dist.all_gather(parts, x.cpu().contiguous())
        return all(torch.equal(p.view(torch.int16), parts[0].view(torch.int16)) for p in parts)

    ok = True

    def expect(cond, what):
        nonlocal ok
        if not cond:
            print(f"rank {rank}: FAILED {what}", flush=True)
        ok &= bool(cond)

    ctx = EmuHipContext(dev, rank, world)
    # ---- tiny fixture
    z = tiny.load(os.path.join(ROOT, "tests", "golden"), "vit_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    cfg = tiny.oracle_cfg(v, l, vocab)
    vit = VitEngine(v, ctx)
    vit.load_weights(W.items())
    vit.init_token_parallel(rank, world, allgather, timeout_ms=20000)
    r0, r1 = token_rows(v.tokens, rank, world)
    for j in range(z["image"].shape[0]):
        image = t(z["image"][j:j + 1]).to(BF16)
        dist.barrier()
        got = vit.forward_token_parallel(image.to(dev))
        torch.cuda.synchronize(dev)
        expect(vit.rows_computed() == (r0, r1), f"rows {vit.rows_computed()} != {(r0, r1)}")
        expect(same_on_all_ranks(got), f"image {j}: tokens differ between ranks")
        e_feats, e_ref = rel(got, t(z["feats"][j:j + 1])), rel(got, R.vit_forward(image.float(), W, cfg.vit))
        expect(e_feats < 3e-2 and e_ref < 2e-2, f"image {j}: feats {e_feats:.3e} oracle {e_ref:.3e}")
        # hipGraph: the exchanges' sequence numbers live on the device, so a captured encode replays correctly
        st = torch.cuda.Stream(device=dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        src = image.to(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            out = vit.forward_token_parallel(src)
        dist.barrier()
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize(dev)
        expect(torch.equal(out.view(torch.int16), got.view(torch.int16)), f"image {j}: graph replay != eager")
        del g
    expect(any(token_rows(v.tokens, r, world)[1] - token_rows(v.tokens, r, world)[0] < v.tokens for r in range(world)),
           "some rank computes fewer than all rows")
    print(f"rank {rank}: tiny rows [{r0}, {r1}) of {v.tokens}", flush=True)
    del vit
    # ---- true width: the EVA-CLIP-4B block shape, the first blocks
    wv = CLIPVisionCfg(layers=int(os.environ.get("EMU_VIT_TP_TEST_LAYERS", "2")))
    assert (wv.width, wv.heads, wv.tokens) == (1792, 16, 1025)
    big = VitEngine(wv, ctx)
    big.load_weights(synth.iter_synth(synth.vit_param_shapes(wv), seed=23, device=dev, dtype=BF16))
    big.init_token_parallel(rank, world, allgather, timeout_ms=20000)
    img = torch.randn(1, 3, wv.image_size, wv.image_size, generator=torch.Generator().manual_seed(3)).to(dev)
    want = big.forward(img)
    dist.barrier()
    got = big.forward_token_parallel(img)
    torch.cuda.synchronize(dev)
    e = rel(got, want)
    expect(e < 3e-2, f"true width: {e:.3e} against the replicated forward")
    expect(same_on_all_ranks(got), "true width: tokens differ between ranks")
    print(f"rank {rank}: true width rows {big.rows_computed()} rel {e:.2e}", flush=True)
    del big
    torch.cuda.empty_cache()
    # ---- end to end: EmuModel with the opt-in switch, one image per prompt
    if "--e2e" in sys.argv:
        z = tiny.load(os.path.join(ROOT, "tests", "golden"), "generate_tiny.npz")
        v, l, vocab, W = tiny.weights_from(z)

        def bcast(b):
            box = [b]
            dist.broadcast_object_list(box, src=0)
            return box[0]
        ctx.init_tp(bcast, allgather_bytes=allgather, rccl=not shared, p2p_timeout_ms=20000)
        m = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device=dev, ctx=ctx, vit_token_parallel=True)
        m.load_state_dict(W, strict=True)
        dist.barrier()
        ids = m.generate_ids(t(z["ids1"]), t(z["mask1"]), t(z["image"]).to(dev), max_new_tokens=8).cpu()
        expect(ids.tolist() == z["new1"].tolist(), f"e2e ids {ids.tolist()} != {z['new1'].tolist()}")
        expect(m.visual.rows_computed() == token_rows(v.tokens, rank, world), "e2e: the encode was not token-parallel")
        print(f"rank {rank}: e2e ids match", flush=True)
    torch.cuda.synchronize(dev)
    expect(lib().emu_tp_p2p_giveups() == 0, "give-up counter is not 0")
    flag = torch.tensor([1 if ok else 0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if int(flag.item()) == 1:
        print(f"rank {rank}: token-parallel ViT ok", flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if int(flag.item()) == 1 else 1)


if __name__ == "__main__":
    main()
