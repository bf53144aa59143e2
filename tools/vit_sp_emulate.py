#!/usr/bin/env python
"""Per-rank cost of the token-parallel ViT encode on ONE GPU at the true width (448 x 448, 64 blocks, synthetic weights): one
process runs rank r's token rows (emu_amd/tp.py::token_rows) through the stem and all blocks with the exchanges short-circuited
(emu_vit_set_token_parallel(..., emulate = 1)), next to the replicated encode of the whole image.  The exchanges' cost is not in
these numbers (it is link-bound over xGMI, which one GPU does not have).
Usage: python tools/vit_sp_emulate.py [reps] [tps, e.g. 2,4,8] [--shard TP RANK: time only that shard (for a kernel trace)]"""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from emu_amd import CLIPVisionCfg, synth
from emu_amd.llama import EmuHipContext
from emu_amd.tp import token_rows
from emu_amd.vit import VitEngine

args = sys.argv[1:]
shard = None
if "--shard" in args:
    i = args.index("--shard")
    shard = (int(args[i + 1]), int(args[i + 2]))
    args = args[:i] + args[i + 3:]
reps = int(args[0]) if args else 10
tps = [int(x) for x in args[1].split(",")] if len(args) > 1 else [2, 4, 8]
dev = torch.device("cuda", 0)
v = CLIPVisionCfg(n_query=256, v_query=64)
eng = VitEngine(v, EmuHipContext(dev))
eng.load_weights(synth.iter_synth(synth.vit_param_shapes(v), seed=0, device=dev, dtype=torch.bfloat16))
img = torch.randn(1, 3, v.image_size, v.image_size, device=dev)


def timed(fn, label):
    """hipGraph replay of one encode, median of ``reps`` (HIP events)."""
    st = torch.cuda.Stream(device=dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        fn(); fn()
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        fn()
    g.replay(); torch.cuda.synchronize(dev)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); g.replay(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    print(f"{label}: min {ts[0]:.2f} ms  median {ts[len(ts) // 2]:.2f} ms", flush=True)
    return ts[len(ts) // 2]


with torch.no_grad():
    if shard is not None:
        tp, r = shard
        eng.init_token_parallel(r, tp, emulate=True)
        for _ in range(reps):
            eng.forward_token_parallel(img)
        torch.cuda.synchronize(dev)
        print(f"tp {tp} rank {r}: rows {eng.rows_computed()}, {reps} encodes traced", flush=True)
        sys.exit(0)
    base = timed(lambda: eng.forward(img), "replicated encode (every rank, today)")
    # the token-parallel chain with the whole image on one rank: the same launches as the replicated encode
    eng.init_token_parallel(0, 1)
    timed(lambda: eng.forward_token_parallel(img), "token-parallel, world 1")
    for tp in tps:
        worst = 0.0
        for r in sorted({0, tp - 1}):
            eng.init_token_parallel(r, tp, emulate=True)
            r0, r1 = token_rows(v.tokens, r, tp)
            worst = max(worst, timed(lambda: eng.forward_token_parallel(img), f"tp {tp} rank {r} rows [{r0}, {r1}) ({r1 - r0} rows)"))
        print(f"tp {tp}: per-rank encode {worst:.2f} ms (slowest rank, exchanges excluded) vs {base:.2f} ms replicated: "
              f"{base / worst:.2f}x", flush=True)
