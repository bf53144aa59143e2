"""Bit-for-bit check of the UNet's transformer-block path between two builds of libemu_hip.so: the tiny UNet of
tests/test_gpu_unet.py::tiny_unet (channels 64 / 128 / 256, heads 1 / 2 / 4, depths 1 / 1 / 2, cross dim 128, synth seed 5) over the
product of latents 8 x 8 (level 1 has 16 tokens per batch element; level 2 has 8 rows, the few-row stream, which has no GEGLU
epilogue: the forward answers -22 there, after level 1 has run), 16 x 16 and 32 x 32 (every level on whole 64-key groups); 8 and 70
prompt tokens (70: above the cross-attention epilogue's 64 keys, padded to 128); fusion masks 0..7; fp8 off and on; the CFG pair and
either row of it.  Per case it writes the status of emu_unet_forward, the sha256 of the noise prediction and the launches the profiler
recorded (class, M, N, K, tag = epilogue | fused-feature bits << 8, count; in order of first appearance; the distinct lists are kept
once, under "launch tables", and a case names its list): which path ran.  For the
pair, masks 0 and 7, where the forward ran, also the sha256 of the latents after 2 denoise steps, eager and replayed from the captured
graph.  As JSON:

    python tools/unet_forward_equiv.py new.json
    EMU_HIP_TOOLS=1 EMU_HIP_LIB=/path/to/other/libemu_hip.so python tools/unet_forward_equiv.py other.json

Equal files = equal bits and equal launches in every case (profiles/unet_block_refactor_equivalence.md)."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

BF16 = torch.bfloat16
out_path = sys.argv[1] if len(sys.argv) > 1 else "unet_forward_equiv.json"
res = {"launch tables": {}}       # the distinct launch lists, by digest; a case names its list


def save():
    with open(out_path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in res.items()) + "\n}\n")


def h(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:24]


def rand(*shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(BF16).cuda()


def make_engine():
    from emu_amd import synth
    from emu_amd.llama import EmuHipContext
    from emu_amd.unet import UNetCfg, UNetEngine, unet_param_shapes
    cfg = UNetCfg(block_out_channels=(64, 128, 256), transformer_layers_per_block=(1, 1, 2), num_heads=(1, 2, 4),
                  cross_attention_dim=128, projection_class_embeddings_input_dim=128 + 6 * 256)
    W = synth.synth_state_dict(unet_param_shapes(cfg), seed=5, dtype=torch.float32)
    W = {k: (v * (2.0 if v.dim() > 1 else 1.0)) for k, v in W.items()}
    eng = UNetEngine(cfg, EmuHipContext(torch.device("cuda", 0)))
    eng.load_state_dict(W)
    return eng


def forward(eng, lat, half):
    """emu_unet_forward on the pair (half = -1) or one row of it: (status, noise prediction, the profiler's rows)."""
    import ctypes as C
    from emu_amd import ops
    from emu_amd._lib import ProfRowC, lib
    _, _, H, W = lat.shape
    ws = eng._workspace(H, W)
    eps = torch.zeros((2 if half < 0 else 1) * H * W, 4, device="cuda", dtype=BF16)
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib().emu_profile_launches(1)
    status = lib().emu_unet_forward(eng.handle, lat.data_ptr(), H, W, eng.temb_table.data_ptr(), eng.sigmas.data_ptr(), st.data_ptr(),
                                    eps.data_ptr(), ws.data_ptr(), ws.numel(), ops.stream(eng.device))
    torch.cuda.synchronize()
    rows = (ProfRowC * 256)()
    n = lib().emu_profile_launches_read(C.cast(rows, C.c_void_p), 256)
    lib().emu_profile_launches(0)
    launches = [[rows[i].klass.decode(), rows[i].M, rows[i].N, rows[i].K, rows[i].tag, rows[i].launches] for i in range(n)]
    return status, eps, launches


def main():
    eng = make_engine()
    with torch.no_grad():
        for side in (8, 16, 32):
            for n_ctx in (8, 70):
                sch = eng.set_timesteps(4)
                eng.set_context(rand(2, n_ctx, 128, seed=100 + n_ctx), 8 * side, 8 * side)
                lat = (rand(1, 4, side, side, seed=side).float() * sch.init_noise_sigma).to(BF16).contiguous()
                for fp8 in (0, 1):
                    eng.use_fp8(bool(fp8))
                    for mask in range(8):
                        assert eng.set_fusion(mask) == mask
                        for half in (-1, 0, 1):
                            eng.set_cfg_half(half)
                            status, eps, launches = forward(eng, lat, half)
                            eng.set_cfg_half(-1)
                            name = f"lat{side}_ctx{n_ctx}_fp8{fp8}_mask{mask}_half{half}"
                            key = hashlib.sha256(json.dumps(launches).encode()).hexdigest()[:12]
                            res["launch tables"][key] = launches
                            res[name] = {"status": status, "eps": h(eps), "launches": key}
                        if mask in (0, 7) and status == 0:
                            for graph in (False, True):
                                eng.set_timesteps(4)
                                eng._graph = None
                                out = eng.denoise(lat.clone(), 3.0, use_graph=graph, steps=2)
                                res[f"lat{side}_ctx{n_ctx}_fp8{fp8}_mask{mask}_half-1"]["denoise2_graph" if graph else "denoise2_eager"] = h(out)
                    print(f"lat{side} ctx{n_ctx} fp8{fp8} done", flush=True)
                    save()
                eng.use_fp8(False)
                eng.set_fusion(7)
    save()
    print("EQUIV DONE", len(res) - 1, "cases,", len(res["launch tables"]), "distinct launch lists", flush=True)


if __name__ == "__main__":
    main()
