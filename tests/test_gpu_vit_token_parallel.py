"""GPU: the token-parallel ViT encode of one image (emu_vit_forward_tp, VitEngine.forward_token_parallel).  Ranks sharing this GPU
(EMU_TP_SHARED_GPU=1) run tests/vit_tp_worker.py under torch.distributed.run, as test_engine_tp_ranks_sharing_one_gpu does; world 1
and the fp8 refusal run in this process."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import tiny

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _run_worker(world, *args):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", EMU_TP_SHARED_GPU="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "vit_tp_worker.py"), *args]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("token-parallel ViT ok") == world, r.stdout[-3000:]
    return r.stdout


@pytest.mark.parametrize("world", [2, 4])
def test_vit_token_parallel_ranks_sharing_one_gpu(world):
    """Tiny fixture image by image (bit-identical tokens on every rank, the bounds of test_vit_and_encode_image, own rows only,
    eager == hipGraph replay, no give-up) and the true EVA-CLIP-4B block width against the replicated forward; at world 2 also
    EmuModel(vit_token_parallel=True) end to end: greedy ids with an image == generate_tiny.npz."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    out = _run_worker(world, *(["--e2e"] if world == 2 else []))
    if world == 2:
        assert out.count("e2e ids match") == 2, out[-3000:]


def _tiny_vit(golden_dir):
    from emu_amd.llama import EmuHipContext
    from emu_amd.vit import VitEngine
    z = tiny.load(golden_dir, "vit_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    ctx = EmuHipContext(torch.device("cuda", 0))
    vit = VitEngine(v, ctx)
    vit.load_weights(W.items())
    return vit, z


def test_vit_token_parallel_world1_is_the_replicated_forward(golden_dir):
    vit, z = _tiny_vit(golden_dir)
    vit.init_token_parallel(0, 1)
    for j in range(z["image"].shape[0]):
        image = torch.from_numpy(np.asarray(z["image"][j:j + 1])).to(BF16).cuda()
        want = vit.forward(image)
        got = vit.forward_token_parallel(image)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        assert vit.rows_computed() == (0, vit.cfg.tokens)


def test_vit_token_parallel_refuses_fp8_blocks():
    from emu_amd import CLIPVisionCfg, synth
    from emu_amd._lib import EmuHipError
    from emu_amd.llama import EmuHipContext
    from emu_amd.vit import VitEngine
    v = CLIPVisionCfg(image_size=56, patch_size=14, width=256, layers=1, head_width=128, mlp_ratio=2.0)
    vit = VitEngine(v, EmuHipContext(torch.device("cuda", 0)))
    vit.load_weights(synth.iter_synth(synth.vit_param_shapes(v), seed=5, device="cuda", dtype=BF16))
    vit.init_token_parallel(0, 1)
    vit.use_fp8(True)
    with pytest.raises(EmuHipError):
        vit.forward_token_parallel(torch.randn(1, 3, 56, 56, device="cuda"))
