"""Wall time of the image front end and back end, host path against GPU path, same process, interleaved.

    python tools/preprocess_time.py [--reps 20] [--json out.json]

In: from "PIL image in hand" to "device tensor ready" (stream synchronised) for one image and for 8 frames at 448 x 448, 600 x 800,
1080 x 1920 and 3024 x 4032 -- ``image_transform(img).to(dev)`` (the option-off path) against ``GpuImageTransform`` -- and the new path
split into ``np.asarray``, staging + H2D copy and the kernels (events around the launches; per-kernel times come from a
``rocprofv3 --kernel-trace --stats -- python tools/preprocess_time.py`` run of its own).
Out: the 1024 x 1024 tail of ``EmuVisualGeneration.forward``: ``.cpu().permute().float().numpy()`` + ``numpy_to_pil`` against
``to_uint8_hwc(...).cpu()`` + ``Image.fromarray``.  Medians over ``--reps`` alternating repetitions after a warm-up."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch
from PIL import Image

from emu_amd.chat import image_transform
from emu_amd.diffusion import EmuVisualGeneration
from emu_amd.preprocess import GpuImageTransform, to_uint8_hwc

SHAPES = [(448, 448), (600, 800), (1080, 1920), (3024, 4032)]


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    tf = GpuImageTransform(448, device=dev)
    rng = np.random.default_rng(0)
    rows = []
    for h, w in SHAPES:
        for n in (1, 8):
            imgs = [Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for _ in range(n)]
            host = lambda: torch.stack([image_transform(i) for i in imgs]).to(dev)
            gpu = lambda: tf.batch(imgs)
            assert torch.equal(gpu(), host().to(torch.bfloat16))
            arrays = [np.asarray(i) for i in imgs]
            plan = tf.plan(h, w)
            srcs = [torch.from_numpy(x.copy()).to(dev) for x in arrays]
            out = torch.empty(n, 3, 448, 448, device=dev, dtype=torch.bfloat16)
            ws = torch.empty(max(plan.ws_bytes, 1), device=dev, dtype=torch.uint8)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def kernels():
                e0.record()
                for i, s in enumerate(srcs):
                    tf.run(plan, s, out[i], ws)
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)
            t = {k: [] for k in ("host", "gpu", "asarray", "stage", "kernels")}
            reps = max(3, a.reps // (4 if h * w * n > 2e7 else 1))
            for r in range(reps + 2):
                s = {"host": wall(host), "gpu": wall(gpu)}
                t0 = time.perf_counter()
                arr = [np.asarray(i) for i in imgs]
                s["asarray"] = (time.perf_counter() - t0) * 1e3
                s["stage"] = wall(lambda: tf._stage(arr))
                s["kernels"] = kernels()
                if r >= 2:                                                    # two warm-up rounds
                    for k in t:
                        t[k].append(s[k])
            row = {"in": f"{h}x{w}", "images": n, "reps": reps, **{k + "_ms": round(statistics.median(v), 3) for k, v in t.items()},
                   "source_MB": round(h * w * 3 * n / 1e6, 2)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    x = torch.rand(1, 3, 1024, 1024, device=dev).to(torch.bfloat16)
    old = lambda: EmuVisualGeneration.numpy_to_pil(x.cpu().permute(0, 2, 3, 1).float().numpy())[0]
    new = lambda: Image.fromarray(to_uint8_hwc(x).cpu().numpy()[0])
    assert np.array_equal(np.asarray(old()), np.asarray(new()))
    t_old, t_new = [], []
    for r in range(a.reps + 2):
        o, n_ = wall(old), wall(new)
        if r >= 2:
            t_old.append(o); t_new.append(n_)
    tail = {"out": "1024x1024", "host_tail_ms": round(statistics.median(t_old), 3), "gpu_tail_ms": round(statistics.median(t_new), 3)}
    print(json.dumps(tail), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"in": rows, "out": tail, "cpus": len(os.sched_getaffinity(0)), "pillow": Image.__version__}, f, indent=1)


if __name__ == "__main__":
    main()
