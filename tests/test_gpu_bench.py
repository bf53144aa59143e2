"""`bench.py --gpus 1` at reduced depth: a plain run prints the headline line and nothing that needs runs of its own (no roofline,
no extra legs), `--steps` is the number of timed steps, and `--dump-outputs DIR` writes the last timed step's outputs as float32 /
float64 .npy files that are the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps, warmup):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--layers", "2", "--vit-layers", "2", "--dump-outputs", str(out_dir)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "EMU_TP_SHARED_GPU")}
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_and_dump_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    d = _bench(tmp_path / "a", 5, 2)
    assert d["steps"] == 5 and d["warmup"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert {"metric", "unit", "higher_is_better", "dtype"} <= set(d) and d["unit"] == "tokens/s" and d["dtype"] == "bf16"
    assert not {"roofline", "extra", "cpu_baseline", "denoise", "legs", "decode_fp8_weights", "beam_search_5"} & set(d), sorted(d)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("logits", "next_token", "generated_ids")}
    assert got["logits"].dtype == np.float32 and got["logits"].ndim == 2 and got["logits"].shape[0] == 1
    assert np.isfinite(got["logits"]).all()
    assert got["next_token"].dtype == np.float64 and got["generated_ids"].dtype == np.float64
    # the prompt's first new token + one per warm-up and timed step; the last one is the last step's pick
    assert got["generated_ids"].shape == (1 + 2 + 5,) and got["generated_ids"][-1] == got["next_token"][0]
    assert sum(v.nbytes for v in got.values()) < 64 << 20
    # same arguments, same inputs: a second run computes the same outputs
    _bench(tmp_path / "b", 5, 2)
    for n, v in got.items():
        w = np.load(tmp_path / "b" / f"{n}.npy")
        if n == "logits":
            np.testing.assert_allclose(w, v, rtol=1e-2, atol=1e-2)
        else:
            np.testing.assert_array_equal(w, v)
