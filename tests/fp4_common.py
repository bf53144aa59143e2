"""Helpers shared by the MXFP4 GPU test modules (tests/test_gpu_fp4.py, test_gpu_fp4_wide.py, test_gpu_fp4_gemm.py).  A plain
module: each test module imports what it uses, the ``tiny_fp4`` fixture by name (it is module-scoped, so every importing module
gets its own engine)."""
import ctypes as C

import pytest
import torch

from tests import tiny

BF16 = torch.bfloat16


def rel_err(got, want):
    got, want = got.float().cpu(), want.float().cpu()
    return float((got - want).norm() / want.norm().clamp_min(1e-12))


def bfr(x):
    return x.to(BF16).float()


_CASE = {}


def _case(N, K, seed_extra=0):
    """Weights, their 4-bit tensors on the device and the exact dequantisation, once per shape."""
    from emu_amd import mxfp4, ops
    key = (N, K, seed_extra)
    if key not in _CASE:
        g = torch.Generator().manual_seed(N * 3 + K + seed_extra)
        w = (torch.randn(N, K, generator=g) * 0.03).to(BF16)
        q, sc = ops.quantize_mxfp4_rows(w.cuda())
        _CASE[key] = (q, sc, mxfp4.dequantize(q.cpu(), sc.cpu()))
    return _CASE[key]


def _tiny_model(golden_dir, weights=None):
    from emu_amd import EmuModel, TextDecoderCfg
    z = tiny.load(golden_dir, "generate_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    m = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda")
    m.load_state_dict(W if weights is None else weights, strict=True)
    return m, v, l, vocab, W


@pytest.fixture(scope="module")
def tiny_fp4(golden_dir):
    from emu_amd import mxfp4
    from oracle import emu2_ref as R
    m, v, l, vocab, W = _tiny_model(golden_dir)
    W = R.bf16_round(W)
    W4 = dict(W)
    for k, t in W.items():                       # blocks run along K inside a row: they commute with the row packing
        if k.startswith("decoder.lm.") and t.dim() == 2 and "embed_tokens" not in k:
            W4[k] = mxfp4.dequantize(*mxfp4.quantize_rows(t))
    return m, W, W4, tiny.oracle_cfg(v, l, vocab)


def _f32(cache):
    cache.k = [None if t is None else t.float() for t in cache.k]
    cache.v = [None if t is None else t.float() for t in cache.v]
    return cache


def _gemv_profile(fn):
    """weight_bytes and launches the weight-stream profiler saw while fn ran."""
    from emu_amd._lib import check, lib
    check(lib().emu_profile_gemv(1), "emu_profile_gemv")
    try:
        fn()
        torch.cuda.synchronize()
        ms, wb, nl = C.c_double(), C.c_double(), C.c_long()
        check(lib().emu_profile_gemv_read(C.byref(ms), C.byref(wb), C.byref(nl)), "emu_profile_gemv_read")
    finally:
        check(lib().emu_profile_gemv(0), "emu_profile_gemv")
    return wb.value, nl.value
