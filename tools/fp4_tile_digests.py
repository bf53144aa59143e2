#!/usr/bin/env python
"""sha256 of the outputs of the kernels that share csrc/fp4_tile.h, for a bit-for-bit comparison of two builds (needs a GPU):

    python tools/fp4_tile_digests.py > this.txt
    EMU_HIP_TOOLS=1 EMU_HIP_LIB=<other libemu_hip.so> python tools/fp4_tile_digests.py > other.txt

One line per case: ``ops.linear_fp4w_thin`` at M = 3 / 8 / 9 / 16 and ``ops.linear_fp4w_gemm`` at M = 17 / 33 / 65 / 130, each at
(N, K) = (37, 256) (one stage) and (64, 1536) (six stages: deeper than any ring) with bias, with the residual, and SwiGLU (N = 38
for the narrow shape); ``ops.linear`` on bf16 through csrc/gemv_thin.hip at M = 5 / 16, (37, 512), epilogues 0..4 (SwiGLU: N = 38);
``ops.linear_fp8w_thin`` at M = 3 / 5 / 16, (264, 768) and (37, 256), plain / residual / SwiGLU, the weight rows per workgroup pinned to
16 and to 32 (emu_gemm_tune bits 28-29); ``ops.linear_fp4w_mfma`` at K = 896 (a partial last stage), M = 3 / 9 / 16 / 20, N = 264.
Seeded inputs; the summation order does not depend on the build, so equal digests are the bar (profiles/fp4_tile_refactor_equivalence.md).
"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emu_amd import _lib, ops  # noqa: E402

BF16 = torch.bfloat16


def digest(t):
    return hashlib.sha256(t.contiguous().view(torch.int16).cpu().numpy().tobytes()).hexdigest()


def inputs(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) * 0.03).to(BF16).cuda()
    x = torch.randn(M, K, generator=g).to(BF16).cuda()
    bias = torch.randn(N, generator=g).to(BF16).cuda()
    res = torch.randn(M, N, generator=g).to(BF16).cuda()
    return w, x, bias, res


def main():
    if not torch.cuda.is_available():
        sys.exit("fp4_tile_digests.py runs the kernels on a GPU; none found")
    for fn, rows in ((ops.linear_fp4w_thin, (3, 8, 9, 16)), (ops.linear_fp4w_gemm, (17, 33, 65, 130))):
        for M in rows:
            for N, K in ((37, 256), (64, 1536)):
                for what in ("bias", "resid", "swiglu"):
                    n = N + 1 if what == "swiglu" and N & 1 else N
                    w, x, bias, res = inputs(M, n, K, 1000 * M + n + K)
                    q, sc = ops.quantize_mxfp4_rows(w)
                    if what == "bias":
                        out = fn(x, q, sc, bias=bias)
                    elif what == "resid":
                        out = fn(x, q, sc, res=res, epi=ops.EPI_RESID)
                    else:
                        out = fn(x, q, sc, epi=ops.EPI_SWIGLU)
                    print(f"{fn.__name__} M={M} N={n} K={K} {what} {digest(out)}", flush=True)
    for M in (5, 16):
        for epi in range(5):
            N, K = (38 if epi == ops.EPI_SWIGLU else 37), 512
            w, x, bias, res = inputs(M, N, K, 77 * M + epi)
            out = ops.linear(x, w, bias=bias, res=res if epi == ops.EPI_RESID else None, epi=epi)
            print(f"linear(bf16, thin stream) M={M} N={N} K={K} epi={epi} {digest(out)}", flush=True)
    for pin in (1, 2):
        _lib.lib().emu_gemm_tune(pin << 28)
        try:
            for M in (3, 5, 16):
                for N, K in ((264, 768), (37, 256)):
                    for epi in (ops.EPI_NONE, ops.EPI_RESID, ops.EPI_SWIGLU):
                        n = N + 1 if epi == ops.EPI_SWIGLU and N & 1 else N
                        w, x, bias, res = inputs(M, n, K, 31 * M + n + K + epi)
                        q, sc = ops.quantize_fp8_rows(w)
                        out = ops.linear_fp8w_thin(x, q, sc, res=res if epi == ops.EPI_RESID else None, epi=epi)
                        print(f"linear_fp8w_thin pin={pin} M={M} N={n} K={K} epi={epi} {digest(out)}", flush=True)
        finally:
            _lib.lib().emu_gemm_tune(0)
    for M in (3, 9, 16, 20):
        for epi in (ops.EPI_NONE, ops.EPI_RESID, ops.EPI_SWIGLU):
            w, x, bias, res = inputs(M, 264, 896, 13 * M + epi)
            q, sc = ops.quantize_mxfp4_rows(w)
            out = ops.linear_fp4w_mfma(x, q, sc, res=res if epi == ops.EPI_RESID else None, epi=epi)
            print(f"linear_fp4w_mfma M={M} N=264 K=896 epi={epi} {digest(out)}", flush=True)


if __name__ == "__main__":
    with torch.no_grad():
        main()
