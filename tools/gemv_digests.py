#!/usr/bin/env python
"""sha256 of the output of one seeded call per kernel family of the few-row weight-stream plan (csrc/gemv.hip::gemv_plan) and
epilogue, for a bit-for-bit comparison of two builds (needs a GPU):

    python tools/gemv_digests.py > this.txt
    EMU_HIP_TOOLS=1 EMU_HIP_LIB=<other libemu_hip.so> python tools/gemv_digests.py > other.txt

One line per case.  bf16, one row: the single round trip with 4 trips (520, 6656) and 9 trips (96, 17920), the wave form (1030, 64) and
(2050, 2240); under ``emu_gemm_tune`` bit 17 the block kernel's head (520, 6656, norm), preload (520, 6656) and rolling (96, 17920,
norm) forms.  The block kernel at 2 / 3 / 5 / 8 rows on (64, 256) and (1002, 896) (K = 256 at 5 / 8 rows: the thin stream); the register-fed MFMA kernel at 9 / 13 rows on
(50, 64); the thin stream at 4 / 8 / 16 rows on (50, 256) and (264, 768).  fp8: the round trip (1, 1000, 6656), the block kernel with
8-byte loads (2, 1000, 6656) and with 16-byte loads (2, 38, 8208).  MXFP4 rows at 1 / 2 rows on (37, 256) and (64, 1536).  Every
epilogue the family has (SwiGLU on an even N).  Seeded inputs; the summation order does not depend on the build, so equal digests are
the bar (profiles/gemv_plan_refactor_equivalence.md).
"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from emu_amd import _lib, ops  # noqa: E402

BF16 = torch.bfloat16
BLOCK_ONLY = 1 << 17


def digest(t):
    return hashlib.sha256(t.contiguous().view(torch.int16).cpu().numpy().tobytes()).hexdigest()


def run(kind, what, M, N, K, norm, epis, tune=0):
    for epi in epis:
        n = N + 1 if epi == ops.EPI_SWIGLU and N & 1 else N
        g = torch.Generator().manual_seed(1000 * M + n + K + 7 * epi)
        w = (torch.randn(n, K, generator=g) * 0.03).to(BF16).cuda()
        x = torch.randn(M, K, generator=g).to(BF16).cuda()
        bias = torch.randn(n, generator=g).to(BF16).cuda()
        res = torch.randn(M, n, generator=g).to(BF16).cuda()
        nw = (1 + 0.1 * torch.randn(K, generator=g)).to(BF16).cuda()
        kw = dict(bias=bias, res=res if epi == ops.EPI_RESID else None, norm_w=nw if norm else None, eps=1e-5 if norm else 0.0, epi=epi)
        _lib.lib().emu_gemm_tune(tune)
        try:
            if kind == "fp8":
                out = ops.linear_fp8w(x, *ops.quantize_fp8_rows(w), **kw)
            elif kind == "fp4":
                out = ops.linear_fp4w(x, *ops.quantize_mxfp4_rows(w), **kw)
            else:
                out = ops.linear(x, w, **kw)
        finally:
            _lib.lib().emu_gemm_tune(0)
        print(f"{kind} {what} M={M} N={n} K={K} norm={int(norm)} epi={epi} {digest(out)}", flush=True)


def main():
    if not torch.cuda.is_available():
        sys.exit("gemv_digests.py runs the kernels on a GPU; none found")
    all5, three = range(5), (ops.EPI_NONE, ops.EPI_RESID, ops.EPI_SWIGLU)
    run("bf16", "round trip 4 trips", 1, 520, 6656, False, all5)
    run("bf16", "round trip 9 trips", 1, 96, 17920, False, all5)
    for N, K in ((1030, 64), (2050, 2240)):
        run("bf16", "wave", 1, N, K, False, (ops.EPI_NONE, ops.EPI_RESID))
    run("bf16", "block head", 1, 520, 6656, True, all5, BLOCK_ONLY)
    run("bf16", "block preload", 1, 520, 6656, False, all5, BLOCK_ONLY)
    run("bf16", "block rolling", 1, 96, 17920, True, all5, BLOCK_ONLY)
    for M in (2, 3, 5, 8):
        for N, K in ((64, 256), (1002, 896)):
            run("bf16", "block (thin stream: 5 / 8 rows of K = 256)", M, N, K, False, all5)
    for M in (9, 13):
        run("bf16", "register-fed mfma", M, 50, 64, False, all5)
    for M in (4, 8, 16):
        for N, K in ((50, 256), (264, 768)):
            run("bf16", "thin stream", M, N, K, False, all5)
    run("fp8", "round trip", 1, 1000, 6656, False, three)
    run("fp8", "block 8-byte loads", 2, 1000, 6656, False, three)
    run("fp8", "block 16-byte loads", 2, 38, 8208, False, three)
    for M in (1, 2):
        for N, K in ((37, 256), (64, 1536)):
            run("fp4", "rows", M, N, K, False, three)


if __name__ == "__main__":
    with torch.no_grad():
        main()
