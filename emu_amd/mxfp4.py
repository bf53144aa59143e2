"""MXFP4 (OCP microscaling, 4-bit) weight format of the optional fp4 decode stream: the definition, in pure torch.

A packed weight matrix ``[N, K]`` (``K % 32 == 0``) is stored as

* elements ``uint8 [N, K/2]``: element ``2j`` in the low nibble of byte ``j``, element ``2j+1`` in the high nibble.  A code is a
  sign bit (8) and an E2M1 magnitude index: 0, 0.5, 1, 1.5, 2, 3, 4, 6;
* scales ``uint8 [N, K/32]``, E8M0: one per block of 32 consecutive elements of a row, ``scale = 2 ** (byte - 127)``.  The
  matrix-core kernels want the scale rows at a stride of ``scale_stride(K)`` bytes, which is more than ``K/32`` where K is no
  multiple of 256: ``pad_scales``.

``quantize_rows`` is round-to-nearest with the OCP MX scale rule: for a block with ``amax > 0`` the exponent is
``e = floor(log2(amax)) - 2`` clamped to [-126, 125] (so ``amax / 2**e`` lies in [4, 8) and magnitudes above 6 saturate), an
all-zero block gets byte 127, byte 255 is never produced; ``w / 2**e`` is rounded to the nearest grid point, ties to the even
code; the sign is kept (-0 may occur).  Every dequantised value is exactly representable in bf16, and quantising a dequantised
matrix returns the same bytes.

This module is what the HIP kernels (csrc/gemv_fp4.hip) are pinned against, and what users prepare tensors with offline
(``LlamaEngine.load_fp4``); it runs on the CPU or on the device and imports nothing but torch.  Quality on a trained
checkpoint is NOT measured by this project (round-to-nearest on Gaussian weights: 0.114 relative L2): a calibrated quantiser
may produce the same two tensors by any method.
"""
from typing import Tuple

import torch

BLOCK = 32
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
E_MIN, E_MAX = -126, 125


def pack_codes(codes: torch.Tensor) -> torch.Tensor:
    """codes uint8 [..., K] (values 0..15) -> bytes uint8 [..., K/2]: element 2j low nibble, 2j+1 high nibble."""
    assert codes.dtype == torch.uint8 and codes.shape[-1] % 2 == 0
    c = codes.reshape(*codes.shape[:-1], codes.shape[-1] // 2, 2)
    return (c[..., 0] | (c[..., 1] << 4)).contiguous()


def unpack_codes(packed: torch.Tensor) -> torch.Tensor:
    """bytes uint8 [..., K/2] -> codes uint8 [..., K]."""
    assert packed.dtype == torch.uint8
    return torch.stack((packed & 15, packed >> 4), dim=-1).reshape(*packed.shape[:-1], packed.shape[-1] * 2)


def decode_codes(codes: torch.Tensor) -> torch.Tensor:
    """codes uint8 -> fp32 values of the unscaled E2M1 elements (-0 for code 8)."""
    grid = torch.tensor(GRID, dtype=torch.float32, device=codes.device)
    mag = grid[(codes & 7).long()]
    return torch.where((codes & 8) != 0, -mag, mag)


def scale_values(scales: torch.Tensor) -> torch.Tensor:
    """E8M0 bytes -> fp32 powers of two, 2 ** (byte - 127) (byte 0 gives the fp32 denormal 2 ** -127)."""
    assert scales.dtype == torch.uint8
    return torch.ldexp(torch.ones((), dtype=torch.float32, device=scales.device), scales.to(torch.int32) - 127)


def quantize_rows(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """w [N, K] (bf16 / fp16 / fp32, K % 32 == 0) -> (packed uint8 [N, K/2], scales uint8 [N, K/32])."""
    if w.dim() != 2 or w.shape[1] % BLOCK:
        raise ValueError(f"quantize_rows: expected [N, K] with K % {BLOCK} == 0, got {tuple(w.shape)}")
    wf = w.to(torch.float32)
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("quantize_rows: non-finite weight")
    N, K = wf.shape
    blk = wf.reshape(N, K // BLOCK, BLOCK)
    amax = blk.abs().amax(dim=-1)
    # amax = m * 2**x with m in [0.5, 1): floor(log2(amax)) = x - 1, exact for every finite positive float
    _, x = torch.frexp(amax)
    e = (x.to(torch.int32) - 3).clamp(E_MIN, E_MAX)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    # exact: a power-of-two factor (the product of a tiny element under a large amax may underflow -- it rounds to code 0 anyway)
    a = (blk * torch.ldexp(torch.ones((), dtype=torch.float32, device=wf.device), -e)[..., None]).abs()
    # nearest grid point, ties to the even code: the midpoints 0.25 / 1.25 / 2.5 / 5 fall to the code below, 0.75 / 1.75 / 3.5 above
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8) + (a >= 1.75).to(torch.uint8)
            + (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8) + (a > 5.0).to(torch.uint8))
    code = code | (torch.signbit(blk).to(torch.uint8) << 3)
    return pack_codes(code.reshape(N, K)), (e + 127).to(torch.uint8)


def dequantize(packed: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """(packed uint8 [N, K/2], scales uint8 [N, K/32]) -> fp32 [N, K]; every value is exact in bf16."""
    if packed.dim() != 2 or scales.dim() != 2 or packed.shape[0] != scales.shape[0] or packed.shape[1] != scales.shape[1] * (BLOCK // 2):
        raise ValueError(f"dequantize: shapes {tuple(packed.shape)} / {tuple(scales.shape)} are not [N, K/2] / [N, K/32]")
    N = packed.shape[0]
    v = decode_codes(unpack_codes(packed)).reshape(N, -1, BLOCK)
    return (v * scale_values(scales)[..., None]).reshape(N, -1)


def scale_stride(K: int) -> int:
    """Bytes between the scale rows of a [N, K] matrix as the matrix-core kernels want them (``fp4_scale_stride`` in
    csrc/kernels.h): they fetch the 8 scale bytes of a 256-wide K stage by 4-byte DMA, so a row spans whole stages.  ``K / 32``
    where ``K % 256 == 0`` (nothing to pad), else ``8 * ceil(K / 256)``: 32 for K = 896, 72 for K = 2240."""
    if K < BLOCK or K % BLOCK:
        raise ValueError(f"scale_stride: K = {K} is not a positive multiple of {BLOCK}")
    return K // BLOCK if K % 256 == 0 else 8 * ((K + 255) // 256)


def pad_scales(scales: torch.Tensor, K: int) -> torch.Tensor:
    """scales uint8 [N, K/32] -> uint8 [N, scale_stride(K)], the new columns filled with byte 127 (2 ** 0; the kernels read them
    and never use them).  ``padded[:, :K // 32]`` is the input again; where ``K % 256 == 0`` the input itself is returned."""
    if scales.dtype != torch.uint8 or scales.dim() != 2 or scales.shape[1] != K // BLOCK:
        raise ValueError(f"pad_scales: expected uint8 [N, {K // BLOCK}] for K = {K}, got {scales.dtype} {tuple(scales.shape)}")
    stride = scale_stride(K)
    if stride == scales.shape[1]:
        return scales
    out = torch.full((scales.shape[0], stride), 127, dtype=torch.uint8, device=scales.device)
    out[:, :scales.shape[1]] = scales
    return out


def bytes_per_row(K: int) -> int:
    """Bytes one weight row of K elements streams: K/2 element bytes + K/32 scale bytes."""
    return K // 2 + K // BLOCK
