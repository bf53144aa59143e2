"""Tensor-level wrappers of the primitive C-ABI operators (include/emu_hip.h).

PyTorch is only the allocator/stream provider here: every function hands raw device pointers of bf16 CUDA
(ROCm) tensors to libemu_hip.so on torch's current stream.  No function has a torch fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import mxfp4
from ._lib import TokenTrieC, check, lib

EPI_NONE, EPI_RESID, EPI_SWIGLU, EPI_SILU, EPI_GELU, EPI_GEGLU = range(6)
BF16 = torch.bfloat16


def stream(ref=None) -> int:
    """HIP stream handle for one library call: torch's current stream of the device that holds ``ref`` (a tensor or a
    torch.device; None = the current device).  The library launches on that stream without touching the HIP device
    state, and a launch on a stream of another GPU than the calling thread's current one is invalid -- so a ``ref`` on
    another device is refused here (no hidden ``set_device``: one process drives one GPU in this design, and
    ``EmuHipContext`` is the one place that makes its device current)."""
    if ref is None:
        return torch.cuda.current_stream().cuda_stream
    dev = ref.device if isinstance(ref, torch.Tensor) else torch.device(ref)
    if dev.type == "cuda" and dev.index is not None and dev.index != torch.cuda.current_device():
        raise ValueError(f"emu_amd: operand on {dev} but the current device is cuda:{torch.cuda.current_device()}; one process "
                         "drives one GPU -- create the EmuHipContext for that device (it makes it current) or call "
                         "torch.cuda.set_device first")
    return torch.cuda.current_stream(dev).cuda_stream


def _p(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def _req(t: torch.Tensor, name: str, dtype=BF16):
    if not t.is_cuda:
        raise ValueError(f"{name} must be a GPU tensor (emu_amd has no CPU path)")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if t.stride(-1) != 1:
        raise ValueError(f"{name} must be contiguous in its last dimension")


def linear(x, w, bias=None, res=None, norm_w=None, eps: float = 0.0, epi: int = EPI_NONE, out=None):
    """out[m, n] = epi(sum_k x[m, k] w[n, k] + bias[n]); see emu_linear_bf16."""
    _req(x, "x"); _req(w, "w")
    assert x.dim() == 2 and w.dim() == 2 and x.shape[1] == w.shape[1], (x.shape, w.shape)
    M, K = x.shape
    N = w.shape[0]
    n_out = N // 2 if epi in (EPI_SWIGLU, EPI_GEGLU) else N
    if out is None:
        out = torch.empty(M, n_out, device=x.device, dtype=BF16)
    _req(out, "out")
    if res is not None:
        _req(res, "res")
    check(lib().emu_linear_bf16(_p(x), _p(w), _p(bias), _p(res), _p(norm_w), _p(out), M, N, K,
                                x.stride(0), w.stride(0), res.stride(0) if res is not None else 0,
                                out.stride(0), float(eps), int(epi), stream(x)), "emu_linear_bf16")
    return out


def linear_fused(x, w, bias=None, res=None, epi: int = EPI_NONE, out=None, stats_out=None, ln=None, vt=None, cross=None):
    """emu_linear_fused_bf16: ``linear`` (M > 8) with the fused epilogues of the UNet transformer blocks.
    ``stats_out`` fp32 [N/128, M, 2]: per-row partial (sum, sum of squares) of the output per 128-column slot.
    ``ln`` = (c fp32 [N], d fp32 [N], stats fp32 [K/128, M, 2], eps): x is the un-normalised activation, w = W * gamma.
    ``vt`` = (vt_out bf16 [B, N - col0, S_pad], col0, S): columns >= col0 are stored key-contiguous instead of row-major.
    ``cross`` = (k_rows bf16 [B * n, ldk], vt bf16 [B, N / 64, 64, n_pad], n, rows_per_batch, scale): x @ w^T is attn2.to_q and the
    output is the cross-attention over the n <= 64 cached keys (see emu_linear_fx)."""
    import ctypes as C
    from ._lib import LinearFxC
    _req(x, "x"); _req(w, "w")
    M, K = x.shape
    N = w.shape[0]
    n_out = N // 2 if epi in (EPI_SWIGLU, EPI_GEGLU) else N
    if out is None:
        out = torch.empty(M, n_out, device=x.device, dtype=BF16)
    fx = LinearFxC()
    if stats_out is not None:
        assert stats_out.dtype == torch.float32 and stats_out.is_contiguous() and stats_out.numel() == (N // 128) * M * 2
        fx.row_stats_out = stats_out.data_ptr()
    if ln is not None:
        c, d, stats, eps = ln
        assert c.dtype == d.dtype == stats.dtype == torch.float32 and c.numel() == d.numel() == N and stats.is_contiguous()
        fx.ln_c, fx.ln_d, fx.ln_stats, fx.ln_slots, fx.ln_eps = c.data_ptr(), d.data_ptr(), stats.data_ptr(), stats.shape[0], float(eps)
    if vt is not None:
        vt_out, col0, S = vt
        _req(vt_out, "vt_out")
        fx.vt_out, fx.vt_col0, fx.vt_s, fx.vt_spad = vt_out.data_ptr(), int(col0), int(S), vt_out.shape[-1]
    if cross is not None:
        ck, cvt, n_ctx, rows, scale = cross
        _req(ck, "cross_k"); _req(cvt, "cross_vt")
        fx.cross_k, fx.cross_vt, fx.cross_ldk, fx.cross_n = ck.data_ptr(), cvt.data_ptr(), ck.stride(0), int(n_ctx)
        fx.cross_npad, fx.cross_rows, fx.cross_scale = cvt.shape[-1], int(rows), float(scale)
    check(lib().emu_linear_fused_bf16(_p(x), _p(w), _p(bias), _p(res), _p(out), M, N, K, x.stride(0), w.stride(0),
                                      res.stride(0) if res is not None else 0, out.stride(0), int(epi), C.byref(fx), stream(x)),
          "emu_linear_fused_bf16")
    return out


def quantize_fp8_rows(w):
    """Per-row symmetric OCP e4m3fn quantisation of a packed bf16 weight [N, K]: returns (bytes uint8 [N, K], scale fp32
    [N]) with w ~= fp8(bytes) * scale[:, None]; see emu_quantize_fp8_rows."""
    _req(w, "w")
    assert w.dim() == 2 and w.stride(1) == 1
    N, K = w.shape
    q = torch.empty(N, K, device=w.device, dtype=torch.uint8)
    sc = torch.empty(N, device=w.device, dtype=torch.float32)
    check(lib().emu_quantize_fp8_rows(_p(w), w.stride(0), _p(q), q.stride(0), _p(sc), N, K, stream(w)),
          "emu_quantize_fp8_rows")
    return q, sc


def quantize_mxfp4_rows(w):
    """Round-to-nearest MXFP4 quantisation of a packed bf16 weight [N, K] (K % 32 == 0) on the device: returns (element bytes
    uint8 [N, K/2], E8M0 scales uint8 [N, K/32]), bit-exact with ``emu_amd.mxfp4.quantize_rows``; see emu_quantize_mxfp4_rows."""
    _req(w, "w")
    assert w.dim() == 2 and w.stride(1) == 1
    N, K = w.shape
    q = torch.empty(N, K // 2, device=w.device, dtype=torch.uint8)
    sc = torch.empty(N, K // 32, device=w.device, dtype=torch.uint8)
    check(lib().emu_quantize_mxfp4_rows(_p(w), w.stride(0), _p(q), q.stride(0), _p(sc), sc.stride(0), N, K, stream(w)),
          "emu_quantize_mxfp4_rows")
    return q, sc


FORM_HEAD, FORM_PRELOAD, FORM_RT = 1, 2, 3          # GemvForm of the bf16 plan (include/emu_hip.h: emu_gemv_geometry_query)


def pack_bf16_rows(w, rows: int):
    """The 13-bit lossless packing of a bf16 weight [N, K] (K % 32 == 0) on the device, for row groups of ``rows`` (2 or 4) rows:
    the dict of ``emu_amd.bf16pack.pack`` (planes and flags on the device), byte for byte; see emu_bf16_pack."""
    _req(w, "w")
    assert w.dim() == 2 and rows in (2, 4)
    N, K = w.shape
    G, KV = (N + rows - 1) // rows, K // 8
    u8 = dict(device=w.device, dtype=torch.uint8)
    p = {"lo": torch.empty(G, rows // 2, KV, 16, **u8), "nib": torch.empty(G, KV, rows, 4, **u8), "sign": torch.empty(G, KV, rows, **u8),
         "flags": torch.empty((G + 31) // 32, device=w.device, dtype=torch.int32), "rows": rows, "shape": (N, K)}
    hb = C.c_int(0)
    check(lib().emu_bf16_pack(_p(w), w.stride(0), N, K, rows, _p(p["lo"]), _p(p["nib"]), _p(p["sign"]), _p(p["flags"]), C.byref(hb),
                              stream(w)), "emu_bf16_pack")
    p["hb"] = int(hb.value)
    return p


def pack12_bf16_rows(w, rows: int):
    """The 12-bit lossless packing of a bf16 weight [N, K] (K % 32 == 0) on the device, for row groups of ``rows`` (2 or 4) rows: the
    dict of ``emu_amd.bf16pack.pack12`` (planes, patch records and flags on the device), byte for byte; see emu_bf16_pack12."""
    _req(w, "w")
    assert w.dim() == 2 and rows in (2, 4)
    N, K = w.shape
    G, KV = (N + rows - 1) // rows, K // 8
    u8 = dict(device=w.device, dtype=torch.uint8)
    i32 = dict(device=w.device, dtype=torch.int32)
    p = {"lo": torch.empty(G, rows // 2, KV, 16, **u8), "nib": torch.empty(G, KV, rows, 4, **u8), "patch": torch.empty(G, 8, **i32),
         "flags": torch.empty((G + 31) // 32, **i32), "rows": rows, "shape": (N, K), "bits": 12}
    hb, flagged = C.c_int(0), C.c_int(0)
    check(lib().emu_bf16_pack12(_p(w), w.stride(0), N, K, rows, _p(p["lo"]), _p(p["nib"]), _p(p["patch"]), _p(p["flags"]), C.byref(hb),
                                C.byref(flagged), stream(w)), "emu_bf16_pack12")
    p["hb"], p["flagged"] = int(hb.value), int(flagged.value)
    return p


def pack_set_c(p):
    """The emu_bf16_pack_set of a 13-bit packed dict (None, or a 12-bit dict: the empty set, rows 0)."""
    from ._lib import Bf16PackSetC
    if p is None or "patch" in p:
        return Bf16PackSetC(None, None, None, None, 0, 0)
    return Bf16PackSetC(_p(p["lo"]), _p(p["nib"]), _p(p["sign"]), _p(p["flags"]), p["hb"], p["rows"])


def pack12_set_c(p):
    """The emu_bf16_pack12_set of a 12-bit packed dict (None, or a 13-bit dict: the empty set, rows 0)."""
    from ._lib import Bf16Pack12SetC
    if p is None or "patch" not in p:
        return Bf16Pack12SetC(None, None, None, None, 0, 0)
    return Bf16Pack12SetC(_p(p["lo"]), _p(p["nib"]), _p(p["patch"]), _p(p["flags"]), p["hb"], p["rows"])


def linear_bf16pack(x, w, p, form: int, res=None, norm_w=None, eps: float = 0.0, epi: int = EPI_NONE, out=None):
    """One activation row over the packed set ``p`` of ``w`` in the given bf16 form (FORM_*); see emu_linear_bf16pack."""
    _req(x, "x"); _req(w, "w")
    assert x.dim() == 2 and x.shape[0] == 1 and w.is_contiguous() and tuple(w.shape) == tuple(p["shape"]) and x.shape[1] == w.shape[1]
    N, K = w.shape
    if out is None:
        out = torch.empty(1, N // 2 if epi == EPI_SWIGLU else N, device=x.device, dtype=BF16)
    if "patch" in p:                                 # a 12-bit set: its own entry point
        s = pack12_set_c(p)
        check(lib().emu_linear_bf16pack12(_p(x), _p(w), C.byref(s), _p(res), _p(norm_w), _p(out), N, K, form, eps, epi, stream(x)),
              "emu_linear_bf16pack12")
        return out
    s = pack_set_c(p)
    check(lib().emu_linear_bf16pack(_p(x), _p(w), C.byref(s), _p(res), _p(norm_w), _p(out), N, K, form, eps, epi, stream(x)),
          "emu_linear_bf16pack")
    return out


def linear_bf16pack_thin(x, w, p, res=None, epi: int = EPI_NONE, out=None):
    """4..16 activation rows over the packed set ``p`` of ``w`` on the matrix cores, the bits of ``linear(x, w)``; the library
    refuses (-22) what has no packed twin; see emu_linear_bf16pack_thin (a 12-bit set: emu_linear_bf16pack12_thin)."""
    _req(x, "x"); _req(w, "w")
    assert x.dim() == 2 and x.is_contiguous() and w.is_contiguous() and tuple(w.shape) == tuple(p["shape"]) and x.shape[1] == w.shape[1]
    M, (N, K) = x.shape[0], w.shape
    if out is None:
        out = torch.empty(M, N // 2 if epi == EPI_SWIGLU else N, device=x.device, dtype=BF16)
    _req(out, "out")
    assert out.is_contiguous() and (res is None or (res.is_contiguous() and tuple(res.shape) == (M, N)))
    if "patch" in p:                                 # a 12-bit set: its own entry point
        s = pack12_set_c(p)
        check(lib().emu_linear_bf16pack12_thin(_p(x), _p(w), C.byref(s), _p(res), _p(out), M, N, K, int(epi), stream(x)),
              "emu_linear_bf16pack12_thin")
        return out
    s = pack_set_c(p)
    check(lib().emu_linear_bf16pack_thin(_p(x), _p(w), C.byref(s), _p(res), _p(out), M, N, K, int(epi), stream(x)),
          "emu_linear_bf16pack_thin")
    return out


def linear_fp4w(x, w4, scales, bias=None, res=None, norm_w=None, eps: float = 0.0, epi: int = EPI_NONE, out=None):
    """``linear`` over an MXFP4 weight stream (decode rows only, M <= 2; K % 32 == 0); see emu_linear_fp4w_bf16."""
    _req(x, "x"); _req(w4, "w4", torch.uint8); _req(scales, "scales", torch.uint8)
    assert x.dim() == 2 and w4.dim() == 2 and scales.dim() == 2 and w4.shape[0] == scales.shape[0], (x.shape, w4.shape, scales.shape)
    assert w4.stride(1) == 1 and scales.stride(1) == 1
    M, K = x.shape
    N = w4.shape[0]
    if K % 32 == 0:                                # (any other K is the library's to refuse)
        assert w4.shape[1] == K // 2 and scales.shape[1] == K // 32, (x.shape, w4.shape, scales.shape)
    cols = N // 2 if epi == EPI_SWIGLU else N
    if out is None:
        out = torch.empty(M, cols, device=x.device, dtype=BF16)
    _req(out, "out")
    if res is not None:
        _req(res, "res")
    check(lib().emu_linear_fp4w_bf16(_p(x), _p(w4), _p(scales), _p(bias), _p(res), _p(norm_w), _p(out), M, N, K,
                                     x.stride(0), w4.stride(0), scales.stride(0), res.stride(0) if res is not None else 0,
                                     out.stride(0), float(eps), int(epi), stream(x)), "emu_linear_fp4w_bf16")
    return out


def _linear_fp4w_mfma(symbol, x, w4, scales, bias, res, epi, out):
    """The shared body of ``linear_fp4w_thin`` and ``linear_fp4w_gemm``: one argument list, ``symbol`` names the C entry point."""
    _req(x, "x"); _req(w4, "w4", torch.uint8); _req(scales, "scales", torch.uint8)
    assert x.dim() == 2 and w4.dim() == 2 and scales.dim() == 2 and w4.shape[0] == scales.shape[0], (x.shape, w4.shape, scales.shape)
    assert x.stride(1) == 1 and w4.stride(1) == 1 and scales.stride(1) == 1
    M, K = x.shape
    N = w4.shape[0]
    if K % 32 == 0:                                # (any other K is the library's to refuse)
        assert w4.shape[1] == K // 2 and scales.shape[1] == K // 32, (x.shape, w4.shape, scales.shape)
    cols = N // 2 if epi == EPI_SWIGLU else N
    if out is None:
        out = torch.empty(M, cols, device=x.device, dtype=BF16)
    _req(out, "out")
    if bias is not None:
        _req(bias, "bias")
    if res is not None:
        _req(res, "res")
    check(getattr(lib(), symbol)(_p(x), _p(w4), _p(scales), _p(bias), _p(res), _p(out), M, N, K, x.stride(0), w4.stride(0),
                                 scales.stride(0), res.stride(0) if res is not None else 0, out.stride(0), int(epi), stream(x)), symbol)
    return out


def linear_fp4w_thin(x, w4, scales, bias=None, res=None, epi: int = EPI_NONE, out=None):
    """``linear`` over an MXFP4 weight stream for 1..16 rows on the matrix cores (K % 256 == 0, no fused norm; epi NONE / RESID /
    SWIGLU); see emu_linear_fp4w_thin_bf16.  Any other K % 32 == 0 from 256 up: ``linear_fp4w_mfma``."""
    return _linear_fp4w_mfma("emu_linear_fp4w_thin_bf16", x, w4, scales, bias, res, epi, out)


def linear_fp4w_gemm(x, w4, scales, bias=None, res=None, epi: int = EPI_NONE, out=None):
    """``linear`` over MXFP4 weights for 17 rows and more (K % 256 == 0, no fused norm; epi NONE / RESID / SWIGLU): the 4-bit GEMM,
    same arithmetic and rounding points as ``linear_fp4w_thin``; see emu_linear_fp4w_gemm_bf16.  Any other K % 32 == 0 from 256 up:
    ``linear_fp4w_mfma``."""
    return _linear_fp4w_mfma("emu_linear_fp4w_gemm_bf16", x, w4, scales, bias, res, epi, out)


def linear_fp4w_mfma(x, w4, scales, bias=None, res=None, epi: int = EPI_NONE, out=None):
    """``linear`` over MXFP4 weights on the matrix cores for any row count and any K >= 256 with K % 32 == 0 (no fused norm; epi NONE
    / RESID / SWIGLU): ``linear_fp4w_thin``'s kernel up to 16 rows, ``linear_fp4w_gemm``'s above, the same tiles, a K that is no
    multiple of 256 ending in a partial stage.  ``scales`` is [N, K/32] (padded here: ``mxfp4.pad_scales``) or already a view
    [N, K/32] / [N, mxfp4.scale_stride(K)] whose row stride is a multiple of 4 and at least ``mxfp4.scale_stride(K)``; see
    emu_linear_fp4w_mfma_bf16."""
    K = x.shape[1]
    if K >= 32 and K % 32 == 0 and scales.dim() == 2:      # (any other K is the library's to refuse)
        stride = mxfp4.scale_stride(K)
        if scales.shape[1] == K // 32 and scales.stride(0) < stride:
            scales = mxfp4.pad_scales(scales.contiguous(), K)
        if scales.shape[1] == stride:
            scales = scales[:, :K // 32]
    return _linear_fp4w_mfma("emu_linear_fp4w_mfma_bf16", x, w4, scales, bias, res, epi, out)


def linear_fp8(x8, xscale, w8, wscale, bias=None, res=None, epi: int = EPI_NONE, out=None):
    """fp8 x fp8 GEMM (both operands from ``quantize_fp8_rows``) -> bf16; see emu_linear_fp8_bf16."""
    _req(x8, "x8", torch.uint8); _req(w8, "w8", torch.uint8)
    _req(xscale, "xscale", torch.float32); _req(wscale, "wscale", torch.float32)
    assert x8.dim() == 2 and w8.dim() == 2 and x8.shape[1] == w8.shape[1], (x8.shape, w8.shape)
    M, K = x8.shape
    N = w8.shape[0]
    n_out = N // 2 if epi in (EPI_SWIGLU, EPI_GEGLU) else N
    if out is None:
        out = torch.empty(M, n_out, device=x8.device, dtype=BF16)
    _req(out, "out")
    if res is not None:
        _req(res, "res")
    check(lib().emu_linear_fp8_bf16(_p(x8), _p(xscale), _p(w8), _p(wscale), _p(bias), _p(res), _p(out), M, N, K, x8.stride(0),
                                    w8.stride(0), res.stride(0) if res is not None else 0, out.stride(0), int(epi), stream(x8)),
          "emu_linear_fp8_bf16")
    return out


def linear_fp8w(x, w8, wscale, bias=None, res=None, norm_w=None, eps: float = 0.0, epi: int = EPI_NONE, out=None):
    """``linear`` over an fp8 weight stream (decode rows only, M <= 2); see emu_linear_fp8w_bf16."""
    _req(x, "x"); _req(w8, "w8", torch.uint8); _req(wscale, "wscale", torch.float32)
    assert x.dim() == 2 and w8.dim() == 2 and x.shape[1] == w8.shape[1], (x.shape, w8.shape)
    M, K = x.shape
    N = w8.shape[0]
    n_out = N // 2 if epi == EPI_SWIGLU else N
    if out is None:
        out = torch.empty(M, n_out, device=x.device, dtype=BF16)
    _req(out, "out")
    if res is not None:
        _req(res, "res")
    check(lib().emu_linear_fp8w_bf16(_p(x), _p(w8), _p(wscale), _p(bias), _p(res), _p(norm_w), _p(out), M, N, K,
                                     x.stride(0), w8.stride(0), res.stride(0) if res is not None else 0,
                                     out.stride(0), float(eps), int(epi), stream(x)), "emu_linear_fp8w_bf16")
    return out


def _linear_fp8w_mfma(fn, symbol, lo, hi, beyond, x, w8, wscale, bias, res, epi, out):
    """The three W8A16 matrix-core entry points (``fn``: the wrapper's name, ``symbol``: its C function) differ in their row range
    ``lo..hi`` alone (``hi`` None: no upper end); ``beyond``: where a caller with other row counts should go.  Every argument is checked before any device work."""
    for name, t, dt in (("x", x, BF16), ("w8", w8, torch.uint8), ("wscale", wscale, torch.float32), ("bias", bias, BF16),
                        ("res", res, BF16), ("out", out, BF16)):
        if t is None and name in ("bias", "res", "out"):
            continue
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{fn}: {name} must be a tensor, got {type(t).__name__}")
        if t.dtype != dt or t.dim() < 1 or t.stride(-1) != 1:
            raise ValueError(f"{fn}: {name} must be {dt} and contiguous in its last dimension, got {t.dtype} "
                             f"{tuple(t.shape)} with strides {t.stride()}")
    if x.dim() != 2 or w8.dim() != 2 or x.shape[1] != w8.shape[1]:
        raise ValueError(f"{fn}: x [M, K] and w8 [N, K] must agree in K, got {tuple(x.shape)} and {tuple(w8.shape)}")
    M, K = x.shape
    N = w8.shape[0]
    if hi is None and M < lo:
        raise ValueError(f"{fn}: {lo} rows and more, got M = {M} ({beyond})")
    if hi is not None and not lo <= M <= hi:
        raise ValueError(f"{fn}: {lo}..{hi} rows, got M = {M} ({beyond})")
    if (N + 63) // 64 > 65535 and hi is None:
        raise ValueError(f"{fn}: at most 65535 column tiles of 64 weight rows, got N = {N}")
    if N < 1 or K < 256 or K % 256:
        raise ValueError(f"{fn}: N >= 1 and K a multiple of 256, at least 256; got N = {N}, K = {K}")
    if epi not in (EPI_NONE, EPI_RESID, EPI_SWIGLU):
        raise ValueError(f"{fn}: epi must be EPI_NONE, EPI_RESID or EPI_SWIGLU, got {epi}")
    if epi == EPI_SWIGLU and N % 2:
        raise ValueError(f"{fn}: EPI_SWIGLU needs an even N (interleaved gate / up rows), got {N}")
    if wscale.dim() != 1 or wscale.numel() != N:
        raise ValueError(f"{fn}: wscale must be fp32 [{N}], got {tuple(wscale.shape)}")
    if w8.stride(0) % 16 or w8.stride(0) < K or w8.data_ptr() % 16:
        raise ValueError(f"{fn}: w8 rows must start on 16-byte boundaries (row stride {w8.stride(0)} bytes, "
                         f"offset {w8.data_ptr() % 16})")
    if x.stride(0) % 8 or x.stride(0) < K or x.data_ptr() % 16:
        raise ValueError(f"{fn}: x rows must start on 16-byte boundaries (row stride {x.stride(0)} elements, "
                         f"offset {x.data_ptr() % 16} bytes)")
    cols = N // 2 if epi == EPI_SWIGLU else N
    if bias is not None and bias.numel() != N:
        raise ValueError(f"{fn}: bias must be bf16 [{N}], got {tuple(bias.shape)}")
    if epi == EPI_RESID and (res is None or tuple(res.shape) != (M, N)):
        raise ValueError(f"{fn}: EPI_RESID needs res bf16 [{M}, {N}]")
    if out is None:
        out = torch.empty(M, cols, device=x.device, dtype=BF16)
    elif tuple(out.shape) != (M, cols):
        raise ValueError(f"{fn}: out must be bf16 [{M}, {cols}], got {tuple(out.shape)}")
    for name, t in (("x", x), ("w8", w8), ("wscale", wscale), ("bias", bias), ("res", res), ("out", out)):
        if t is not None and (not t.is_cuda or t.device != x.device):
            raise ValueError(f"{fn}: {name} must be a GPU tensor on x's device (emu_amd has no CPU path)")
    check(getattr(lib(), symbol)(_p(x), _p(w8), _p(wscale), _p(bias), _p(res), _p(out), M, N, K, x.stride(0), w8.stride(0),
                                 res.stride(0) if res is not None else 0, out.stride(0), int(epi), stream(x)), symbol)
    return out


def linear_fp8w_thin(x, w8, wscale, bias=None, res=None, epi: int = EPI_NONE, out=None):
    """``linear`` over an fp8 weight stream (``quantize_fp8_rows``' bytes and row scales) for 1..16 rows on the matrix cores: K >= 256
    and K % 256 == 0, no fused norm, epi NONE / RESID / SWIGLU; see emu_linear_fp8w_thin_bf16.  Every argument is checked here, before
    any device work: a ``ValueError`` says what is wrong, nothing falls back to another kernel."""
    return _linear_fp8w_mfma("linear_fp8w_thin", "emu_linear_fp8w_thin_bf16", 1, 16, "17 rows and more: the W8A8 GEMM, linear_fp8",
                             x, w8, wscale, bias, res, epi, out)


def linear_fp8w_gemm(x, w8, wscale, bias=None, res=None, epi: int = EPI_NONE, out=None):
    """The same product for 17..64 rows (beams x batch): the W8A16 GEMM of csrc/gemm_fp8.hip, same arguments, requirements, epilogues
    and rounding points as ``linear_fp8w_thin``; see emu_linear_fp8w_gemm_bf16.  Every argument is checked here, before any device
    work: a ``ValueError`` says what is wrong, nothing falls back to another kernel."""
    return _linear_fp8w_mfma("linear_fp8w_gemm", "emu_linear_fp8w_gemm_bf16", 17, 64,
                             "up to 16 rows: linear_fp8w_thin; 65 and more: linear, or the W8A8 GEMM linear_fp8",
                             x, w8, wscale, bias, res, epi, out)


def linear_fp8w_tile(x, w8, wscale, bias=None, res=None, epi: int = EPI_NONE, out=None):
    """The same product for 65 rows and more (prompts, scoring prefills, beams x batch): the 64 x 128 form of csrc/gemm_fp8.hip's
    kernel, same arguments, requirements, epilogues and rounding points as ``linear_fp8w_gemm``, whose results it repeats bit for bit
    row by row; see emu_linear_fp8w_tile_bf16.  Every argument is checked here, before any device work: a ``ValueError`` says what is
    wrong, nothing falls back to another kernel."""
    return _linear_fp8w_mfma("linear_fp8w_tile", "emu_linear_fp8w_tile_bf16", 65, None,
                             "up to 16 rows: linear_fp8w_thin; 17..64: linear_fp8w_gemm", x, w8, wscale, bias, res, epi, out)


def rmsnorm(x, w, eps: float, out=None):
    _req(x, "x"); _req(w, "w")
    rows, cols = x.shape
    if out is None:
        out = torch.empty_like(x)
    check(lib().emu_rmsnorm_bf16(_p(x), _p(w), _p(out), rows, cols, x.stride(0), out.stride(0), float(eps), stream(x)),
          "emu_rmsnorm_bf16")
    return out


def layernorm(x, w, b, eps: float, res=None, out=None):
    _req(x, "x")
    assert x.is_contiguous()
    rows, cols = x.shape
    if out is None:
        out = torch.empty_like(x)
    check(lib().emu_layernorm_bf16(_p(x), _p(w), _p(b), _p(res), _p(out), rows, cols, float(eps), stream(x)),
          "emu_layernorm_bf16")
    return out


def layernorm_q8(x, w, b, eps: float, res=None, want_y: bool = True):
    """``layernorm`` + per-row e4m3 quantisation of its bf16 result in one launch (see emu_layernorm_q8_bf16):
    returns (y or None, bytes uint8 [rows, cols], scale fp32 [rows])."""
    _req(x, "x")
    assert x.is_contiguous()
    rows, cols = x.shape
    y = torch.empty_like(x) if want_y else None
    q = torch.empty(rows, cols, device=x.device, dtype=torch.uint8)
    sc = torch.empty(rows, device=x.device, dtype=torch.float32)
    check(lib().emu_layernorm_q8_bf16(_p(x), _p(w), _p(b), _p(res), _p(y), _p(q), _p(sc), rows, cols, float(eps), stream(x)),
          "emu_layernorm_q8_bf16")
    return y, q, sc


def embed_gather(ids, table, out=None):
    _req(ids, "ids", torch.int32); _req(table, "table")
    n = ids.numel()
    if out is None:
        out = torch.empty(n, table.shape[1], device=table.device, dtype=BF16)
    check(lib().emu_embed_gather_bf16(_p(ids), _p(table), _p(out), n, table.shape[1], table.shape[0], stream(table)),
          "emu_embed_gather_bf16")
    return out


def scatter_rows(src, dst_rows, out):
    _req(src, "src"); _req(dst_rows, "dst_rows", torch.int32); _req(out, "out")
    assert src.is_contiguous() and out.is_contiguous() and src.shape[0] == dst_rows.numel()
    check(lib().emu_scatter_rows_bf16(_p(src), _p(dst_rows), _p(out), src.shape[0], src.shape[1], stream(src)),
          "emu_scatter_rows_bf16")
    return out


def argmax(logits, vocab: Optional[int] = None, suppress_id: int = -1, out=None):
    _req(logits, "logits")
    rows = logits.shape[0]
    vocab = logits.shape[1] if vocab is None else vocab
    if out is None:
        out = torch.empty(rows, device=logits.device, dtype=torch.int32)
    check(lib().emu_argmax_bf16(_p(logits), logits.stride(0), rows, vocab, suppress_id, _p(out), stream(logits)),
          "emu_argmax_bf16")
    return out


def trie_tables(tables):
    """``_lib.TokenTrieC`` (include/emu_hip.h: emu_token_trie) over ``tables`` = (first, tok, child), int32 on the device
    (``emu_amd.constrain.TokenTrie.tables``).  The struct holds addresses only: the caller keeps ``tables`` alive."""
    first, tok, child = tables
    for name, t in (("first", first), ("tok", tok), ("child", child)):
        _req(t, name, torch.int32)
    if first.numel() < 2 or tok.numel() != child.numel():
        raise ValueError("trie tables: first [nodes + 1], tok [edges], child [edges]")
    return TokenTrieC(_p(first), _p(tok), _p(child), first.numel() - 1, tok.numel())


# The selection kernels' entry points: (step kind, selection variant) -> C symbol.  A variant is its kind's plain entry point with its
# own arguments ahead of the stream: "trie" the constraint's tables (``trie_tables``) and the rows' nodes (int32, in/out), "ngram" the
# size of the no-repeat n-gram ban.  The beam sampler step has no "trie" variant.
SELECT_ENTRY = {
    ("sample", "plain"): "emu_sample_bf16", ("sample", "trie"): "emu_sample_trie_bf16", ("sample", "ngram"): "emu_sample_ngram_bf16",
    ("sample_step", "plain"): "emu_llama_sample_step", ("sample_step", "trie"): "emu_llama_sample_step_trie",
    ("sample_step", "ngram"): "emu_llama_sample_step_ngram",
    ("beam_step", "plain"): "emu_beam_step_bf16", ("beam_step", "trie"): "emu_beam_step_trie_bf16",
    ("beam_step", "ngram"): "emu_beam_step_ngram_bf16",
    ("beam_sample_step", "plain"): "emu_beam_sample_step_bf16", ("beam_sample_step", "ngram"): "emu_beam_sample_step_ngram_bf16",
}


def select_call(library, kind: str, variant: str, args: tuple, stream_ptr, ctx=None, trie=None, node=None, ngram: int = 0) -> None:
    """Call the ``SELECT_ENTRY`` of (``kind``, ``variant``) in ``library`` (the caller's ``lib()``) with the kind's common ``args``,
    then the variant's own, then the stream; a failure is reported under the symbol's name (``ctx``: as ``check``'s)."""
    name = SELECT_ENTRY[kind, variant]
    own = (C.byref(trie), _p(node)) if variant == "trie" else (int(ngram),) if variant == "ngram" else ()
    check(getattr(library, name)(*args, *own, stream_ptr), name, ctx)


def sample(logits, step_dev, params, out=None, vocab: Optional[int] = None, hist=None, uniforms=None, unfinished=None,
           probs_out=None, trie=None, node=None, ngram: Optional[int] = None):
    """``emu_sample_bf16`` (include/emu_hip.h; specified in emu_amd/sampling.py): one token per row of bf16 ``logits`` [rows, >= vocab]
    under ``params`` (``_lib.SampleParamsC``).  ``step_dev`` int32 [1] on the device = the step index the kernel reads: the number of
    history rows of ``hist`` int32 [steps, rows] in use, the row of ``uniforms`` fp32 [steps, rows], the min-length comparison.
    ``unfinished`` int32 [rows] and ``probs_out`` fp32 [rows, >= vocab] are optional.  ``trie`` (``trie_tables``) with ``node``
    int32 [rows], in/out: the "trie" variant (``SELECT_ENTRY``), the selection under a constraint.  ``ngram`` (not None): the "ngram"
    variant, the no-repeat n-gram ban of that size over ``hist`` (0 = off; not built together with a trie).  Returns ``out`` int32
    [rows]."""
    _req(logits, "logits")
    rows = logits.shape[0]
    vocab = logits.shape[1] if vocab is None else vocab
    if out is None:
        out = torch.empty(rows, device=logits.device, dtype=torch.int32)
    for name, t, dt in (("step_dev", step_dev, torch.int32), ("hist", hist, torch.int32), ("uniforms", uniforms, torch.float32),
                        ("unfinished", unfinished, torch.int32), ("probs_out", probs_out, torch.float32), ("out", out, torch.int32),
                        ("node", node, torch.int32)):
        if t is not None:
            _req(t, name, dt)
    args = (_p(logits), logits.stride(0), rows, vocab, _p(hist), hist.stride(0) if hist is not None else 0,
            hist.shape[0] if hist is not None else 0, _p(step_dev), _p(uniforms),
            uniforms.stride(0) if uniforms is not None else 0, uniforms.shape[0] if uniforms is not None else 0,
            C.byref(params), _p(unfinished), _p(out), _p(probs_out), probs_out.stride(0) if probs_out is not None else 0)
    constrained = trie is not None or node is not None
    if ngram is not None and constrained:
        raise ValueError("the n-gram ban together with a constraint is not built on the device")
    if constrained and (trie is None or node is None or node.numel() < rows):
        raise ValueError("a constrained selection needs the trie's tables and a node per row")
    variant = "ngram" if ngram is not None else "trie" if constrained else "plain"
    select_call(lib(), "sample", variant, args, stream(logits), trie=trie, node=node, ngram=ngram or 0)
    return out


def token_logprob(logits, targets, ref_logits=None, vocab: Optional[int] = None, step_dev=None, out=None):
    """``emu_token_logprob_bf16`` (include/emu_hip.h; specified in emu_amd/scoring.py): the log-probability of the forced target of
    every row of bf16 ``logits`` [rows, >= vocab].  ``targets`` int32 [rows] -- or [steps, rows] with ``step_dev`` int32 [1] on the
    device naming the row of it (and of every output) in use.  ``ref_logits`` [rows, >= vocab] bf16 adds ``kl`` and ``agree``.
    Returns a dict of ``lp`` / ``lse`` fp32, ``top1`` int32 (and ``kl`` fp32, ``agree`` int32), shaped like ``targets``; ``out`` may
    hand in such a dict to be written into."""
    def flat(t, name, dtype):        # (is_contiguous, not _req's stride test: a one-element dimension may carry any stride)
        if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dtype} GPU tensor")

    _req(logits, "logits"); flat(targets, "targets", torch.int32)
    rows = logits.shape[0]
    vocab = logits.shape[1] if vocab is None else vocab
    if targets.shape[-1] != rows or (targets.dim() != 1 and step_dev is None):
        raise ValueError(f"targets must be contiguous int32 [{rows}], or [steps, {rows}] with step_dev; got {tuple(targets.shape)}")
    if ref_logits is not None:
        _req(ref_logits, "ref_logits")
        if ref_logits.shape[0] != rows or ref_logits.shape[1] < vocab:
            raise ValueError(f"ref_logits must be [{rows}, >= {vocab}], got {tuple(ref_logits.shape)}")
    if step_dev is not None:
        flat(step_dev, "step_dev", torch.int32)
    if out is None:
        out = {"lp": torch.empty(targets.shape, device=logits.device, dtype=torch.float32),
               "lse": torch.empty(targets.shape, device=logits.device, dtype=torch.float32),
               "top1": torch.empty(targets.shape, device=logits.device, dtype=torch.int32)}
        if ref_logits is not None:
            out["kl"] = torch.empty(targets.shape, device=logits.device, dtype=torch.float32)
            out["agree"] = torch.empty(targets.shape, device=logits.device, dtype=torch.int32)
    for name, dt in (("lp", torch.float32), ("lse", torch.float32), ("top1", torch.int32), ("kl", torch.float32), ("agree", torch.int32)):
        if out.get(name) is not None:
            flat(out[name], f"out[{name!r}]", dt)
            if out[name].shape != targets.shape:
                raise ValueError(f"out[{name!r}] must be shaped like targets")
    check(lib().emu_token_logprob_bf16(_p(logits), logits.stride(0), rows, vocab, _p(targets), rows, _p(step_dev), _p(ref_logits),
                                       ref_logits.stride(0) if ref_logits is not None else 0, _p(out.get("lp")), _p(out.get("lse")),
                                       _p(out.get("top1")), _p(out.get("kl")), _p(out.get("agree")), rows, stream(logits)),
          "emu_token_logprob_bf16")
    return out


def avgpool_tokens(x, grid: int, stride: int):
    """x [B, 1+grid*grid, C] -> [B, (grid/stride)^2, C] (cls dropped)."""
    _req(x, "x")
    assert x.is_contiguous()
    B, _, Cc = x.shape
    go = grid // stride
    out = torch.empty(B, go * go, Cc, device=x.device, dtype=BF16)
    check(lib().emu_avgpool_tokens_bf16(_p(x), _p(out), B, grid, Cc, stride, stream(x)), "emu_avgpool_tokens_bf16")
    return out


def rope_kv_append(qkv, cos, sin, pos, slot, kcache, vcache, B: int, T: int, H: int, D: int):
    _req(qkv, "qkv"); _req(kcache, "kcache"); _req(vcache, "vcache")
    _req(pos, "pos", torch.int32); _req(slot, "slot", torch.int32)
    assert qkv.is_contiguous() and kcache.is_contiguous() and vcache.is_contiguous()
    S_max = kcache.shape[-2]
    check(lib().emu_rope_kv_append_bf16(_p(qkv), _p(cos), _p(sin), _p(pos), _p(slot), _p(kcache), _p(vcache),
                                        B, T, H, D, S_max, stream(qkv)), "emu_rope_kv_append_bf16")


def transpose_v(v, B: int, H: int, S: int, D: int, sb: int, sh: int, ss: int, S_pad: Optional[int] = None):
    _req(v, "v")
    S_pad = (S + 63) // 64 * 64 if S_pad is None else S_pad
    vt = torch.empty(B, H, D, S_pad, device=v.device, dtype=BF16)
    check(lib().emu_transpose_v_bf16(_p(v), sb, sh, ss, _p(vt), B, H, S, D, S_pad, stream(v)), "emu_transpose_v_bf16")
    return vt


def flash_attn(q, k, v, causal: bool, scale: float, kstart=None, out=None, vt=None):
    """q [B,Sq,H,D], k/v [B,Sk,H,D] (any strides with D contiguous) -> o [B,Sq,H,D] (``out`` if given: any strides that are multiples
    of 4 with D contiguous).  ``vt``: the caller's V^T [B,H,D,Sk_pad] (``transpose_v``: zero in [Sk, ceil64(Sk))) instead of ``v``."""
    _req(q, "q"); _req(k, "k")
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    if vt is None:
        _req(v, "v")
        vt = transpose_v(v, B, H, Sk, D, v.stride(0), v.stride(2), v.stride(1))
    else:
        _req(vt, "vt")
        assert v is None and vt.is_contiguous() and vt.shape[:3] == (B, H, D), (vt.shape, vt.stride())
    if out is None:
        o = torch.empty(B, Sq, H, D, device=q.device, dtype=BF16)
    else:
        _req(out, "out")
        assert out.shape == (B, Sq, H, D) and out.stride(3) == 1, (out.shape, out.stride())
        o = out
    check(lib().emu_flash_attn_bf16(_p(q), q.stride(0), q.stride(2), q.stride(1),
                                    _p(k), k.stride(0), k.stride(2), k.stride(1), _p(vt),
                                    _p(o), o.stride(0), o.stride(2), o.stride(1), _p(kstart),
                                    B, H, Sq, Sk, vt.shape[-1], D, int(causal), float(scale), stream(q)),
          "emu_flash_attn_bf16")
    return o


def flash_attn_prefix(q, kp, vp, ko, vo, kstart: int, scale: float, out=None):
    """Two-segment flash attention (emu_flash_attn_prefix_bf16; the specification is ``scoring.two_segment_attention``): q [B,Sq,H,D],
    the shared prefix kp / vp [P,H,D] of which keys [kstart, P) count, own keys ko / vo [B,Sk,H,D] (any strides with D contiguous),
    query i sees own keys j <= i + (Sk - Sq) -> o [B,Sq,H,D] (``out`` if given)."""
    _req(q, "q"); _req(kp, "kp"); _req(vp, "vp"); _req(ko, "ko"); _req(vo, "vo")
    B, Sq, H, D = q.shape
    P, Sk = kp.shape[0], ko.shape[1]
    o = torch.empty(B, Sq, H, D, device=q.device, dtype=BF16) if out is None else out
    vtp = transpose_v(vp, 1, H, P, D, 0, vp.stride(1), vp.stride(0))
    vto = transpose_v(vo, B, H, Sk, D, vo.stride(0), vo.stride(2), vo.stride(1))
    check(lib().emu_flash_attn_prefix_bf16(_p(q), q.stride(0), q.stride(2), q.stride(1), _p(kp), kp.stride(1), kp.stride(0), _p(vtp),
                                           _p(ko), ko.stride(0), ko.stride(2), ko.stride(1), _p(vto),
                                           _p(o), o.stride(0), o.stride(2), o.stride(1), int(kstart),
                                           B, H, Sq, P, vtp.shape[-1], Sk, vto.shape[-1], D, float(scale), stream(q)),
          "emu_flash_attn_prefix_bf16")
    return o


def decode_attn(q, kcache, vcache, ctx: int, scale: float, kstart=None, ctx_dev=None, ctx_max: int = 0):
    """q [B,H,D]; caches [B,H,S_max,D] -> o [B,H,D]."""
    _req(q, "q"); _req(kcache, "kcache"); _req(vcache, "vcache")
    B, H, D = q.shape
    S_max = kcache.shape[-2]
    ws = torch.empty(lib().emu_decode_attn_ws_bytes(B, H, D, max(ctx, ctx_max)) // 4, device=q.device,
                     dtype=torch.float32)
    o = torch.empty(B, H, D, device=q.device, dtype=BF16)
    check(lib().emu_decode_attn_bf16(_p(q), q.stride(0), q.stride(1), _p(kcache), _p(vcache), _p(o), o.stride(0),
                                     o.stride(1), _p(kstart), _p(ctx_dev), ctx, ctx_max, _p(ws), B, H, D, S_max,
                                     float(scale), stream(q)), "emu_decode_attn_bf16")
    return o


def decode_fused(qkv, cos, sin, pos, slot, kcache, vcache, H: int, ctx_max: int, scale: float, kstart=None, ws=None,
                 share_nb: int = 0, share_len: int = 0, arrive=None):
    """The decode step's attention launch (emu_decode_fused_bf16): qkv [B, 3*H*D] (q | k | v, not rotated); caches
    [B,H,S_max,D], the new token's rotated key and its value are appended at slot[b] -> o [B,H,D].  ``ws``: the fp32 split-state
    workspace (emu_decode_fused_ws_bytes), allocated here unless the caller brings one; ``arrive``: B*H zeroed int32 counters."""
    _req(qkv, "qkv"); _req(cos, "cos"); _req(sin, "sin"); _req(kcache, "kcache"); _req(vcache, "vcache")
    _req(pos, "pos", torch.int32); _req(slot, "slot", torch.int32)
    assert qkv.is_contiguous() and kcache.is_contiguous() and vcache.is_contiguous() and kcache.shape == vcache.shape
    B, _, S_max, D = kcache.shape
    assert qkv.shape == (B, 3 * H * D) and kcache.shape[1] == H, (qkv.shape, kcache.shape)
    need = lib().emu_decode_fused_ws_bytes(B, H, D, ctx_max) // 4
    if ws is None:
        ws = torch.empty(need, device=qkv.device, dtype=torch.float32)
    _req(ws, "ws", torch.float32)
    assert ws.is_contiguous() and ws.numel() >= need, (ws.numel(), need)
    if kstart is not None:
        _req(kstart, "kstart", torch.int32)
    if arrive is not None:
        _req(arrive, "arrive", torch.int32)
        assert arrive.is_contiguous() and arrive.numel() >= B * H
    o = torch.empty(B, H, D, device=qkv.device, dtype=BF16)
    check(lib().emu_decode_fused_bf16(_p(qkv), _p(cos), _p(sin), _p(pos), _p(slot), _p(kcache), _p(vcache), _p(o), o.stride(0),
                                      o.stride(1), _p(kstart), _p(ws), B, H, D, S_max, ctx_max, float(scale), share_nb,
                                      share_len, _p(arrive), stream(qkv)), "emu_decode_fused_bf16")
    return o


def decode_chunk(qkv, cos, sin, pos0, slot0, kcache, vcache, H: int, T: int, ctx_max: int, scale: float, kstart=None, ws=None):
    """The chunk step's attention launch (emu_decode_chunk_bf16): qkv [B*T, 3*H*D] (not rotated), T rows per sequence at the
    consecutive cache slots slot0[b] + i and positions pos0[b] + i (``pos0`` / ``slot0`` int32 [B]); the T rotated keys and values
    are appended -> o [B*T, H, D].  ``ws``: the fp32 workspace (emu_decode_chunk_ws_bytes), allocated here unless brought."""
    _req(qkv, "qkv"); _req(cos, "cos"); _req(sin, "sin"); _req(kcache, "kcache"); _req(vcache, "vcache")
    _req(pos0, "pos0", torch.int32); _req(slot0, "slot0", torch.int32)
    assert qkv.is_contiguous() and kcache.is_contiguous() and vcache.is_contiguous() and kcache.shape == vcache.shape
    B, _, S_max, D = kcache.shape
    assert qkv.shape == (B * T, 3 * H * D) and kcache.shape[1] == H, (qkv.shape, kcache.shape)
    assert pos0.numel() == B and slot0.numel() == B
    need = lib().emu_decode_chunk_ws_bytes(B, T, H, D, ctx_max) // 4
    if ws is None:
        ws = torch.empty(max(need, 1), device=qkv.device, dtype=torch.float32)
    _req(ws, "ws", torch.float32)
    assert ws.is_contiguous() and ws.numel() >= need, (ws.numel(), need)
    if kstart is not None:
        _req(kstart, "kstart", torch.int32)
    o = torch.empty(B * T, H, D, device=qkv.device, dtype=BF16)
    check(lib().emu_decode_chunk_bf16(_p(qkv), _p(cos), _p(sin), _p(pos0), _p(slot0), _p(kcache), _p(vcache), _p(o), o.stride(0),
                                      o.stride(1), _p(kstart), _p(ws), B, T, H, D, S_max, ctx_max, float(scale), stream(qkv)),
          "emu_decode_chunk_bf16")
    return o


LOOKUP_STATE_INTS = 8          # st of emu_lookup_select_bf16: step, finished, n_draft, hist_len, steps_run, tokens_emitted, -, -


def lookup_select(logits, cur, st, pos0, slot0, ctx, out_ids, hist, max_ngram: int, max_new: int, min_len: int, eos_id: int,
                  stop_on_eos: bool = True, drafts=None, amax=None):
    """The selection behind a chunk step (emu_lookup_select_bf16; ``emu_amd/speculate.py``): logits [T, V] bf16; every other
    tensor int32 on the device and updated in place.  Returns the rows' arg-maxes [T]."""
    _req(logits, "logits")
    T, V = logits.shape
    for name, t in (("cur", cur), ("st", st), ("pos0", pos0), ("slot0", slot0), ("ctx", ctx), ("out_ids", out_ids), ("hist", hist)):
        _req(t, name, torch.int32)
        assert t.is_contiguous(), name
    assert cur.numel() == T and st.numel() >= LOOKUP_STATE_INTS and out_ids.numel() >= max_new and logits.stride(1) == 1
    if drafts is not None:
        _req(drafts, "drafts", torch.int32)
        assert drafts.is_contiguous() and tuple(drafts.shape) == (max_new, T - 1), (drafts.shape, max_new, T)
    if amax is None:
        amax = torch.empty(T, device=logits.device, dtype=torch.int32)
    check(lib().emu_lookup_select_bf16(_p(logits), logits.stride(0), V, T, _p(amax), _p(cur), _p(st), _p(pos0), _p(slot0), _p(ctx),
                                       _p(out_ids), _p(hist), hist.numel(), _p(drafts), int(max_ngram), int(max_new), int(min_len),
                                       int(eos_id), int(bool(stop_on_eos)), stream(logits)), "emu_lookup_select_bf16")
    return amax


def lookup_sample(logits, cur, st, pos0, slot0, ctx, out_ids, hist, max_ngram: int, max_new: int, min_len: int, eos_id: int, params,
                  uniforms=None, stop_on_eos: bool = True, drafts=None, amax=None):
    """``lookup_select`` with the sampler's selection in the place of the arg-maxes (emu_lookup_sample_bf16;
    ``emu_amd/speculate.py``: ``row_select``): row i <= n_draft picks its id as ``sample`` picks output index step + i, with the
    history ``out_ids[:step]`` + ``cur[1:1 + i]`` and ``uniforms[min(step + i, rows - 1)]`` (fp32 [rows] or [rows, 1]; None without
    ``do_sample``).  ``params``: ``_lib.SampleParamsC``.  Returns the picked ids [T]; the entries behind the draft are not written."""
    _req(logits, "logits")
    T, V = logits.shape
    for name, t in (("cur", cur), ("st", st), ("pos0", pos0), ("slot0", slot0), ("ctx", ctx), ("out_ids", out_ids), ("hist", hist)):
        _req(t, name, torch.int32)
        assert t.is_contiguous(), name
    assert cur.numel() == T and st.numel() >= LOOKUP_STATE_INTS and out_ids.numel() >= max_new and logits.stride(1) == 1
    if drafts is not None:
        _req(drafts, "drafts", torch.int32)
        assert drafts.is_contiguous() and tuple(drafts.shape) == (max_new, T - 1), (drafts.shape, max_new, T)
    if uniforms is not None:
        _req(uniforms, "uniforms", torch.float32)
        assert uniforms.is_contiguous() and uniforms.numel() >= 1 and uniforms.numel() == uniforms.shape[0]
    if amax is None:
        amax = torch.zeros(T, device=logits.device, dtype=torch.int32)
    check(lib().emu_lookup_sample_bf16(_p(logits), logits.stride(0), V, T, _p(amax), _p(cur), _p(st), _p(pos0), _p(slot0), _p(ctx),
                                       _p(out_ids), _p(hist), hist.numel(), _p(drafts), int(max_ngram), int(max_new), int(min_len),
                                       int(eos_id), int(bool(stop_on_eos)), C.byref(params), _p(uniforms),
                                       0 if uniforms is None else uniforms.numel(), stream(logits)), "emu_lookup_sample_bf16")
    return amax


CONV_3X3,CONV_3X3_S2, CONV_3X3_UP2 = 1, 2, 3


def groupnorm_nhwc(x, gamma, beta, groups: int, eps: float, silu: bool = False):
    """x [B, HW, C] (NHWC) -> GroupNorm(groups)(+SiLU), same shape."""
    _req(x, "x")
    assert x.is_contiguous() and x.dim() == 3
    B, HW, Cc = x.shape
    ws = torch.empty(lib().emu_groupnorm_ws_bytes(B, HW, Cc), device=x.device, dtype=torch.uint8)
    y = torch.empty_like(x)
    check(lib().emu_groupnorm_nhwc_bf16(_p(x), _p(gamma), _p(beta), _p(y), _p(ws), B, HW, Cc, groups, float(eps), int(silu),
                                        stream(x)), "emu_groupnorm_nhwc_bf16")
    return y


def conv3x3_nhwc(x, w, bias=None, bias2=None, res=None, mode: int = CONV_3X3):
    """x [B, H, W, Cin] NHWC, w [Cout, 3, 3, Cin] -> [B, Ho, Wo, Cout]."""
    _req(x, "x"); _req(w, "w")
    assert x.is_contiguous() and w.is_contiguous()
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho, Wo = (H, W) if mode == CONV_3X3 else (((H + 1) // 2, (W + 1) // 2) if mode == CONV_3X3_S2 else (2 * H, 2 * W))
    y = torch.empty(B, Ho, Wo, Cout, device=x.device, dtype=BF16)
    check(lib().emu_conv3x3_nhwc_bf16(_p(x), _p(w), _p(bias), _p(bias2), bias2.stride(0) if bias2 is not None else 0, _p(res),
                                      _p(y), B, H, W, Cin, Cout, mode, stream(x)), "emu_conv3x3_nhwc_bf16")
    return y


def softmax_rows_(x, scale: float = 1.0, bias=None):
    """In-place x = bf16(softmax(x * scale [+ bias], dim=-1)) for a 2-D bf16 tensor (bias: bf16 [rows, cols])."""
    _req(x, "x")
    assert x.dim() == 2
    if bias is not None:
        _req(bias, "bias")
        assert bias.shape == x.shape
    check(lib().emu_softmax_rows_bf16(_p(x), _p(bias), x.shape[0], x.shape[1], x.stride(0),
                                      bias.stride(0) if bias is not None else 0, float(scale), stream(x)), "emu_softmax_rows_bf16")
    return x


def prefetch(t: torch.Tensor, workgroups: int = 256, nbytes: Optional[int] = None):
    """Touch the first ``nbytes`` (default: all) of a contiguous tensor into the infinity cache; see emu_prefetch."""
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError("prefetch needs a contiguous GPU tensor")
    n = t.numel() * t.element_size() if nbytes is None else int(nbytes)
    check(lib().emu_prefetch(_p(t), n, int(workgroups), stream(t)), "emu_prefetch")


def gemv_chain(ctx_handle, specs, err: Optional[torch.Tensor] = None):
    """A chain of one-row projections in ONE persistent launch (emu_gemv_chain_bf16; csrc/decode_engine.hip).  ``specs``: list of
    dicts with keys w [N, K], x ([1, K] or None = the previous op's output), gain, eps, epi, res, out (None when the next op takes
    the output).  Returns (outputs list with None for handed-over ones, err counter tensor).  Raises EmuHipError(-95) for shapes the
    engine does not cover."""
    import ctypes as C
    from ._lib import ChainOpC
    n = len(specs)
    arr = (ChainOpC * n)()
    keep, outs = [], []
    dev = specs[0]["w"].device
    for i, sp in enumerate(specs):
        w = sp["w"]; _req(w, "w")
        N, K = w.shape
        epi = int(sp.get("epi", EPI_NONE))
        x = sp.get("x")
        nxt_takes = i + 1 < n and specs[i + 1].get("x") is None
        out = None
        if not nxt_takes:
            out = sp.get("out")
            if out is None:
                out = torch.empty(1, N // 2 if epi == EPI_SWIGLU else N, device=dev, dtype=BF16)
        outs.append(out)
        gain, res = sp.get("gain"), sp.get("res")
        arr[i] = ChainOpC(_p(w), N, K, _p(gain), float(sp.get("eps", 0.0)), epi, _p(res), _p(x), 0 if x is not None else 1, _p(out))
        keep += [w, x, gain, res, out]
    nb = lib().emu_gemv_chain_granule_bytes(arr, n)
    gran = torch.empty(max(nb, 16), device=dev, dtype=torch.uint8)
    if err is None:
        err = torch.zeros(1, device=dev, dtype=torch.int32)
    check(lib().emu_gemv_chain_bf16(ctx_handle, arr, n, gran.data_ptr(), gran.numel(), err.data_ptr(), stream(dev)), "emu_gemv_chain_bf16")
    return outs, err, (gran, keep)


def image_resample_norm(src, plan, lut, out, ws=None):
    """emu_image_resample_norm: src uint8 [H, W, 3] (unit pixel / channel strides, any row pitch) -> out [3, S, S] bf16 or fp32 =
    Normalize(ToTensor(PIL bicubic resize)), bit-exact.  ``plan``: the device tables (emu_amd.preprocess.ResamplePlan); launch only."""
    _req(src, "src", torch.uint8)
    if src.dim() != 3 or src.shape[2] != 3 or src.stride(1) != 3 or tuple(src.shape[:2]) != (plan.h, plan.w):
        raise ValueError(f"src must be uint8 [{plan.h}, {plan.w}, 3] with interleaved pixels, got {tuple(src.shape)} strides {src.stride()}")
    if out.dtype not in (BF16, torch.float32) or not out.is_cuda or not out.is_contiguous() or out.dim() != 3 \
            or out.shape[0] != 3 or out.shape[1] != out.shape[2]:
        raise ValueError("out must be a contiguous GPU [3, S, S] tensor, bf16 or fp32")
    _req(lut, "lut", torch.float32)
    if ws is not None:
        _req(ws, "ws", torch.uint8)
    check(lib().emu_image_resample_norm(_p(src), src.stride(0), plan.h, plan.w, _p(plan.hcoef), _p(plan.hbounds), plan.hk,
                                        _p(plan.vcoef), _p(plan.vbounds), plan.vk, plan.row0, plan.nrows, _p(lut), _p(out),
                                        int(out.dtype == torch.float32), out.shape[1], _p(ws), ws.numel() if ws is not None else 0,
                                        stream(src)), "emu_image_resample_norm")
    return out


def image_to_u8_nhwc(x, out=None):
    """emu_image_to_u8_nhwc: bf16 [N, C, H, W] in [0, 1] -> uint8 [N, H, W, C] = rint(x * 255)."""
    _req(x, "x")
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError("x must be a contiguous [N, C, H, W] tensor")
    N, Cc, H, W = x.shape
    if out is None:
        out = torch.empty(N, H, W, Cc, device=x.device, dtype=torch.uint8)
    _req(out, "out", torch.uint8)
    check(lib().emu_image_to_u8_nhwc(_p(x), _p(out), N, Cc, H, W, stream(x)), "emu_image_to_u8_nhwc")
    return out
