"""Image pre- and post-processing on the device, bit-exact with the host path.

In: ``GpuImageTransform`` computes what ``emu_amd.chat.image_transform`` computes -- ``PIL.Image.resize((S, S), BICUBIC)``, ToTensor,
Normalize (Emu2/emu/chat.py:35-39, Emu2/emu/diffusion.py:58-63) -- from the uint8 pixels with the kernels of csrc/image.hip.  Pillow's
8-bit resample is integer arithmetic once its coefficient tables exist; ``resample_coeffs`` restates how Pillow builds them
(``precompute_coeffs`` + ``normalize_coeffs_8bpc`` of src/libImaging/Resample.c, bicubic filter) in numpy doubles, which is the one
place where bit-exactness is decided and is checked on the CPU (tests/test_preprocess_host.py).  ToTensor + Normalize is a 3 x 256
table built with the very expression ``image_transform`` evaluates.

Out: ``to_uint8_hwc`` is ``numpy_to_pil``'s ``(x * 255).round().astype("uint8")`` (diffusion.py:214-234) on the decoded bf16 NCHW image.

Whatever the kernels do not cover (a PIL mode other than RGB, a side above 16384, more than 1024 taps, H > 100 W) goes through the host
``image_transform`` and is moved to the device: the option never changes what a prompt computes.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .constants import EVA_IMAGE_SIZE, OPENAI_DATASET_MEAN, OPENAI_DATASET_STD

PRECISION_BITS = 32 - 8 - 2            # Pillow's 8-bit coefficient precision: 22 fractional bits
MAX_SIDE = 16384                       # EMU_IMAGE_MAX_SIDE
MAX_OUT = 4096                         # EMU_IMAGE_MAX_OUT
MAX_TAPS = 1024                        # EMU_IMAGE_MAX_TAPS
_LDS_MAX = 60 * 1024                   # csrc/image.hip: IMG_LDS_MAX
BF16 = torch.bfloat16


def _bicubic(x: np.ndarray) -> np.ndarray:
    """Pillow's ``bicubic_filter`` (a = -0.5), operation for operation in double."""
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def resample_coeffs(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's bicubic tables for resampling ``in_size`` pixels to ``out_size``: (coeffs int32 [out, ksize], bounds int32 [out, 2]).
    ``bounds[x] = (first tap, tap count)``; output x is ``clip8((1 << 21) + sum_k in[first + k] * coeffs[x, k]) >> 22)``.  ksize is
    Pillow's ``ceil(support) * 2 + 1`` (support = 2 * max(in / out, 1)), cut to ``in_size`` (no output has more taps than that)."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("sizes must be positive")
    scale = float(np.float32(in_size) - np.float32(0.0)) / out_size          # (double)(in1 - in0) / outSize, the box is float
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    xx = np.arange(out_size, dtype=np.float64)
    center = 0.0 + (xx + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)           # (int) truncates toward zero
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    ksize = min(ksize, in_size)
    k = np.arange(ksize, dtype=np.int64)[None, :]
    w = _bicubic(((k + xmin[:, None]) - center[:, None] + 0.5) * ss)
    w = np.where(k < xmax[:, None], w, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                                         # sequential sum, as the C loop (np.sum is pairwise)
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    q = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)   # truncation
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    return np.ascontiguousarray(q.astype(np.int32)), np.ascontiguousarray(bounds)


def normalize_lut(mean=OPENAI_DATASET_MEAN, std=OPENAI_DATASET_STD) -> torch.Tensor:
    """fp32 [3, 256]: ToTensor + Normalize of every byte value, with the expression ``image_transform`` evaluates."""
    t = torch.arange(256, dtype=torch.uint8)[None, :].expand(len(mean), 256).to(torch.float32) / 255.0
    m = torch.tensor(mean, dtype=torch.float32)[:, None]
    s = torch.tensor(std, dtype=torch.float32)[:, None]
    return ((t - m) / s).contiguous()


def _h_pass_fits(w: int, s: int, hk: int) -> bool:
    """csrc/image.hip::pick_tx: some strip width's coefficients and source span fit in LDS."""
    for tx in (64, 32, 16, 8):
        span = min(((tx - 1) * w + s - 1) // s + hk + 2, w)
        if tx * (hk | 1) * 4 + (span * 3 + 8 + 3) // 4 * 4 <= _LDS_MAX:
            return True
    return False


def gpu_shape_ok(h: int, w: int, size: int) -> bool:
    """The kernels cover an H x W source resampled to size x size (pure host arithmetic; mirrors the library's -22 rules)."""
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE and 1 <= size <= MAX_OUT):
        return False
    for n in (h, w):
        if n != size:
            sup = 2.0 * max(n / size, 1.0)
            if min(int(math.ceil(sup)) * 2 + 1, n) > MAX_TAPS:
                return False
    if w != size and not _h_pass_fits(w, size, min(int(math.ceil(2.0 * max(w / size, 1.0))) * 2 + 1, w)):
        return False
    return True


def pillow_pass_order(h: int, w: int, size: int) -> str:
    """"hv" (horizontal pass first: ImagingResample's own order) or "vh": ``Image.resize`` of recent Pillow releases resamples a
    very tall image (H > 100 * W, shrinking vertically) in two calls, vertical first.  The two orders round differently, and the
    kernels implement "hv" only, so "vh" shapes take the host path."""
    return "vh" if h > w * 100 and size < h else "hv"


def select_path(img, size: int) -> str:
    """"gpu" or "host" for one input: PIL mode RGB, a numpy uint8 [H, W, 3] array or a torch.uint8 [H, W, 3] tensor whose shape the
    kernels cover take the GPU path; anything else (other PIL modes, oversize shapes, ``pillow_pass_order`` "vh") the host
    ``image_transform``."""
    if isinstance(img, torch.Tensor):
        ok = img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3
        shape = tuple(img.shape[:2])
    elif isinstance(img, np.ndarray):
        ok = img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
        shape = tuple(img.shape[:2])
    elif hasattr(img, "mode") and hasattr(img, "size"):
        ok = img.mode == "RGB"
        shape = (img.size[1], img.size[0])
    else:
        raise TypeError(f"expected a PIL image, a uint8 [H, W, 3] array or tensor, got {type(img)}")
    ok = ok and gpu_shape_ok(shape[0], shape[1], size) and pillow_pass_order(shape[0], shape[1], size) == "hv"
    return "gpu" if ok else "host"


class ResamplePlan:
    """Device tables of one (H, W) -> S resample; everything a launch needs besides the pixels."""
    __slots__ = ("h", "w", "hcoef", "hbounds", "hk", "vcoef", "vbounds", "vk", "row0", "nrows", "ws_bytes")


class GpuImageTransform:
    """``image_transform`` on the device: ``transform(img) -> [3, S, S]`` and ``transform.batch(imgs) -> [N, 3, S, S]`` device tensors of
    ``dtype`` (bf16: the round-to-nearest-even of the fp32 value, what the ViT stem makes of an fp32 image; or fp32), equal to
    ``image_transform(img, size, mean, std)`` bit for bit."""
    TABLE_CACHE = 32                    # (in_size, out_size) table pairs kept on the device
    PINNED_MAX = 64 << 20               # staging buffer bound; a larger image is copied from pageable memory

    def __init__(self, size: int = EVA_IMAGE_SIZE, mean=OPENAI_DATASET_MEAN, std=OPENAI_DATASET_STD, device="cuda",
                 dtype: torch.dtype = BF16):
        if dtype not in (BF16, torch.float32):
            raise ValueError("dtype must be torch.bfloat16 or torch.float32")
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("mean and std must have three entries (RGB)")
        self.size, self.mean, self.std = int(size), tuple(mean), tuple(std)
        self.device, self.dtype = torch.device(device), dtype
        self._lut: Optional[torch.Tensor] = None
        self._tables: "OrderedDict[Tuple[int, int], tuple]" = OrderedDict()
        self._pinned: Optional[torch.Tensor] = None
        self._pinned_free: Optional[torch.cuda.Event] = None

    # ------------------------------------------------------------------ tables (uploads happen here, never between launches)
    def _table(self, n: int):
        key = (n, self.size)
        hit = self._tables.get(key)
        if hit is not None:
            self._tables.move_to_end(key)
            return hit
        coef, bounds = resample_coeffs(n, self.size)
        ent = (torch.from_numpy(coef).to(self.device), torch.from_numpy(bounds).to(self.device), coef.shape[1],
               int(bounds[0, 0]), int(bounds[-1, 0] + bounds[-1, 1]))
        self._tables[key] = ent
        while len(self._tables) > self.TABLE_CACHE:
            self._tables.popitem(last=False)
        return ent

    def plan(self, h: int, w: int) -> ResamplePlan:
        from ._lib import lib
        if not gpu_shape_ok(h, w, self.size):
            raise ValueError(f"{h} x {w} -> {self.size} is outside what the resample kernels cover")
        if self._lut is None:
            self._lut = normalize_lut(self.mean, self.std).to(self.device)
        p = ResamplePlan()
        p.h, p.w = int(h), int(w)
        p.hcoef = p.hbounds = p.vcoef = p.vbounds = None
        p.hk = p.vk = 0
        p.row0, p.nrows = 0, p.h
        if w != self.size:
            p.hcoef, p.hbounds, p.hk, _, _ = self._table(w)
        if h != self.size:
            p.vcoef, p.vbounds, p.vk, first, end = self._table(h)
            p.row0, p.nrows = first, end - first
        p.ws_bytes = int(lib().emu_image_resample_ws_bytes(p.h, p.w, self.size))
        return p

    def run(self, plan: ResamplePlan, src: torch.Tensor, out: torch.Tensor, ws: Optional[torch.Tensor]) -> torch.Tensor:
        """Launch only (no allocation, upload or synchronisation: capturable).  src uint8 [H, W, 3] on the device with unit channel
        and pixel strides (any row pitch), out [3, S, S] of this transform's dtype, ws uint8 of at least ``plan.ws_bytes``."""
        from . import ops
        return ops.image_resample_norm(src, plan, self._lut, out, ws)

    # ------------------------------------------------------------------ inputs
    def _host_fallback(self, img) -> torch.Tensor:
        from .chat import image_transform
        if not hasattr(img, "resize"):
            from PIL import Image
            a = img.cpu().numpy() if isinstance(img, torch.Tensor) else img
            img = Image.fromarray(np.ascontiguousarray(a))
        return image_transform(img, self.size, self.mean, self.std).to(self.device, self.dtype)

    @staticmethod
    def _pitched(t: torch.Tensor) -> torch.Tensor:
        return t if t.stride(2) == 1 and t.stride(1) == 3 and t.stride(0) >= 3 * t.shape[1] else t.contiguous()

    def _stage(self, arrays: Sequence[np.ndarray]) -> List[torch.Tensor]:
        """Host pixels -> device uint8 tensors: packed into the pinned staging buffer and sent with one asynchronous copy per group
        of images that fits in it."""
        outs: List[Optional[torch.Tensor]] = [None] * len(arrays)
        group, used = [], 0

        def flush():
            nonlocal group, used
            if not group:
                return
            if self._pinned is None or self._pinned.numel() < used:
                self._pinned = torch.empty(max(used, 1 << 20), dtype=torch.uint8).pin_memory()
                self._pinned_free = None
            if self._pinned_free is not None:
                self._pinned_free.synchronize()                               # the previous group's copy has left the buffer
            host = self._pinned.numpy()
            off = 0
            for i in group:
                a = arrays[i]
                np.copyto(host[off:off + a.size].reshape(a.shape), a)
                off += a.size
            dev = self._pinned[:used].to(self.device, non_blocking=True)
            self._pinned_free = torch.cuda.Event()
            self._pinned_free.record(torch.cuda.current_stream(self.device))
            off = 0
            for i in group:
                a = arrays[i]
                outs[i] = dev[off:off + a.size].view(a.shape)
                off += a.size
            group, used = [], 0

        for i, a in enumerate(arrays):
            if a.size > self.PINNED_MAX:
                outs[i] = torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
                continue
            if used + a.size > self.PINNED_MAX:
                flush()
            group.append(i)
            used += a.size
        flush()
        return outs

    def batch(self, images: Sequence) -> torch.Tensor:
        """One [N, 3, S, S] tensor for N images of any sizes: tables first, then one staged upload, then the launches."""
        n, S = len(images), self.size
        out = torch.empty(n, 3, S, S, device=self.device, dtype=self.dtype)
        todo, host_arrays, host_slots = [], [], []
        for i, img in enumerate(images):
            if select_path(img, S) == "host":
                out[i] = self._host_fallback(img)
                continue
            if isinstance(img, torch.Tensor) and img.is_cuda:
                src = self._pitched(img.to(self.device))
                todo.append([i, self.plan(src.shape[0], src.shape[1]), src])
                continue
            a = img.numpy() if isinstance(img, torch.Tensor) else np.asarray(img)
            todo.append([i, self.plan(a.shape[0], a.shape[1]), None])
            host_slots.append(len(todo) - 1)
            host_arrays.append(a)
        with torch.cuda.device(self.device):
            for slot, dev in zip(host_slots, self._stage(host_arrays)):
                todo[slot][2] = dev
            ws_bytes = max([p.ws_bytes for _, p, _ in todo], default=0)
            ws = torch.empty(ws_bytes, device=self.device, dtype=torch.uint8) if ws_bytes else None
            for i, p, src in todo:
                self.run(p, src, out[i], ws)
        return out

    def __call__(self, img) -> torch.Tensor:
        return self.batch([img])[0]


def to_uint8_hwc(image_nchw: torch.Tensor) -> torch.Tensor:
    """bf16 [N, C, H, W] (or [C, H, W]) in [0, 1] on the device -> uint8 [N, H, W, C] (or [H, W, C]) device tensor equal to
    ``(x.float().permute(0, 2, 3, 1).numpy() * 255).round().astype("uint8")``."""
    from . import ops
    if image_nchw.dim() == 3:
        return ops.image_to_u8_nhwc(image_nchw[None])[0]
    return ops.image_to_u8_nhwc(image_nchw)
