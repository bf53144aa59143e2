"""Host side of the GPU image front end (emu_amd/preprocess.py), checked on the CPU against Pillow itself.

``resample_coeffs`` restates how Pillow builds its 8-bit bicubic tables; the tables drive a short numpy integer resample here, and
its result must be array-equal to ``Image.resize((S, S), BICUBIC)`` -- the arithmetic the kernels of csrc/image.hip repeat."""
import numpy as np
import pytest
import torch
from PIL import Image

from emu_amd.chat import image_transform
from emu_amd.preprocess import (MAX_SIDE, gpu_shape_ok, normalize_lut, pillow_pass_order, resample_coeffs, select_path)

# downscale, upscale, identity, one axis only, degenerate, extreme aspect ratios, 12 MP (H, W)
SHAPES = [(600, 800), (1080, 1920), (100, 100), (300, 200), (448, 448), (224, 224), (448, 1000), (1000, 448), (1, 1), (2, 3),
          (7, 5000), (5000, 7), (3024, 4032)]
KINDS = ["random", "smooth", "binary"]
SIZES = [448, 224]


def make_image(h, w, kind, seed=0):
    rng = np.random.default_rng(seed + 7919 * h + w)
    if kind == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "smooth":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) % 256], -1).astype(np.uint8)
    return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)


def _pass(a, coef, bounds):
    """One resample pass along axis 1 of a uint8 [R, N, 3] array, in Pillow's integer arithmetic."""
    out = np.empty((a.shape[0], coef.shape[0], 3), np.uint8)
    for x in range(coef.shape[0]):
        x0, n = bounds[x]
        acc = (a[:, x0:x0 + n, :].astype(np.int32) * coef[x, :n][None, :, None]).sum(1, dtype=np.int32) + (1 << 21)
        out[:, x] = np.clip(acc >> 22, 0, 255).astype(np.uint8)
    return out


def integer_resample(a, size):
    """Two passes through a uint8 intermediate; a pass whose input size equals ``size`` is skipped; the horizontal pass covers only
    the rows the vertical pass reads.  Order as ``pillow_pass_order`` says."""
    h, w = a.shape[:2]
    hv = pillow_pass_order(h, w, size) == "hv"
    t = a
    for axis in ("h", "v") if hv else ("v", "h"):
        if axis == "h" and w != size:
            if hv and h != size:
                vb = resample_coeffs(h, size)[1]
                first, end = vb[0, 0], vb[-1, 0] + vb[-1, 1]
                full = np.zeros((h, size, 3), np.uint8)
                full[first:end] = _pass(t[first:end], *resample_coeffs(w, size))
                t = full
            else:
                t = _pass(t, *resample_coeffs(w, size))
        if axis == "v" and h != size:
            t = _pass(t.transpose(1, 0, 2), *resample_coeffs(h, size)).transpose(1, 0, 2)
    return t


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_integer_resample_equals_pillow(shape, kind, size):
    a = make_image(shape[0], shape[1], kind)
    want = np.asarray(Image.fromarray(a).resize((size, size), Image.BICUBIC))
    got = integer_resample(a, size)
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())


def test_coeff_tables_shape_and_bounds():
    for n, s in [(4032, 448), (7, 448), (448, 448), (1, 224), (16384, 224)]:
        coef, bounds = resample_coeffs(n, s)
        assert coef.dtype == bounds.dtype == np.int32 and coef.shape[0] == s and bounds.shape == (s, 2)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= n).all()
        assert bounds[:, 1].max() <= coef.shape[1] <= n
        assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(1)) >= 0).all()       # the kernels' strip spans rely on it
        assert np.abs(coef.sum(1) - (1 << 22)).max() <= coef.shape[1]                              # rows sum to one up to rounding
    coef, bounds = resample_coeffs(448, 448)                                                       # identity: one tap of weight 1
    k = np.arange(448) - bounds[:, 0]
    assert (coef[np.arange(448), k] == 1 << 22).all() and (np.abs(coef).sum(1) == 1 << 22).all()
    assert resample_coeffs(4032, 448)[0].shape[1] == 37


@pytest.mark.parametrize("size", [16, 8])
def test_lut_equals_image_transform(size):
    """All 256 values in every channel of a 16 x 16 image: the table is ``image_transform``'s arithmetic, fp32 and bf16."""
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    a = np.stack([v, v[::-1], v.T], -1)
    mean, std = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
    want = image_transform(Image.fromarray(a), 16, mean, std)                 # 16 -> 16: no resample, every value survives
    lut = normalize_lut(mean, std)
    assert lut.shape == (3, 256) and lut.dtype == torch.float32
    got = torch.stack([lut[c][torch.from_numpy(a[:, :, c].astype(np.int64))] for c in range(3)])
    assert torch.equal(got, want)
    assert torch.equal(got.to(torch.bfloat16), want.to(torch.bfloat16))
    if size == 8:                                                              # and through a real resample
        want = image_transform(Image.fromarray(a), 8, mean, std)
        r = integer_resample(a, 8)
        got = torch.stack([lut[c][torch.from_numpy(r[:, :, c].astype(np.int64))] for c in range(3)])
        assert torch.equal(got, want)


def test_fallback_rules():
    rgb = Image.fromarray(make_image(20, 30, "random"))
    assert select_path(rgb, 448) == "gpu"
    for mode in ("L", "RGBA", "P", "I;16", "CMYK", "1"):
        assert select_path(rgb.convert(mode) if mode != "I;16" else Image.new("I;16", (30, 20)), 448) == "host", mode
    assert select_path(np.zeros((20, 30, 3), np.uint8), 448) == "gpu"
    assert select_path(torch.zeros(20, 30, 3, dtype=torch.uint8), 448) == "gpu"
    assert select_path(np.zeros((20, 30), np.uint8), 448) == "host"
    assert select_path(np.zeros((20, 30, 4), np.uint8), 448) == "host"
    assert select_path(np.zeros((20, 30, 3), np.float32), 448) == "host"
    assert select_path(Image.new("RGB", (MAX_SIDE + 1, 2)), 448) == "host"     # oversize
    assert select_path(Image.new("RGB", (2, MAX_SIDE + 1)), 448) == "host"
    assert select_path(Image.new("RGB", (MAX_SIDE, 2)), 448) == "gpu"
    assert not gpu_shape_ok(16384, 16384, 8)                                   # more taps than the kernels take
    assert gpu_shape_ok(16384, 16384, 224) and gpu_shape_ok(3024, 4032, 448)
    assert select_path(Image.new("RGB", (7, 5000)), 448) == "host"             # Pillow resamples H > 100 W vertically first
    assert select_path(Image.new("RGB", (7, 700)), 448) == "gpu"
    with pytest.raises(TypeError):
        select_path("not an image", 448)
