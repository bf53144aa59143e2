"""GPU image front end and back end (csrc/image.hip, emu_amd/preprocess.py): bit-exact with the host path.

Every comparison is ``torch.equal`` / ``array_equal`` against what the option-off code computes: ``image_transform`` (Pillow bicubic
resize -> ToTensor -> Normalize) on the way in, ``numpy_to_pil`` on the way out."""
import re

import numpy as np
import pytest
import torch
from PIL import Image

from tests import tiny
from tests.test_preprocess_host import KINDS, SHAPES, SIZES, make_image

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda"


def _transforms(size):
    from emu_amd.preprocess import GpuImageTransform
    return {d: GpuImageTransform(size, device=DEV, dtype=d) for d in (torch.float32, BF16)}


@pytest.fixture(scope="module")
def transforms():
    return {s: _transforms(s) for s in SIZES}


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_transform_equals_host(transforms, shape, size):
    from emu_amd.chat import image_transform
    for kind in KINDS:
        img = Image.fromarray(make_image(shape[0], shape[1], kind))
        want = image_transform(img, size)
        got32 = transforms[size][torch.float32](img)
        got16 = transforms[size][BF16](img)
        assert got32.dtype == torch.float32 and got16.dtype == BF16 and got32.is_cuda and got32.shape == (3, size, size)
        assert torch.equal(got32, want.to(DEV)), (kind, int((got32.cpu() != want).sum()))
        assert torch.equal(got16, want.to(BF16).to(DEV)), kind


@pytest.mark.parametrize("size", SIZES)
def test_input_forms_and_row_pitch(transforms, size):
    """numpy array, host tensor, device tensor, and a device tensor whose rows are further apart than 3 * W bytes (odd pitch, so
    rows start at every alignment)."""
    from emu_amd.chat import image_transform
    for h, w, pad in [(600, 800, 5), (37, 53, 2), (size, 301, 7), (500, size, 3), (size, size, 1)]:
        a = make_image(h, w, "random", seed=3)
        want = image_transform(Image.fromarray(a), size).to(DEV)
        tf = transforms[size][torch.float32]
        assert torch.equal(tf(a), want)
        assert torch.equal(tf(torch.from_numpy(a)), want)
        assert torch.equal(tf(torch.from_numpy(a).to(DEV)), want)
        wide = torch.zeros(h, w + pad, 3, dtype=torch.uint8)
        wide[:, :w] = torch.from_numpy(a)
        wide[:, w:] = 255                                                      # must never be read
        view = wide.to(DEV)[:, :w]
        assert not view.is_contiguous() and view.stride(0) == 3 * (w + pad)
        assert torch.equal(tf(view), want)
        assert torch.equal(transforms[size][BF16](view), want.to(BF16))


def test_fallback_inputs_match_host(transforms):
    from emu_amd.chat import image_transform
    a = make_image(40, 60, "random")
    for img in (Image.fromarray(a).convert("L"), Image.fromarray(make_image(5000, 7, "smooth")),
                Image.fromarray(make_image(2, 16500, "random"))):
        want = image_transform(img, 224)
        assert torch.equal(transforms[224][torch.float32](img), want.to(DEV))
        assert torch.equal(transforms[224][BF16](img), want.to(BF16).to(DEV))
    rgba = Image.fromarray(a).convert("RGBA")                                  # what the host path refuses, the option refuses alike
    with pytest.raises(RuntimeError):
        image_transform(rgba, 224)
    with pytest.raises(RuntimeError):
        transforms[224][BF16](rgba)


def test_batch(transforms):
    tf = transforms[448][BF16]
    imgs = [Image.fromarray(make_image(h, w, "random", seed=i)) for i, (h, w) in
            enumerate([(600, 800), (448, 448), (100, 700), (1080, 1920), (31, 17)])]
    got = tf.batch(imgs)
    assert got.shape == (5, 3, 448, 448)
    assert torch.equal(got, torch.stack([tf(i) for i in imgs]))
    mixed = [imgs[0], imgs[1].convert("L"), np.array(imgs[2]), torch.from_numpy(np.array(imgs[3])).to(DEV)]
    assert torch.equal(tf.batch(mixed), torch.stack([tf(i) for i in mixed]))
    frames = [make_image(360, 640, "smooth", seed=i) + np.uint8(i) for i in range(12)]
    got = tf.batch(frames)
    assert got.shape == (12, 3, 448, 448) and torch.equal(got, torch.stack([tf(f) for f in frames]))
    assert len(tf._tables) <= tf.TABLE_CACHE


@pytest.fixture(scope="module")
def tiny_model(golden_dir):
    from emu_amd import EmuModel, TextDecoderCfg
    z = tiny.load(golden_dir, "generate_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    m = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda")
    m.load_state_dict(W, strict=True)
    return m, v


def test_vit_sees_the_same_image(tiny_model):
    """encode_image(bf16 from the GPU transform) is bit-identical to encode_image(fp32 from the host transform): the stem's own
    fp32 -> bf16 conversion rounds to nearest even, which is what the kernel's bf16 output is."""
    from emu_amd.chat import image_transform
    from emu_amd.preprocess import GpuImageTransform
    m, v = tiny_model
    tf = GpuImageTransform(v.image_size, device=DEV)
    assert tf.dtype == BF16
    imgs = [Image.fromarray(make_image(h, w, "random", seed=9)) for h, w in [(600, 800), (90, 50)]]
    host = torch.stack([image_transform(i, v.image_size) for i in imgs]).to(DEV)
    dev = tf.batch(imgs)
    assert host.dtype == torch.float32 and dev.dtype == BF16
    assert torch.equal(m.encode_image(dev), m.encode_image(host))


class _Tok:
    """Tokenizer stand-in: special tokens get their ids, every other character one id of its own."""
    SPECIAL = {"[IMG]": 32001, "[/IMG]": 32002, "<image>": 32003, "[gIMG]": 32004, "[VIDEO]": 32007}

    def __call__(self, text, padding="longest", return_tensors="pt"):
        pat = re.compile("|".join(re.escape(k) for k in self.SPECIAL))
        rows = []
        for t in text:
            ids, pos = [1], 0
            for mt in pat.finditer(t):
                ids += [3 + ord(c) % 200 for c in t[pos:mt.start()]] + [self.SPECIAL[mt.group()]]
                pos = mt.end()
            rows.append(ids + [3 + ord(c) % 200 for c in t[pos:]])
        n = max(len(r) for r in rows)
        out = type("Enc", (), {})()
        out.input_ids = torch.tensor([[32000] * (n - len(r)) + r for r in rows])
        out.attention_mask = torch.tensor([[0] * (n - len(r)) + [1] * len(r) for r in rows])
        return out

    def batch_decode(self, ids, skip_special_tokens=True):
        return [" ".join(str(int(i)) for i in row) for row in ids]


def test_chat_generation_same_ids(tiny_model):
    from emu_amd.chat import EmuChatGeneration
    m, v = tiny_model
    m.decoder.tokenizer = _Tok()
    off = EmuChatGeneration(m, eva_size=v.image_size, gpu_preprocess=False)
    on = EmuChatGeneration(m, eva_size=v.image_size, gpu_preprocess=True)
    assert not off.gpu_preprocess and on.gpu_preprocess
    a, b = Image.fromarray(make_image(600, 800, "random", seed=1)), Image.fromarray(make_image(70, 45, "smooth", seed=2))
    kw = dict(num_beams=1, max_new_tokens=8)
    chat = [["compare", a, "with", b], ["the first"], ["why?"]]
    assert on(chat, **kw) == off(chat, **kw)
    frames = [Image.fromarray(make_image(90, 160, "smooth", seed=i)) for i in range(3)]
    video = ["[VIDEO]", *frames, "[/VIDEO]", "what happens", a]
    assert on(video, **kw) == off(video, **kw)
    arrays = ["[VIDEO]", *[np.asarray(f) for f in frames], "[/VIDEO]", "what happens", torch.from_numpy(np.array(a)).to(DEV)]
    assert on(arrays, **kw) == off(video, **kw)                               # decoder-style inputs: arrays and device tensors


def test_option_default_reads_environment(tiny_model, monkeypatch):
    from emu_amd.chat import EmuChatGeneration
    from emu_amd.preprocess import GpuImageTransform
    m, v = tiny_model
    monkeypatch.delenv("EMU_GPU_PREPROCESS", raising=False)
    assert not EmuChatGeneration(m).gpu_preprocess
    monkeypatch.setenv("EMU_GPU_PREPROCESS", "1")
    c = EmuChatGeneration(m)
    assert c.gpu_preprocess and isinstance(c.transform, GpuImageTransform)
    assert not EmuChatGeneration(m, gpu_preprocess=False).gpu_preprocess


def test_every_bf16_value_to_byte():
    """Every bf16 bit pattern in [0, 1]: the byte equals numpy_to_pil's (x * 255).round().astype(uint8)."""
    from emu_amd.preprocess import to_uint8_hwc
    bits = torch.arange(0, 0x3F80 + 1, dtype=torch.int32).to(torch.int16)     # +0.0 .. 1.0
    x = bits.view(BF16)
    assert float(x[0]) == 0.0 and float(x[-1]) == 1.0 and bool((x.float() >= 0).all()) and bool((x.float() <= 1).all())
    want = (x.float().numpy() * 255).round().astype("uint8")
    n = x.numel()
    for c, shape in [(1, (1, 1, 1, n)), (3, (1, 3, 1, n))]:                    # scalar form (C = 1; n odd) and C = 3
        got = to_uint8_hwc(x.repeat(c).view(shape).to(DEV)).cpu().numpy()
        assert got.shape == (1, 1, n, c) and all(np.array_equal(got[0, 0, :, k], want) for k in range(c))
    pad = torch.cat([x, x[:3]])                                                # vector form: C = 3, H * W % 4 == 0
    assert pad.numel() % 4 == 0
    got = to_uint8_hwc(pad.repeat(3).view(1, 3, 4, -1).to(DEV)).cpu().numpy().reshape(-1, 3)
    assert all(np.array_equal(got[:n, k], want) for k in range(3))


def test_to_uint8_layout():
    from emu_amd.preprocess import to_uint8_hwc
    g = torch.Generator().manual_seed(4)
    x = torch.rand(2, 3, 64, 48, generator=g).to(BF16)
    want = (x.permute(0, 2, 3, 1).float().numpy() * 255).round().astype("uint8")
    got = to_uint8_hwc(x.to(DEV))
    assert got.dtype == torch.uint8 and got.shape == (2, 64, 48, 3) and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(to_uint8_hwc(x[0].to(DEV)).cpu().numpy(), want[0])
    y = torch.rand(1, 3, 5, 7, generator=g).to(BF16)                           # H * W % 4 != 0
    assert np.array_equal(to_uint8_hwc(y.to(DEV)).cpu().numpy(), (y.permute(0, 2, 3, 1).float().numpy() * 255).round().astype("uint8"))


def test_resample_captured_in_a_graph(transforms):
    """plan() uploads, run() only launches: captured and replayed it gives the eager bytes."""
    tf = transforms[448][BF16]
    a = make_image(600, 800, "random", seed=5)
    b = make_image(600, 800, "binary", seed=6)
    want_a, want_b = tf(a), tf(b)
    plan = tf.plan(600, 800)
    src = torch.from_numpy(a).to(DEV)
    out = torch.zeros(3, 448, 448, device=DEV, dtype=BF16)
    ws = torch.empty(plan.ws_bytes, device=DEV, dtype=torch.uint8)
    tf.run(plan, src, out, ws)                                                 # warm-up outside the capture
    torch.cuda.synchronize()
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tf.run(plan, src, out, ws)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want_a)
    src.copy_(torch.from_numpy(b).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want_b)


def test_status_for_bad_sizes(transforms):
    """-22 through the status only: the library refuses before any launch."""
    from emu_amd._lib import lib
    tf = transforms[448][BF16]
    plan = tf.plan(600, 800)
    src = torch.zeros(600, 800, 3, device=DEV, dtype=torch.uint8)
    out = torch.zeros(3, 448, 448, device=DEV, dtype=BF16)
    ws = torch.empty(plan.ws_bytes, device=DEV, dtype=torch.uint8)
    s = torch.cuda.current_stream().cuda_stream

    def call(h=600, w=800, pitch=2400, size=448, ws_bytes=plan.ws_bytes, hk=plan.hk):
        return lib().emu_image_resample_norm(src.data_ptr(), pitch, h, w, plan.hcoef.data_ptr(), plan.hbounds.data_ptr(), hk,
                                             plan.vcoef.data_ptr(), plan.vbounds.data_ptr(), plan.vk, plan.row0, plan.nrows,
                                             tf._lut.data_ptr(), out.data_ptr(), 0, size, ws.data_ptr(), ws_bytes, s)
    assert call(w=16385) == -22 and call(h=16385) == -22
    assert call(size=4097) == -22
    assert call(ws_bytes=plan.nrows * 1344 - 1) == -22 and call(ws_bytes=0) == -22
    assert call(pitch=2399) == -22 and call(hk=1025) == -22
    assert lib().emu_image_resample_ws_bytes(600, 800, 448) == 600 * 1344 and lib().emu_image_resample_ws_bytes(600, 448, 448) == 0
    assert lib().emu_image_to_u8_nhwc(out.data_ptr(), ws.data_ptr(), 1, 5, 4, 4, s) == -22
    assert lib().emu_image_to_u8_nhwc(out.data_ptr(), ws.data_ptr(), 1, 3, 16385, 4, s) == -22
    assert call() == 0
    torch.cuda.synchronize()


def test_visual_generation_pixel_identical():
    """EmuVisualGeneration on the tiny fixture of tests/test_gpu_unet.py: the prompt embeddings (autoencoding mode) and the returned
    PIL image are identical with the option on and off."""
    from emu_amd import CLIPVisionCfg, EmuModel, LlamaCfg, TextDecoderCfg, synth
    from emu_amd.diffusion import EmuVisualGeneration
    from emu_amd.llama import EmuHipContext
    from emu_amd.unet import UNetCfg, UNetEngine, unet_param_shapes
    from emu_amd.vae import VaeCfg, VaeDecoder, vae_decoder_param_shapes
    ctx = EmuHipContext(torch.device("cuda", 0))
    dec = VaeDecoder(VaeCfg(block_out_channels=(64, 64, 128, 128)), ctx)
    Wv = synth.synth_state_dict(vae_decoder_param_shapes(dec.cfg), seed=9, dtype=torch.float32)
    assert dec.load_state_dict({k: (v * (2.0 if v.dim() > 1 else 1.0)) for k, v in Wv.items()}) == []
    vis = CLIPVisionCfg(image_size=56, patch_size=14, width=128, layers=1, head_width=64, mlp_ratio=2.0, n_query=4, v_query=4)
    lcfg = LlamaCfg(hidden_size=128, intermediate_size=256, num_attention_heads=1, num_hidden_layers=1)
    enc = EmuModel(vis, TextDecoderCfg(), llama_cfg=lcfg, device="cuda", ctx=ctx)
    enc.load_state_dict(synth.synth_state_dict(synth.emu_param_shapes(vis, lcfg, 32272), seed=2))
    ucfg = UNetCfg(block_out_channels=(64, 128, 256), transformer_layers_per_block=(1, 1, 2), num_heads=(1, 2, 4),
                   cross_attention_dim=128, projection_class_embeddings_input_dim=128 + 6 * 256)
    Wu = synth.synth_state_dict(unet_param_shapes(ucfg), seed=5)
    unet = UNetEngine(ucfg, ctx)
    unet.load_state_dict({k: (v * (2.0 if v.dim() > 1 else 1.0)) for k, v in Wu.items()})
    off = EmuVisualGeneration(multimodal_encoder=enc, unet=unet, vae=dec, eva_size=56, gpu_preprocess=False)
    on = EmuVisualGeneration(multimodal_encoder=enc, unet=unet, vae=dec, eva_size=56, gpu_preprocess=True)
    pil = Image.fromarray(make_image(40, 60, "random", seed=1))
    for cfg in (True, False):
        assert torch.equal(on._prepare_and_encode_inputs([pil], cfg), off._prepare_and_encode_inputs([pil], cfg))
    torch.manual_seed(0)
    want = off([pil], height=128, width=128, num_inference_steps=3, guidance_scale=3.0)
    torch.manual_seed(0)
    got = on([pil], height=128, width=128, num_inference_steps=3, guidance_scale=3.0)
    assert got.nsfw_content_detected is None and got.image.size == want.image.size == (128, 128) and got.image.mode == "RGB"
    assert np.array_equal(np.asarray(got.image), np.asarray(want.image))
    # a safety checker wants float images: that case stays on the host tail
    checked = EmuVisualGeneration(multimodal_encoder=enc, unet=unet, vae=dec, eva_size=56, gpu_preprocess=True,
                                  safety_checker=lambda im: (im, [False]))
    torch.manual_seed(0)
    out = checked([pil], height=128, width=128, num_inference_steps=3, guidance_scale=3.0)
    assert out.nsfw_content_detected is False and np.array_equal(np.asarray(out.image), np.asarray(want.image))
