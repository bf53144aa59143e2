"""Pin the CPU oracle (oracle/emu2_ref.py) against outputs of the REAL reference frozen in
tests/golden/ by oracle/make_golden.py (reference imported from /root/reference/Emu2/emu)."""
import numpy as np
import pytest
import torch

from oracle import emu2_ref as R
from tests import tiny

TOL = dict(rtol=2e-4, atol=2e-5)     # fp32 vs fp32, different op order only


def _t(a):
    return torch.from_numpy(np.asarray(a))


def test_vit_and_encode_image(golden_dir):
    z = tiny.load(golden_dir, "vit_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    cfg = tiny.oracle_cfg(v, l, vocab)
    image = _t(z["image"])
    feats = R.vit_forward(image, W, cfg.vit)
    torch.testing.assert_close(feats, _t(z["feats"]), **TOL)
    torch.testing.assert_close(R.encode_image(image, W, cfg), _t(z["encode"]), **TOL)
    torch.testing.assert_close(R.encode_image(image, W, cfg, n_query=1), _t(z["encode_nq1"]), **TOL)


def test_llama_model_ragged(golden_dir):
    z = tiny.load(golden_dir, "llama_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    cfg = tiny.oracle_cfg(v, l, vocab)
    embeds, mask = _t(z["embeds"]), _t(z["mask"])
    h = R.llama_model(embeds, mask, W, cfg.llama)
    ref = _t(z["hidden"])
    valid = mask.bool()
    torch.testing.assert_close(h[valid], ref[valid], **TOL)      # padded query rows are don't-care
    logits = torch.nn.functional.linear(h[:, -1], W["decoder.lm.lm_head.weight"])
    torch.testing.assert_close(logits, _t(z["logits"]), rtol=2e-4, atol=2e-4)


def test_generate_greedy_token_exact(golden_dir):
    z = tiny.load(golden_dir, "generate_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    cfg = tiny.oracle_cfg(v, l, vocab)
    new1, m1 = R.emu_generate(_t(z["ids1"]), _t(z["mask1"]), _t(z["image"]), W, cfg, max_new_tokens=8,
                              return_margins=True)
    assert new1.tolist() == z["new1"].tolist()
    new2, m2 = R.emu_generate(_t(z["ids2"]), _t(z["mask2"]), None, W, cfg, max_new_tokens=6,
                              return_margins=True)
    assert new2.tolist() == z["new2"].tolist()
    # the fixtures are only useful for bf16 kernels if the top-2 margin is not degenerate
    assert float(m1.min()) > 0.05 and float(m2.min()) > 0.05, (m1, m2)


def test_generate_multi_image_token_exact(golden_dir):
    """Several [<IMG_PLH>] blocks in one prompt with image=[n,3,H,W] (emu.py:196-203), and a ragged batch whose rows carry
    one and two images: greedy ids of the real reference, margins > 0.05 so a bf16 engine can be held to them."""
    z = tiny.load(golden_dir, "generate_multi_image_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    cfg = tiny.oracle_cfg(v, l, vocab)
    imgs = _t(z["images"])
    for tag, n_new in (("a", 8), ("b", 6)):
        ids = _t(z["ids_" + tag])
        n_img = int(z["n_img_" + tag])
        assert int((ids == 32003).sum()) == n_img * cfg.n_query and n_img >= 2
        new, m = R.emu_generate(ids, _t(z["mask_" + tag]), imgs[:n_img], W, cfg, max_new_tokens=n_new, return_margins=True)
        assert new.tolist() == z["new_" + tag].tolist()
        assert float(m.min()) > 0.05, m
    # swapping the two images of prompt a must change the result (the scatter is order-preserving, not a set)
    swapped = R.emu_generate(_t(z["ids_a"]), _t(z["mask_a"]), imgs[:2].flip(0), W, cfg, max_new_tokens=8)
    assert swapped.tolist() != z["new_a"].tolist()


def test_generate_video_token_exact(golden_dir):
    """Video frames ([gIMG] slots, v_query tokens per frame) alone and mixed with an image: ids of the real reference."""
    z = tiny.load(golden_dir, "generate_video_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    cfg = tiny.oracle_cfg(v, l, vocab)
    new4, m4 = R.emu_generate(_t(z["ids4"]), _t(z["mask4"]), None, W, cfg, max_new_tokens=6, return_margins=True,
                              video=_t(z["video"]))
    assert new4.tolist() == z["new4"].tolist()
    new5, m5 = R.emu_generate(_t(z["ids5"]), _t(z["mask5"]), _t(z["image"]), W, cfg, max_new_tokens=6,
                              return_margins=True, video=_t(z["video"]))
    assert new5.tolist() == z["new5"].tolist()
    print("video margins", m4.tolist(), m5.tolist())


def test_emu1_vit_g_and_causal_former_match_real_reference(golden_dir):
    """Emu1 caption path up to the LLaMA input: EVA-CLIP-g forward_features (pre-norm) -> ln_visual -> CausalFormer (T5
    decoder) against outputs of the REAL Emu1 modules (oracle/make_golden_emu1.py), fp32."""
    from oracle import emu1_ref as E
    z = tiny.load(golden_dir, "emu1_tiny.npz")
    v, t5, out_dim, W, cfg = tiny.emu1_from(z)
    img = _t(z["image"])
    feats = E.vit_g_forward(img, W, cfg.vit)
    assert feats.shape == tuple(z["feats"].shape)
    assert float((feats - _t(z["feats"])).norm() / _t(z["feats"]).norm()) < 1e-5
    lnv = torch.nn.functional.layer_norm(feats, (feats.shape[-1],), W["ln_visual.weight"], W["ln_visual.bias"], 1e-6)
    assert float((lnv - _t(z["ln_visual"])).norm() / _t(z["ln_visual"]).norm()) < 1e-5
    out = E.encode_image(img, W, cfg)
    assert out.shape == tuple(z["cformer"].shape) == (2, 8, out_dim)
    assert float((out - _t(z["cformer"])).norm() / _t(z["cformer"]).norm()) < 1e-5


def test_emu1_generate_matches_real_reference(golden_dir):
    """Emu.generate of the REAL Emu1 class (whole model in bf16, as inference.py runs it): greedy ids and the default
    5-beam search (length_penalty 0), in fp32 and in bf16 arithmetic."""
    from oracle import emu1_ref as E
    z = tiny.load(golden_dir, "emu1_generate_tiny.npz")
    v, t5, l, vocab, W, cfg = tiny.emu1_generate_from(z)
    ids, mask, img = _t(z["ids"]), _t(z["mask"]), _t(z["image"])
    for dt in (torch.float32, torch.bfloat16):
        Wd = R.cast_weights(W, dt)
        out, m = E.emu1_generate(ids, mask, img.to(dt), Wd, cfg, 6, num_beams=1, return_margins=True)
        assert out.tolist() == z["greedy"].tolist()
        assert float(m.min()) > 0.05, m
        beam = E.emu1_generate(ids, mask, img.to(dt), Wd, cfg, 6, num_beams=5)
        assert beam.tolist() == z["beam"].tolist()


def test_generate_beam_search_token_exact(golden_dir):
    """The reference's default decoding (num_beams=5, max_new_tokens=10, length_penalty=-1): ids of the real reference."""
    z = tiny.load(golden_dir, "generate_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    cfg = tiny.oracle_cfg(v, l, vocab)
    b1 = R.emu_generate(_t(z["ids1"]), _t(z["mask1"]), _t(z["image"]), W, cfg, max_new_tokens=10, num_beams=5)
    assert b1.tolist() == z["beam1"].tolist()
    b2 = R.emu_generate(_t(z["ids2"]), _t(z["mask2"]), None, W, cfg, max_new_tokens=10, num_beams=5)
    assert b2.tolist() == z["beam2"].tolist()
    # random-init models make beam pruning decisions near-ties (margin ~0.01 nat above); the 3-beam fixture used for the
    # bf16 GPU comparison must have a usable margin at every pruning boundary and between the two best results
    b3, margin = R.emu_generate(_t(z["ids3"]), _t(z["mask3"]), _t(z["image"]), W, cfg, max_new_tokens=6, num_beams=3,
                                return_margins=True)
    assert b3.tolist() == z["beam3"].tolist()
    assert margin > 0.08, margin


@pytest.mark.parametrize("cached", [False, True])
def test_generate_image(golden_dir, cached):
    z = tiny.load(golden_dir, "generate_image_tiny.npz")
    v, l, vocab, W = tiny.weights_from(z)
    cfg = tiny.oracle_cfg(v, l, vocab)
    fn = R.emu_generate_image_cached if cached else R.emu_generate_image_uncached
    out = fn(_t(z["prompt_text"]), None, W, cfg)
    torch.testing.assert_close(out, _t(z["out_text"]), rtol=1e-3, atol=1e-4)
    out = fn(_t(z["prompt_img"]), _t(z["image"]), W, cfg)
    torch.testing.assert_close(out, _t(z["out_img"]), rtol=1e-3, atol=1e-4)


def test_live_reference_bf16_matches_oracle_bf16(golden_dir):
    """The reference run in bf16 on CPU (its last hidden state frozen in tests/golden/llama_tiny_ref_bf16.npz by
    oracle/make_golden_ref_bf16.py; re-run live where the reference is importable, build container only): the oracle's bf16 mode
    reproduces its rounding points on lm.model (tolerance = 1 bf16 ulp-ish)."""
    from oracle import ref_import
    z = tiny.load(golden_dir, "llama_tiny.npz")
    zr = tiny.load(golden_dir, "llama_tiny_ref_bf16.npz")
    np.testing.assert_array_equal(zr["mask"], z["mask"])
    ref = _t(zr["hidden_bf16"])
    if ref_import.available():
        from oracle.make_golden_ref_bf16 import reference_bf16_hidden
        torch.testing.assert_close(reference_bf16_hidden(z).float(), ref, rtol=0, atol=0)
    v, l, vocab, W = tiny.weights_from(z)
    cfg = tiny.oracle_cfg(v, l, vocab)
    embeds, mask = _t(z["embeds"]).to(torch.bfloat16), _t(z["mask"])
    h = R.llama_model(embeds, mask, R.cast_weights(W, torch.bfloat16), cfg.llama)
    valid = mask.bool()
    torch.testing.assert_close(h[valid].float(), ref[valid].float(), rtol=2e-2, atol=2e-2)
