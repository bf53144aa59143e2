"""GPU tests of the MXFP4 GEMM for 17 rows and more (csrc/gemm_fp4.hip, ``ops.linear_fp4w_gemm``,
``LlamaEngine.use_fp4(True, wide=True, all_rows=True)``, ``LlamaEngine.release_bf16``).

The kernel is W4A16: weights are decoded to bf16 exactly and multiplied on the bf16 matrix cores, so it computes what the bf16 GEMM
computes on the dequantised weights up to fp32 summation order.  The tolerances are those tests/test_gpu_fp4_wide.py uses for the same
arithmetic.  (a) the decode of every code in every nibble / byte position, exactly, all one-hot rows in ONE call; (b) the linear, plain
and with the residual, on both sides of every row-tile boundary of the three instantiations (32 / 64 / 128 rows); (c) bias and SwiGLU;
(d) the rejections; (e) an engine prefill in mode 3 against the CPU oracle on the dequantised weights, with a witness that only the
4-bit bytes streamed; (f) mode 2 leaves such a prefill bit-identical to bf16; (g) greedy and 5-beam ids against a twin engine that
holds the dequantised weights as bf16; (h) ``release_bf16``: memory falls, every output is bit-identical, the other modes refuse.
"""
import pytest
import torch

from tests import tiny
from tests.fp4_common import BF16, _case, _gemv_profile, _tiny_model, bfr, rel_err, tiny_fp4  # noqa: F401 (tiny_fp4: the fixture)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ (a) decode, exhaustive
def _exhaustive(scale_bytes):
    """Row n: code n % 16 at position n // 16 of EVERY block (the other positions hold position-dependent codes); one block per
    scale byte.  Returns the host dequantisation [N, K] and the device output [K, N] for all K one-hot rows fed in ONE call."""
    from emu_amd import mxfp4, ops
    K = 32 * len(scale_bytes)
    N = 16 * 32
    codes = torch.empty(N, K, dtype=torch.uint8)
    pos = torch.arange(K) % 32
    for n in range(N):
        c, p = n % 16, n // 16
        codes[n] = ((pos * 5 + 3 + n) % 16).to(torch.uint8)
        codes[n, pos == p] = c
    scales = torch.tensor(scale_bytes, dtype=torch.uint8).repeat(N, 1)
    # 4 * 2^126, 6 * 2^126 and 2 * 2^127 upwards exceed the largest fp32 / bf16 number: under scale bytes 253 and 254 the host value
    # of those codes is inf, and one inf anywhere in a weight row turns every other output of that row into 0 * inf = NaN in ANY dot
    # product.  Codes whose product is not a number keep their sign and fall back to magnitude 0 / 0.5 in those blocks, so every
    # byte, every position and every code whose product exists is still checked exactly.
    over = ~torch.isfinite(mxfp4.dequantize(mxfp4.pack_codes(codes), scales))
    codes[over] &= 0b1001
    packed = mxfp4.pack_codes(codes)
    want = mxfp4.dequantize(packed, scales)
    assert bool(torch.isfinite(want).all()) and torch.equal(want.to(BF16).float(), want)
    assert bool((over.reshape(N, -1, 32).any(-1).any(0) == (torch.tensor(scale_bytes) >= 253)).all())
    eye = torch.eye(K, dtype=BF16).cuda()
    got = ops.linear_fp4w_gemm(eye, packed.cuda(), scales.cuda()).float().cpu()
    return want, got


def test_decode_exhaustive_gemm():
    """All 16 codes in every nibble and byte position of a block under 16 scale bytes whose products are all normal bf16 numbers.
    All K = 512 one-hot rows go in ONE call (M = 512: four row tiles of the 128-row form, both stages, every k position), so every
    output is a single product through v_cvt_scalef32_pk_bf16_fp4 and the MFMA and must equal the host dequantisation exactly."""
    want, got = _exhaustive([3, 4, 60, 100, 125, 126, 127, 128, 129, 150, 200, 250, 251, 252, 253, 254])
    assert want.shape[1] == 512 and got.shape == (512, 512)
    assert bool((want.abs()[want != 0] >= 2.0 ** -126).all())                   # every product is a normal bf16 number
    assert torch.equal(got, want.t())


def test_decode_denormal_products_gemm():
    """Scale bytes 1 and 2: products of magnitude 2^-127 .. 2^-126 * 0.75 are bf16 denormals.  Each output must equal the host
    value or be a zero of the right sign; the other scale bytes are normal and must be exact (the rule of
    tests/test_gpu_fp4_wide.py::test_decode_denormal_products).  All K = 256 one-hot rows in ONE call: two row tiles, one stage."""
    want, got = _exhaustive([1, 2, 127, 128, 129, 150, 200, 250])
    assert got.shape == (256, 512)
    want = want.t()
    exact = got == want
    flushed = (got == 0) & (torch.signbit(got) == torch.signbit(want))
    denorm = (want != 0) & (want.abs() < 2.0 ** -126)
    print(f"bf16-denormal products: {int(denorm.sum())}, exact {int((exact & denorm).sum())}, flushed to signed zero {int((flushed & denorm & ~exact).sum())}")
    assert bool((exact | (flushed & denorm)).all())
    assert bool(exact[~denorm].all())


# ------------------------------------------------------------------------------------------------ (b) linear parity
def _differs_from_bf16_gemm(x, wd, got, **kw):
    """Share of elements that differ from ``ops.linear`` on the dequantised weights; printed only.  nan where the bf16 GEMM does not
    take the shape (its SwiGLU epilogue refuses narrow N)."""
    from emu_amd import ops
    from emu_amd._lib import EmuHipError
    try:
        ref = ops.linear(x.cuda(), wd.to(BF16).cuda(), **kw)
    except EmuHipError:
        return float("nan")
    return float((ref != got).float().mean())


# 17: one over the thin limit; 31 / 32 / 33, 64 / 65 and 129: both sides of the 32-, 64- and 128-row tiles; 300: three row tiles, ragged
@pytest.mark.parametrize("M", [17, 31, 32, 33, 64, 65, 129, 300])
@pytest.mark.parametrize("N,K", [(16, 256), (37, 512), (1000, 6656), (64, 17920)])
def test_linear_fp4w_gemm_plain_and_resid(M, N, K):
    from emu_amd import ops
    q, sc, wd = _case(N, K)
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(BF16)
    res = torch.randn(M, N, generator=g).to(BF16)
    want = bfr(x.float() @ wd.T)
    got = ops.linear_fp4w_gemm(x.cuda(), q, sc)
    e1 = rel_err(got, want)
    d1 = _differs_from_bf16_gemm(x, wd, got)
    got = ops.linear_fp4w_gemm(x.cuda(), q, sc, res=res.cuda(), epi=ops.EPI_RESID)
    e2 = rel_err(got, bfr(want + res.float()))
    print(f"fp4 gemm M={M} N={N} K={K}: rel L2 plain {e1:.2e} resid {e2:.2e}; elements differing from the bf16 GEMM {d1:.4f}")
    assert e1 < 4e-3
    assert e2 < 4e-3


def test_linear_fp4w_gemm_bias():
    from emu_amd import ops
    N, K, M = 300, 512, 40
    q, sc, wd = _case(N, K)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, K, generator=g).to(BF16)
    bias = torch.randn(N, generator=g).to(BF16)
    want = bfr(x.float() @ wd.T + bias.float())
    assert rel_err(ops.linear_fp4w_gemm(x.cuda(), q, sc, bias=bias.cuda()), want) < 4e-3


@pytest.mark.parametrize("M", [17, 130])
@pytest.mark.parametrize("N,K", [(38, 512), (2240, 6656)])
def test_linear_fp4w_gemm_swiglu(M, N, K):
    from emu_amd import ops
    q, sc, wd = _case(N, K, 1)
    g = torch.Generator().manual_seed(11 + M + N)
    x = torch.randn(M, K, generator=g).to(BF16)
    y = bfr(x.float() @ wd.T)
    want = bfr(bfr(torch.nn.functional.silu(y[:, 0::2])) * y[:, 1::2])          # packed rows interleave gate / up
    got = ops.linear_fp4w_gemm(x.cuda(), q, sc, epi=ops.EPI_SWIGLU)
    assert got.shape == (M, N // 2)
    e = rel_err(got, want)
    d = _differs_from_bf16_gemm(x, wd, got, epi=ops.EPI_SWIGLU)
    print(f"fp4 gemm SwiGLU M={M} N={N} K={K}: rel L2 {e:.2e}; elements differing from the bf16 GEMM {d:.4f}")
    assert e < 8e-3


# ------------------------------------------------------------------------------------------------ (d) rejections
def test_fp4_gemm_rejections():
    from emu_amd import ops
    from emu_amd._lib import EmuHipError, lib

    def args(M, N, K):
        return (torch.zeros(M, K, dtype=BF16, device="cuda"), torch.zeros(N, K // 2, dtype=torch.uint8, device="cuda"),
                torch.full((N, K // 32), 127, dtype=torch.uint8, device="cuda"))
    ops.linear_fp4w_gemm(*args(17, 64, 256))
    with pytest.raises(EmuHipError):
        ops.linear_fp4w_gemm(*args(16, 64, 256))
    with pytest.raises(EmuHipError):
        ops.linear_fp4w_gemm(*args(20, 64, 384))
    with pytest.raises(EmuHipError):
        ops.linear_fp4w_gemm(*args(20, 63, 256), epi=ops.EPI_SWIGLU)
    with pytest.raises(EmuHipError):
        ops.linear_fp4w_gemm(*args(20, 64, 256), epi=ops.EPI_RESID)              # residual epilogue without res
    # through the C ABI: a misaligned activation / weight pointer, and a scale stride that is no multiple of 4
    M, N, K = 20, 64, 256
    x, q, sc = args(M + 1, N + 1, K)
    out = torch.empty(M, N, dtype=BF16, device="cuda")
    sc6 = torch.full((N, 6), 127, dtype=torch.uint8, device="cuda")            # K / 32 = 8 scale bytes needed, stride 6

    def call(xp, qp, sp, lds):
        return lib().emu_linear_fp4w_gemm_bf16(xp, qp, sp, None, None, out.data_ptr(), M, N, K, K, K // 2, lds, 0, N, ops.EPI_NONE,
                                               ops.stream(out))
    assert call(x.data_ptr(), q.data_ptr(), sc.data_ptr(), K // 32) == 0
    assert call(x.data_ptr() + 2, q.data_ptr(), sc.data_ptr(), K // 32) == -22
    assert call(x.data_ptr(), q.data_ptr() + 8, sc.data_ptr(), K // 32) == -22
    assert call(x.data_ptr(), q.data_ptr(), sc.data_ptr() + 2, K // 32) == -22
    assert call(x.data_ptr(), q.data_ptr(), sc6.data_ptr(), 6) == -22
    assert call(x.data_ptr(), q.data_ptr(), sc.data_ptr(), 10) == -22          # wide enough, but lds % 4 != 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ engine
def _prefill_inputs(B, S, hidden, pad, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, S, hidden, generator=g) * 0.5).to(BF16)
    mask = torch.ones(B, S, dtype=torch.long)
    if pad:
        mask[1, :pad] = 0                                                        # left padding on row 1
    return x, mask


@pytest.mark.parametrize("B,pad", [(1, 0), (2, 7)])
def test_fp4_all_rows_prefill_matches_oracle_and_streams_the_4bit_set(tiny_fp4, B, pad):     # (e)
    """A prefill of 24 / 48 rows in mode 3 == the oracle's prefill on the dequantised weights (padded rows are don't-care), logits
    of ALL rows through the 4-bit head included.  The weight-stream profiler, which counts the bf16 few-row streams, the 4-bit
    streams and the 4-bit GEMM but no bf16 GEMM, saw one launch per matrix and exactly the 4-bit bytes: no projection ran on bf16."""
    from emu_amd import mxfp4
    from oracle import emu2_ref as R
    m, W, W4, cfg = tiny_fp4
    lm = m.decoder.lm
    S = 24
    x, mask = _prefill_inputs(B, S, cfg.llama.hidden, pad, 21 + B)
    want = R.llama_model(x.float(), mask, R.cast_weights(W4, torch.float32), cfg.llama, final_norm=False)
    out = {}

    def run():
        out["h"], _, _ = lm.prefill(x.cuda(), mask)
        out["l"] = lm.logits(out["h"].reshape(B * S, -1).contiguous())
    mats = [lm._keep[f"{i}.{k}"] for i in range(cfg.llama.layers) for k in lm._FP4_KINDS] + [lm.lm_head]
    try:
        lm.use_fp4(True, wide=True, all_rows=True)
        assert lm.fp4_all and lm.fp4_wide and lm.fp4_decode
        fp4_bytes = lm.weight_bytes_per_token()
        wb, nl = _gemv_profile(run)
    finally:
        lm.use_fp4(False)
    assert not lm.fp4_all
    ok = mask.bool()
    e_h = rel_err(out["h"].cpu()[ok], want[ok])
    h = R.rms_norm(want, W["decoder.lm.model.norm.weight"].float(), cfg.llama.rms_eps)
    wl = h @ W4["decoder.lm.lm_head.weight"].T
    e_l = rel_err(out["l"].view(B, S, -1).cpu()[ok], wl[ok])
    print(f"fp4 mode 3 prefill B={B} vs oracle: hidden {e_h:.2e}, logits {e_l:.2e}; profiler {wb:.0f} bytes in {nl} launches")
    assert e_h < 2e-2
    assert e_l < 2.5e-2
    assert fp4_bytes == sum(t.shape[0] * mxfp4.bytes_per_row(t.shape[1]) for t in mats)
    assert wb == fp4_bytes and nl == len(mats)
    assert wb != sum(t.numel() * 2 for t in mats)


def test_fp4_mode_2_leaves_the_prefill_on_bf16(tiny_fp4):                                    # (f)
    """In mode 2 the same 24-row prefill (and its logits) is bit-identical to an engine that never enabled fp4."""
    m, W, W4, cfg = tiny_fp4
    lm = m.decoder.lm
    x, mask = _prefill_inputs(1, 24, cfg.llama.hidden, 0, 22)

    def run():
        h, _, _ = lm.prefill(x.cuda(), mask)
        return h.cpu(), lm.logits(h.reshape(24, -1).contiguous()).cpu()
    h0, l0 = run()
    try:
        lm.use_fp4(True, wide=True)
        assert not getattr(lm, "fp4_all", False)
        h1, l1 = run()
    finally:
        lm.use_fp4(False)
    assert torch.equal(h0, h1) and torch.equal(l0, l1)


def test_fp4_all_rows_equals_twin_engine(tiny_fp4, golden_dir):                              # (g)
    """Mode 3 against a twin engine that holds the dequantised weights as bf16 and runs the bf16 kernels: both see the same weights
    at every row count.  A row whose ids differ from the twin's is EXCLUDED, and only where the existing screens allow it: greedy, the
    twin's top-2 logit margin at the first divergence is below 0.08 (tests/test_gpu_fp4.py::
    test_fp4_greedy_equals_twin_engine_graph_equals_eager); 5 beams, the twin's gap between the two continuations' accumulated
    scores is below 0.08 (tests/test_gpu_fp4_wide.py::test_fp4_wide_beam_search_equals_twin_engine).  The same engine, prompts and
    twin are also run the way those two tests run them (greedy in mode 1, beams in mode 2, bf16 prefill), their excluded rows are
    counted by the same screens, and mode 3 may exclude at most as many rows as they do, greedy and beams each.
    The 20-row step is a beam step: four prompts (one left-padded) are prefilled, their cache is fanned out to 4 x 5 beam rows that
    share the prompt's slots (``fan_out_kv``), and one step of 20 rows -- the case that fell back to bf16 in mode 2 -- is compared
    with the twin's on hidden states, none excluded."""
    from emu_amd import EmuModel, TextDecoderCfg
    from oracle import emu2_ref as R
    m, W, W4, cfg = tiny_fp4
    z = tiny.load(golden_dir, "generate_tiny.npz")
    v, l, vocab, _ = tiny.weights_from(z)
    ids, mask = torch.from_numpy(z["ids2"]), torch.from_numpy(z["mask2"])
    n_new, (B, S) = 6, ids.shape
    m4 = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda")
    m4.load_state_dict(W4, strict=True)
    twin = EmuModel(v, TextDecoderCfg(instruct=True), llama_cfg=l, device="cuda")
    twin.load_state_dict(W4, strict=True)
    lm4, tl = m4.decoder.lm, twin.decoder.lm
    kw_g = dict(max_new_tokens=n_new, stop_on_eos=False)
    kw_b = dict(max_new_tokens=n_new, num_beams=5, hf_semantics="5.x")
    P, NB, S20 = 4, 5, 24
    x4, mask4 = _prefill_inputs(P, S20, cfg.llama.hidden, 3, 23)
    g = torch.Generator().manual_seed(26)
    step_in = (torch.randn(P * NB, cfg.llama.hidden, generator=g) * 0.5).to(BF16).cuda()     # 20 different tokens, one per beam

    def step20(e):
        s_max = e.kv_capacity(S20 + 1)
        _, kstart, pos = e.prefill(x4.cuda(), mask4, s_max)
        e.fan_out_kv(P, NB, S20, s_max)
        try:
            return e.decode_embeds(step_in, pos.repeat_interleave(NB).contiguous(), S20, kstart.repeat_interleave(NB).contiguous()).cpu()
        finally:
            e.set_kv_share(0, 0)

    def ids_in_mode(kw, **mode):
        try:
            lm4.use_fp4(True, **mode)
            return m4.generate_ids(ids, mask, None, **kw).cpu()
        finally:
            lm4.use_fp4(False)
    ref_g = ids_in_mode(kw_g)                                                    # the existing greedy twin test's mode
    ref_b = ids_in_mode(kw_b, wide=True)                                         # the existing beam twin test's mode
    try:
        lm4.use_fp4(True, wide=True, all_rows=True)
        got_g = m4.generate_ids(ids, mask, None, **kw_g).cpu()
        got_b = m4.generate_ids(ids, mask, None, **kw_b).cpu()
        again_b = m4.generate_ids(ids, mask, None, **kw_b).cpu()
        got_20 = step20(lm4)
    finally:
        lm4.use_fp4(False)
    assert got_b.tolist() == again_b.tolist()
    # ---- greedy: the twin's ids, and its logits along them (teacher-forced with its own ids) for the top-2 margins
    want_g = twin.generate_ids(ids, mask, None, **kw_g).cpu()
    x = twin._prompt_embeds(ids, None, twin.n_query)
    hidden, kstart, pos = tl.prefill(x.view(B, S, -1), mask)
    logits = [tl.logits(hidden[:, -1, :].contiguous()).float().cpu()]
    for i in range(n_new - 1):
        e = tl.embed_tokens(want_g[:, i:i + 1].cuda()).view(B, -1)
        logits.append(tl.logits(tl.decode_embeds(e, pos + i, S + i, kstart)).float().cpu())

    def greedy_excluded(got, what):
        rows = []
        for b in range(B):
            for i in range(n_new):
                if int(got[b, i]) != int(want_g[b, i]):
                    row = logits[i][b].clone()
                    if i < 1:
                        row[R.EOS_ID] = -float("inf")
                    t2 = row.topk(2)
                    assert int(t2.indices[0]) == int(want_g[b, i])
                    margin = float(t2.values[0] - t2.values[1])
                    assert margin < 0.08, f"{what}: greedy row {b} diverged from the twin at step {i} with top-2 margin {margin:.3f}"
                    rows.append(b)
                    break
        return rows
    # ---- 5 beams
    want_b = twin.generate_ids(ids, mask, None, **kw_b).cpu()

    def beam_excluded(got, what):
        rows = []
        for b in range(B):
            if got[b].tolist() == want_b[b].tolist():
                continue
            i = next(j for j in range(n_new) if int(got[b, j]) != int(want_b[b, j]))

            def score(seq):                      # the twin's accumulated log-probabilities up to and including step i, teacher-forced
                xb = twin._prompt_embeds(ids[b:b + 1], None, twin.n_query)
                hid, ks, ps = tl.prefill(xb.view(1, S, -1), mask[b:b + 1])
                lp = torch.log_softmax(tl.logits(hid[:, -1, :].contiguous()).float(), -1)
                tot = float(lp[0, int(seq[0])])
                for j in range(i):
                    e = tl.embed_tokens(seq[j:j + 1][None].cuda()).view(1, -1)
                    lp = torch.log_softmax(tl.logits(tl.decode_embeds(e, ps + j, S + j, ks)).float(), -1)
                    tot += float(lp[0, int(seq[j + 1])])
                return tot
            gap = abs(score(want_b[b]) - score(got[b]))
            assert gap < 0.08, f"{what}: beam row {b} diverged from the twin at step {i}; the twin's gap between the two candidates is {gap:.3f}"
            rows.append(b)
        return rows
    ex_g3, ex_g1 = greedy_excluded(got_g, "mode 3"), greedy_excluded(ref_g, "mode 1")
    ex_b3, ex_b2 = beam_excluded(got_b, "mode 3"), beam_excluded(ref_b, "mode 2")
    print(f"fp4 mode 3 vs the twin engine, excluded rows of {B}: greedy {ex_g3} (mode 1: {ex_g1}), 5 beams {ex_b3} (mode 2: {ex_b2})")
    assert len(ex_g3) <= len(ex_g1), f"greedy: mode 3 excludes rows {ex_g3}, the existing twin screen only {ex_g1}"
    assert len(ex_b3) <= len(ex_b2), f"5 beams: mode 3 excludes rows {ex_b3}, the existing twin screen only {ex_b2}"
    # ---- 20 rows: a prefill of 4 x 24 rows and one step of 4 x 5 beam rows on the shared-prefix cache, both on the 4-bit GEMM
    e20 = rel_err(got_20, step20(tl))
    print(f"fp4 mode 3, 20-row beam step (4 prompts x 5 beams) vs the twin engine: hidden {e20:.2e}")
    assert e20 < 2e-2


def test_fp4_all_rows_head_shard_equals_whole_head(golden_dir):                              # mode 3 on a vocabulary-sharded head
    """emu_llama_set_head_shard on a single-rank context, as tests/test_gpu_fp4_wide.py::test_fp4_wide_head_shard_equals_whole_head
    does for mode 2: the engine is handed rows [r0, r1) of lm_head and of its 4-bit copy; the 20-row and the 70-row mode-3 logits of
    those columns (the single-tile and the prefill form of the 4-bit GEMM, writing at a column offset that is not 8-byte aligned)
    equal the unsharded mode-3 logits bit for bit, every other column is zero, and the profiler saw the shard's 4-bit bytes."""
    from emu_amd import mxfp4
    from emu_amd._lib import check, lib
    m, *_ = _tiny_model(golden_dir)
    lm = m.decoder.lm
    g = torch.Generator().manual_seed(4)
    hid = (torch.randn(70, lm.cfg.hidden_size, generator=g) * 0.5).to(BF16).cuda()
    r0, r1 = 4101, 4101 + 8075                                                   # a ragged slice of the vocabulary at an odd column
    lm.use_fp4(True, wide=True, all_rows=True)
    try:
        whole = {M: lm.logits(hid[:M]).cpu() for M in (20, 70)}
        head = lm.lm_head[r0:r1].contiguous()
        q, sc = (t[r0:r1].contiguous() for t in lm._fp4["lm_head"])
        h = lm.handle
        check(lib().emu_llama_set_head(h, lm.final_norm.data_ptr(), head.data_ptr(), lm.embed.data_ptr(), lm.cos.data_ptr(),
                                       lm.sin.data_ptr()), "emu_llama_set_head")
        check(lib().emu_llama_set_head_fp4(h, q.data_ptr(), sc.data_ptr()), "emu_llama_set_head_fp4", lm.ctx.handle)
        check(lib().emu_llama_set_head_shard(h, r0, r1 - r0), "emu_llama_set_head_shard", lm.ctx.handle)
        shard, seen = {}, {}
        for M in (20, 70):
            out = {}
            seen[M] = _gemv_profile(lambda: out.update(l=lm.logits(hid[:M])))
            shard[M] = out["l"].cpu()
    finally:
        check(lib().emu_llama_set_head_shard(lm.handle, 0, -1), "emu_llama_set_head_shard", lm.ctx.handle)
        check(lib().emu_llama_set_head(lm.handle, lm.final_norm.data_ptr(), lm.lm_head.data_ptr(), lm.embed.data_ptr(),
                                       lm.cos.data_ptr(), lm.sin.data_ptr()), "emu_llama_set_head")
        lm._fp4_register("lm_head")
        lm.use_fp4(False)
    for M in (20, 70):
        assert seen[M] == ((r1 - r0) * mxfp4.bytes_per_row(lm.cfg.hidden_size), 1)
        assert torch.equal(shard[M][:, r0:r1], whole[M][:, r0:r1])
        assert not bool(shard[M][:, :r0].any()) and not bool(shard[M][:, r1:].any())


def test_release_bf16(golden_dir):                                                           # (h)
    """``release_bf16`` frees the bf16 matrices and changes nothing that runs: the same kernels read the same 4-bit pointers."""
    from emu_amd._lib import EmuHipError
    m, v, l, vocab, W = _tiny_model(golden_dir)
    lm = m.decoder.lm
    z = tiny.load(golden_dir, "generate_tiny.npz")
    ids, mask = torch.from_numpy(z["ids2"]), torch.from_numpy(z["mask2"])
    x, xmask = _prefill_inputs(1, 24, lm.cfg.hidden_size, 0, 24)
    x5, mask5 = _prefill_inputs(5, 25, lm.cfg.hidden_size, 0, 25)
    with pytest.raises(RuntimeError, match="all_rows"):
        lm.release_bf16()                                                        # needs mode 3
    lm.use_fp4(True, wide=True, all_rows=True)

    def record():
        h, _, _ = lm.prefill(x.cuda(), xmask)
        lg = lm.logits(h.reshape(24, -1).contiguous())
        m.use_graph = False
        eager = m.generate_ids(ids, mask, None, max_new_tokens=6, stop_on_eos=False).cpu()
        m.use_graph = True
        graph = m.generate_ids(ids, mask, None, max_new_tokens=6, stop_on_eos=False).cpu()
        _, kstart, pos = lm.prefill(x5[:, :24].contiguous().cuda(), mask5[:, :24])
        h5 = lm.decode_embeds(x5[:, 24].contiguous().cuda(), pos, 24, kstart)    # the five rows of a 5-beam step
        l5 = lm.logits(h5)
        beams = m.generate_ids(ids, mask, None, max_new_tokens=4, num_beams=5, hf_semantics="5.x").cpu()
        return h.cpu(), lg.cpu(), eager, graph, h5.cpu(), l5.cpu(), beams
    before = record()
    assert before[2].tolist() == before[3].tolist()
    bytes_4bit = lm.weight_bytes_per_token()
    released = sum(t.numel() * 2 for k, t in lm._keep.items() if k.split(".")[1] in lm._FP4_KINDS) + lm.lm_head.numel() * 2
    head_shape = tuple(lm.lm_head.shape)
    torch.cuda.synchronize()
    mem0 = torch.cuda.memory_allocated()
    lm.release_bf16()
    torch.cuda.synchronize()
    mem1 = torch.cuda.memory_allocated()
    print(f"release_bf16: {released} bytes of bf16 matrices, memory_allocated fell by {mem0 - mem1}")
    assert mem0 - mem1 >= released
    assert lm.lm_head is None and not any(k.split(".")[1] in lm._FP4_KINDS for k in lm._keep) and lm.ready
    assert lm.weight_bytes_per_token() == bytes_4bit
    assert tuple(lm._fp4_source("lm_head").shape) == head_shape and tuple(lm.fp4_dequantized("lm_head").shape) == head_shape
    with pytest.raises(ValueError, match="must be uint8"):                       # load_fp4 still checks shapes, now against the 4-bit tensors
        lm.load_fp4("lm_head", torch.zeros(3, 3, dtype=torch.uint8), torch.zeros(3, 1, dtype=torch.uint8))
    for refused in (lambda: lm.use_fp4(False), lambda: lm.use_fp4(True), lambda: lm.use_fp4(True, wide=True), lambda: lm.use_fp8(),
                    lambda: lm.set_decode_fused(1)):
        with pytest.raises(EmuHipError, match="release"):
            refused()
    with pytest.raises(RuntimeError, match="release_bf16"):                      # a direct call says what happened, no KeyError
        lm.quantize_fp8()
    assert lm.fp4_all and lm.fp4_decode and not getattr(lm, "fp8_decode", False) and lm.decode_fused == 0
    after = record()                                                             # still runs: prefill, logits, eager and graph greedy, beams
    assert after[2].tolist() == after[3].tolist()
    for a, b in zip(before, after):
        assert torch.equal(a, b)
