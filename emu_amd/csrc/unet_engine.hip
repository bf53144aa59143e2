// UNet denoise engine: the C ABI ``emu_unet_*`` (include/emu_hip.h).
//
// One call = one full denoise step of EmuVisualGeneration's loop (Emu2/emu/diffusion.py:130-149):
//   cat([latents]*2) -> scale_model_input -> UNet2DConditionModel (SDXL topology, conf/diffusion_config/unet/
//   config.json:1-72) -> chunk (cond, uncond) -> classifier-free guidance -> EulerDiscreteScheduler.step,
// as ~900 launches on one stream with no allocation or synchronisation (hipGraph-capturable; per-step inputs --
// timestep embedding row, sigma -- are read from device tables through a device-side step counter).
// Activations are NHWC ([B*H*W, C] bf16), so every 1x1 conv / Linear is a plain GEMM, 3x3 convs are implicit GEMMs
// (gemm.hip CONV mode, nearest-x2 upsample and stride 2 folded into the gather), and Transformer2D needs no permute.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/emu_hip.h"
#include "kernels.h"

struct emu_ctx;
int emu_ctx_fail(emu_ctx* c, int code, const char* what);      // engine.hip

namespace {
inline hipStream_t S(emu_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
inline const bf16_t* B16(const void* p) { return reinterpret_cast<const bf16_t*>(p); }
inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }
const ConvGeom NOCONV{0, 0, 0, 0, 0, 0};

struct Resnet {
    std::string name;
    int cin, cout, temb_off;
    const bf16_t *n1g, *n1b, *c1w, *c1b, *n2g, *n2b, *c2w, *c2b, *scw, *scb;
};
struct Proj {                       // one matrix of a transformer block and everything registered for it (resolve_proj)
    const bf16_t *w = nullptr, *b = nullptr;        // "<base>.w" [N, K], "<base>.b" (null: the projection has no bias)
    // optional: the LayerNorm in front folded in -- "<base>.wln" = W * gamma, ".c" = its fp32 row sums, ".d" = W @ beta + bias
    const bf16_t* wln = nullptr;
    const float *c = nullptr, *d = nullptr;
    // optional (emu_unet_use_fp8): "<base>.w.fp8" = e4m3 bytes [N, K], ".w.fp8s" = one fp32 scale per output row
    const uint8_t* q = nullptr;
    const float* s = nullptr;
    bool folded() const { return wln && c && d; }
};
struct LnGB { const bf16_t *g, *b; };
struct TBlock {
    Proj qkv, o1, q2, o2, gg, ff;
    LnGB ln1, ln2, ln3;
    const bf16_t* kv2;
    size_t ctx_off;                 // element offset of this block's {K|V rows, Vt} in the context cache
};
struct Transformer {
    std::string name;
    int c, heads, depth;
    const bf16_t *gng, *gnb, *piw, *pib, *pow_, *pob;
    std::vector<TBlock> blocks;
};

// What a transformer's blocks fuse and in which format their six GEMMs run: the one rule, on integers only (no HIP call, no
// global, no engine; exported as emu_unet_block_plan, tests/test_unet_block_plan.py).  fp8 = emu_unet_use_fp8, fusion =
// emu_unet_set_fusion's mask, M = rows (batch elements x HW).  M <= 8 (toy latents) is the GEMV path, which fuses nothing.
struct BlockPlan {
    bool fp8;               // W8A8 GEMMs: whole 128-column k tiles, rows no wider than launch_layernorm_q8 holds
    bool ln_fold;           // bit 0: the LayerNorms live in their consumer GEMMs (statistics slots are 128 columns wide; no fp8 form)
    bool vt_epilogue;       // bit 1: the qkv projection stores V^T itself (whole 64-key groups)
    bool cross_epilogue;    // bit 2: cross-attention inside the to_q epilogue (rows of one tile within one batch element, <= 64 keys)
    bool prefetch;          // every GEMM of the chain names its successor's weights (Fx::pf; the fp8 GEMM has no such argument)
};
BlockPlan unet_block_plan(bool fp8, int fusion, int M, int C, int HW, int n_ctx, int depth) {
    const bool gemm = M > 8, keys64 = HW % 64 == 0;
    const bool f8 = fp8 && gemm && C % 128 == 0 && C <= 2048;
    return {f8, !f8 && (fusion & 1) && gemm && C % 128 == 0, (fusion & 2) && gemm && keys64,
            (fusion & 4) && gemm && keys64 && n_ctx <= 64, !f8 && gemm && depth > 0};
}
}  // namespace

struct emu_unet {
    emu_ctx* ctx;
    emu_unet_cfg cfg;
    float* splitk = nullptr;            // bound to the caller's workspace at every entry (plan_ws)
    size_t splitk_floats = 0;
    std::map<std::string, const bf16_t*> w;
    bool finalized = false;
    int fusion = 0;                     // bit 0: LayerNorm folded into the consumer GEMMs, bit 1: V^T from the qkv epilogue,
                                        // bit 2: cross-attention inside the attn2 to_q epilogue
    int fusion_avail = 0;               // what the registered tensors allow (set by emu_unet_finalize)
    bool fp8 = false;                   // emu_unet_use_fp8: the transformer blocks' GEMMs W8A8 (fusion bit 0 has no fp8 form)
    int cfg_half = -1;                  // emu_unet_set_cfg_half: -1 = the CFG pair (batch 2); 0 / 1 = only the cond / uncond row (a rank pair splits the pair)
    // resolved structure
    const bf16_t *conv_in_w, *conv_in_b, *te1w, *te1b, *te2w, *te2b, *ae1w, *ae1b, *ae2w, *ae2b, *tpw, *tpb;
    const bf16_t *cno_g, *cno_b, *cout_w, *cout_b;
    std::vector<Resnet> down_res[3], up_res[3];
    std::vector<Transformer> down_tr[3], up_tr[3];
    const bf16_t *down_ds_w[3] = {}, *down_ds_b[3] = {}, *up_us_w[3] = {}, *up_us_b[3] = {};
    Resnet mid_res[2];
    Transformer mid_tr;
    int temb_total = 0;
    size_t ctx_elems = 0;
    int n_ctx = 0;
    const bf16_t* ctx_cache = nullptr;
    const bf16_t* aug_emb = nullptr;
    std::string err;
};

namespace {

int ufail(emu_unet* u, int code, const std::string& what) {
    u->err = what;
    return emu_ctx_fail(u->ctx, code, u->err.c_str());
}
#define UTRY(expr) do { int st__ = (expr); if (st__ != 0) return ufail(u, st__, #expr); } while (0)
#define UPASS(expr) do { int st__ = (expr); if (st__ != 0) return st__; } while (0)     // the callee has recorded the failure

const bf16_t* find(emu_unet* u, const std::string& k, bool required, bool* ok) {
    auto it = u->w.find(k);
    if (it == u->w.end()) {
        if (required) { *ok = false; u->err = "emu_unet_finalize: missing weight '" + k + "'"; }
        return nullptr;
    }
    return it->second;
}

void resolve_resnet(emu_unet* u, Resnet& r, bool* ok) {
    const std::string& p = r.name;
    r.n1g = find(u, p + "norm1.g", true, ok); r.n1b = find(u, p + "norm1.b", true, ok);
    r.c1w = find(u, p + "conv1.w", true, ok); r.c1b = find(u, p + "conv1.b", true, ok);
    r.n2g = find(u, p + "norm2.g", true, ok); r.n2b = find(u, p + "norm2.b", true, ok);
    r.c2w = find(u, p + "conv2.w", true, ok); r.c2b = find(u, p + "conv2.b", true, ok);
    const bool sc = r.cin != r.cout;
    r.scw = find(u, p + "shortcut.w", sc, ok); r.scb = find(u, p + "shortcut.b", sc, ok);
}

// One block matrix from its registered names: "<base>.w" and, with `bias`, "<base>.b" are required; the LayerNorm fold
// "<base>.wln" / ".c" / ".d" is optional (fusion_avail bit 0); the e4m3 copy "<base>.w.fp8" / ".w.fp8s" is required with `fp8`.
Proj resolve_proj(emu_unet* u, const std::string& base, bool bias, bool fp8, bool* ok) {
    Proj p;
    p.w = find(u, base + ".w", true, ok);
    if (bias) p.b = find(u, base + ".b", true, ok);
    p.wln = find(u, base + ".wln", false, ok);
    p.c = reinterpret_cast<const float*>(find(u, base + ".c", false, ok));
    p.d = reinterpret_cast<const float*>(find(u, base + ".d", false, ok));
    p.q = reinterpret_cast<const uint8_t*>(find(u, base + ".w.fp8", fp8, ok));
    p.s = reinterpret_cast<const float*>(find(u, base + ".w.fp8s", fp8, ok));
    return p;
}

// the six matrices of block `b` ("<transformer>transformer_blocks.<k>."): emu_unet_finalize (fp8 = false) and emu_unet_use_fp8
void resolve_block(emu_unet* u, TBlock& tb, const std::string& b, bool fp8, bool* ok) {
    tb.qkv = resolve_proj(u, b + "attn1.qkv", false, fp8, ok); tb.o1 = resolve_proj(u, b + "attn1.out", true, fp8, ok);
    tb.q2 = resolve_proj(u, b + "attn2.q", false, fp8, ok); tb.o2 = resolve_proj(u, b + "attn2.out", true, fp8, ok);
    tb.gg = resolve_proj(u, b + "ff.geglu", true, fp8, ok); tb.ff = resolve_proj(u, b + "ff.out", true, fp8, ok);
}

void resolve_transformer(emu_unet* u, Transformer& t, bool* ok) {
    const std::string& p = t.name;
    t.gng = find(u, p + "norm.g", true, ok); t.gnb = find(u, p + "norm.b", true, ok);
    t.piw = find(u, p + "proj_in.w", true, ok); t.pib = find(u, p + "proj_in.b", true, ok);
    t.pow_ = find(u, p + "proj_out.w", true, ok); t.pob = find(u, p + "proj_out.b", true, ok);
    t.blocks.resize(t.depth);
    for (int k = 0; k < t.depth; ++k) {
        const std::string b = p + "transformer_blocks." + std::to_string(k) + ".";
        TBlock& tb = t.blocks[k];
        tb.ln1 = {find(u, b + "norm1.g", true, ok), find(u, b + "norm1.b", true, ok)};
        tb.ln2 = {find(u, b + "norm2.g", true, ok), find(u, b + "norm2.b", true, ok)};
        tb.ln3 = {find(u, b + "norm3.g", true, ok), find(u, b + "norm3.b", true, ok)};
        tb.kv2 = find(u, b + "attn2.kv.w", true, ok);
        resolve_block(u, tb, b, false, ok);
        if (!(tb.qkv.folded() && tb.q2.folded() && tb.gg.folded())) u->fusion_avail &= ~1;
    }
}

// f(transformer) -> status over every transformer in traversal order (down, mid, up: the order of the context cache); stops at a failure
template <class U, class F> int each_transformer(U* u, F&& f) {
    for (int i = 0; i < 3; ++i) for (auto& t : u->down_tr[i]) UPASS(f(t));
    UPASS(f(u->mid_tr));
    for (int i = 0; i < 3; ++i) for (auto& t : u->up_tr[i]) UPASS(f(t));
    return 0;
}

// ---------------------------------------------------------------- workspace plan
struct Ws {
    bf16_t *colin, *hA, *hB, *cat, *gn, *t1, *sc, *tokA, *tokB, *ln, *qkv, *vt, *att, *q2, *ff;
    bf16_t* skip[12];
    bf16_t *temb_in, *e1, *emb, *semb, *temb_all, *add1;
    uint8_t* x8;            // emu_unet_use_fp8: the current GEMM's activation rows as e4m3 bytes ...
    float* xs;              // ... and their per-row scales
    float* lnstats;         // per-row partial (sum, sum of squares) of the transformer stream, one pair per 128-column slot
    float* gnws;
    float* splitk;          // fp32 K-slices of the split-K GEMMs / convs of the lowest-resolution level
    size_t splitk_floats;
    size_t total;
};

Ws plan_ws(const emu_unet* u, int H, int W, void* base) {
    const emu_unet_cfg& c = u->cfg;
    const int Bn = 2;
    char* p = reinterpret_cast<char*>(base);
    size_t off = 0;
    auto take = [&](size_t elems, size_t esz = 2) { char* r = p ? p + off : nullptr; off += align_up(elems * esz); return r; };
    const size_t hw[3] = {(size_t)H * W, (size_t)((H + 1) / 2) * ((W + 1) / 2), (size_t)((H + 3) / 4) * ((W + 3) / 4)};
    size_t max_h = 0, max_cat = 0, max_tok = 0, max_qkv = 0, max_ff = 0, max_vt = 0, max_st = 0;
    for (int i = 0; i < 3; ++i) {
        max_h = std::max(max_h, Bn * hw[i] * c.ch[i]);
        // widest concat at level i: up block (2-i) first resnet input = ch[i] (or ch[i+1]) + skip
        const int wide = (i == 2) ? 2 * c.ch[2] : c.ch[i + 1] + c.ch[i];
        max_cat = std::max(max_cat, Bn * hw[i] * (size_t)wide);
        if (c.attn[i]) {
            max_tok = std::max(max_tok, Bn * hw[i] * c.ch[i]);
            max_qkv = std::max(max_qkv, Bn * hw[i] * 3 * c.ch[i]);
            max_ff = std::max(max_ff, Bn * hw[i] * 4 * c.ch[i]);
            max_vt = std::max(max_vt, (size_t)Bn * c.ch[i] * ((hw[i] + 63) / 64 * 64));
            max_st = std::max(max_st, (size_t)Bn * hw[i] * ((c.ch[i] + 127) / 128) * 2);
        }
    }
    // a downsampled/upsampled tensor is written at the next level's size with the previous level's channels
    max_h = std::max(max_h, Bn * hw[0] * (size_t)c.ch[1]);        // upsampler output of up block 1: [B, hw0, ch1]
    max_h = std::max(max_h, Bn * hw[1] * (size_t)c.ch[2]);        // upsampler output of up block 0: [B, hw1, ch2]
    Ws w;
    w.colin = (bf16_t*)take(Bn * hw[0] * c.kpad_in);
    w.hA = (bf16_t*)take(max_h); w.hB = (bf16_t*)take(max_h);
    w.cat = (bf16_t*)take(max_cat); w.gn = (bf16_t*)take(max_cat);
    w.t1 = (bf16_t*)take(max_h); w.sc = (bf16_t*)take(max_h);
    w.tokA = (bf16_t*)take(max_tok); w.tokB = (bf16_t*)take(max_tok); w.ln = (bf16_t*)take(max_tok);
    w.qkv = (bf16_t*)take(max_qkv); w.vt = (bf16_t*)take(max_vt); w.att = (bf16_t*)take(max_tok);
    w.q2 = (bf16_t*)take(max_tok); w.ff = (bf16_t*)take(max_ff);
    // skip connections: conv_in, then per down block its resnet/attn outputs and its downsampler output
    int k = 0;
    w.skip[k++] = (bf16_t*)take(Bn * hw[0] * c.ch[0]);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < c.layers_per_block; ++j) w.skip[k++] = (bf16_t*)take(Bn * hw[i] * c.ch[i]);
        if (i < 2) w.skip[k++] = (bf16_t*)take(Bn * hw[i + 1] * c.ch[i]);
    }
    w.temb_in = (bf16_t*)take(Bn * c.ch[0]); w.e1 = (bf16_t*)take(Bn * c.temb_dim); w.emb = (bf16_t*)take(Bn * c.temb_dim);
    w.semb = (bf16_t*)take(Bn * c.temb_dim); w.temb_all = (bf16_t*)take((size_t)Bn * u->temb_total);
    w.add1 = (bf16_t*)take(Bn * c.temb_dim);
    w.x8 = (uint8_t*)take(u->fp8 ? max_ff : 0, 1);
    w.xs = (float*)take(u->fp8 ? max_tok : 0, 4);       // (>= rows of any transformer level)
    w.lnstats = (float*)take(max_st, 4);
    w.gnws = (float*)take(gn_ws_floats(Bn, 2 * c.ch[2] > c.ch[1] + c.ch[0] ? 2 * c.ch[2] : c.ch[1] + c.ch[0], (int)hw[0]), 4);
    w.splitk_floats = EMU_SPLITK_SCRATCH_FLOATS;
    w.splitk = (float*)take(w.splitk_floats, 4);
    w.total = off;
    return w;
}

// optional fused epilogues of one GEMM of a transformer block (GemmArgs: row_stats_out / ln_* / vt_*)
struct Fx {
    float* stats_out = nullptr;         // producer: per-row partial sums of the output for the next LayerNorm
    const Proj* ln = nullptr;           // consumer: LayerNorm of A folded in (W = ln->wln), statistics from `stats_in`
    const float* stats_in = nullptr;
    bf16_t* vt = nullptr;               // qkv projection: V heads (columns >= vt_col0) stored key-contiguous
    int vt_col0 = 0, vt_s = 0, vt_spad = 0;
    const bf16_t* cross_k = nullptr;    // attn2 to_q projection: cross-attention over the cached prompt K / V^T in the epilogue
    const bf16_t* cross_vt = nullptr;
    int cross_ldk = 0, cross_n = 0, cross_npad = 0, cross_rows = 0;
    float cross_scale = 0.f;
    const void* pf = nullptr;           // GemmArgs::pf_*: the weight matrix of the GEMM that follows this one on the stream
    size_t pf_bytes = 0;
    bool any() const { return stats_out || ln || vt || cross_k || pf; }
};

// (an all-default Fx leaves the argument block as it was)
void apply_fx(GemmArgs& g, const Fx& fx) {
    g.row_stats_out = fx.stats_out;
    if (fx.ln) {
        g.W = fx.ln->wln; g.bias = nullptr;
        g.ln_c = fx.ln->c; g.ln_d = fx.ln->d; g.ln_stats = fx.stats_in; g.ln_slots = g.K / 128; g.ln_eps = 1e-5f;
    }
    g.vt_out = fx.vt; g.vt_col0 = fx.vt_col0; g.vt_s = fx.vt_s; g.vt_spad = fx.vt_spad;
    g.cross_k = fx.cross_k; g.cross_vt = fx.cross_vt; g.cross_ldk = fx.cross_ldk; g.cross_n = fx.cross_n;
    g.cross_npad = fx.cross_npad; g.cross_rows = fx.cross_rows; g.cross_scale = fx.cross_scale;
    g.pf_ptr = fx.pf; g.pf_bytes = fx.pf_bytes;
}

int gemm(emu_unet* u, const bf16_t* A, const bf16_t* Wt, const bf16_t* bias, const bf16_t* res, bf16_t* C, int M, int N, int K,
         int lda, int ldres, int ldc, int epi, hipStream_t s, const Fx* fx = nullptr) {
    if (M <= 8) {
        if (fx) return -22;
        GemvArgs g{A, Wt, nullptr, bias, res, C, M, N, K, lda, K, ldres, ldc, 0.f, epi, nullptr};
        return launch_gemv(g, s);
    }
    GemmArgs g{A, Wt, bias, res, C, M, N, K, lda, K, ldres, ldc, epi, NOCONV, nullptr, 0, 0};
    if (u) { g.partial = u->splitk; g.partial_floats = u->splitk_floats; }    // primitives (u == null): process scratch
    if (fx) apply_fx(g, *fx);
    return launch_gemm(g, s);
}

int conv3(emu_unet* u, const bf16_t* x, const bf16_t* Wt, const bf16_t* bias, const bf16_t* bias2, int ldb2, const bf16_t* res,
          bf16_t* y, int Bn, int Hin, int Win, int Cin, int Cout, int mode, hipStream_t s) {
    int Ho = Hin, Wo = Win;
    if (mode == CONV_3X3_S2) { Ho = (Hin + 1) / 2; Wo = (Win + 1) / 2; }
    if (mode == CONV_3X3_UP2) { Ho = 2 * Hin; Wo = 2 * Win; }
    GemmArgs g{x, Wt, bias, res, y, Bn * Ho * Wo, Cout, 9 * Cin, 0, 9 * Cin, Cout, Cout, res ? EPI_RESID : EPI_NONE,
               ConvGeom{mode, Hin, Win, Ho, Wo, Cin}, bias2, Ho * Wo, ldb2};
    if (u) { g.partial = u->splitk; g.partial_floats = u->splitk_floats; }    // primitives (u == null): process scratch
    return launch_gemm(g, s);
}

int run_resnet(emu_unet* u, const Resnet& r, const bf16_t* x, bf16_t* out, const Ws& w, int Bn, int H, int W, hipStream_t s) {
    const emu_unet_cfg& c = u->cfg;
    const int HW = H * W, M = Bn * HW;
    UTRY(launch_groupnorm(x, r.n1g, r.n1b, w.gn, w.gnws, Bn, HW, r.cin, c.groups, c.gn_eps, 1, s));
    UTRY(conv3(u, w.gn, r.c1w, r.c1b, w.temb_all + r.temb_off, u->temb_total, nullptr, w.t1, Bn, H, W, r.cin, r.cout, CONV_3X3, s));
    UTRY(launch_groupnorm(w.t1, r.n2g, r.n2b, w.gn, w.gnws, Bn, HW, r.cout, c.groups, c.gn_eps, 1, s));
    const bf16_t* res = x;
    if (r.cin != r.cout) {
        UTRY(gemm(u, x, r.scw, r.scb, nullptr, w.sc, M, r.cout, r.cin, r.cin, 0, r.cout, EPI_NONE, s));
        res = w.sc;
    }
    UTRY(conv3(u, w.gn, r.c2w, r.c2b, nullptr, 0, res, out, Bn, H, W, r.cout, r.cout, CONV_3X3, s));
    return 0;
}

// Transformer2D: GroupNorm -> proj_in -> blocks of {self-attention, cross-attention on the cached prompt K / V^T, GEGLU
// feed-forward}, each behind its LayerNorm and added to the stream -> proj_out + input.  unet_block_plan says once what the blocks
// fuse; nothing else decides a path.
// Fused path (emu_unet_set_fusion): the three LayerNorms of a block live inside their consumer GEMMs -- the producer of the
// stream (proj_in, attn1 / attn2 out-projection, ff-out) emits per-row partial sums from its epilogue, the consumer (qkv,
// attn2 q, GEGLU) multiplies the un-normalised rows by W * gamma and corrects with mean / rstd in its epilogue -- and the qkv
// projection writes V^T itself.  M <= 8 (toy latents) stays on the unfused GEMV path.
// W8A8 mode (emu_unet_use_fp8; not a reference feature): the six GEMMs of a block take fp8 operands.  The three LayerNorms
// run as launches again -- they hold whole rows, so their output leaves as the consumer's fp8 operand with its per-row scale
// for free (launch_layernorm_q8) -- the attention outputs and the GEGLU product are quantised by a launch of their own
// (their rows are spread over the workgroups of the producing kernel); the V^T stores of the qkv projection and the
// cross-attention inside the to_q epilogue (fusion bits 1, 2) work on finished sums and stay available.  proj_in / proj_out,
// the convs and everything outside the transformer blocks stay bf16.
// Successor prefetch (Fx::pf, GemmArgs::pf_*): every GEMM of the chain names the weight matrix of the GEMM behind it (the
// LayerNorm-folded copy where that is the operand); the attention launches in between only widen the lead.  Same-run A/B on the
// true config: 25.07 -> 24.19 ms per denoise step (profiles/r05_prefetch_ab_unet_linear_transformer_chain.log); naming the
// resnets' conv weights as well added nothing (..._plus_conv_modules.log) and is not done
int run_transformer(emu_unet* u, const Transformer& t, const bf16_t* x, bf16_t* out, const Ws& w, int Bn, int H, int W, hipStream_t s) {
    const int HW = H * W, M = Bn * HW, C = t.c, D = 64;
    const int hwpad = (HW + 63) / 64 * 64, npad = (u->n_ctx + 63) / 64 * 64, n = u->n_ctx;
    const float scale = 0.125f;
    const int hb = u->cfg_half < 0 ? 0 : u->cfg_half;     // first row of the CFG pair this call computes
    const size_t CC = (size_t)C * C * 2;
    const BlockPlan plan = unet_block_plan(u->fp8, u->fusion, M, C, HW, n, (int)t.blocks.size());
    // the epilogue block of a GEMM that writes the stream (`stats`: a folded LayerNorm reads its rows next) and names its successor
    auto chain = [&](bool stats, const void* next, size_t next_bytes) {
        Fx fx;
        if (stats && plan.ln_fold) fx.stats_out = w.lnstats;
        if (plan.prefetch) { fx.pf = next; fx.pf_bytes = next_bytes; }
        return fx;
    };
    auto operand = [&](const Proj& P) { return plan.ln_fold ? (const void*)P.wln : (const void*)P.w; };   // of a GEMM behind a LayerNorm
    // the LayerNorm in front of a projection, three ways: folded into the projection (nothing launched: project(.., normed) hands
    // it the stream's statistics), a launch into w.ln, or (fp8) a launch that leaves the projection's e4m3 operand in w.x8 / w.xs
    auto norm_into = [&](const bf16_t* xin, const LnGB& ln, const bf16_t** A) -> int {
        *A = plan.ln_fold ? xin : w.ln;
        if (plan.fp8) UTRY(launch_layernorm_q8(xin, ln.g, ln.b, nullptr, nullptr, w.x8, w.xs, M, C, 1e-5f, s));
        else if (!plan.ln_fold) UTRY(launch_layernorm(xin, ln.g, ln.b, nullptr, w.ln, M, C, 1e-5f, s));
        return 0;
    };
    // one projection of a block, A [M, K] packed: bf16, or (plan.fp8) the rows quantised per row unless norm_into just did + the
    // fp8 x fp8 GEMM (emu_linear_fp8_bf16's kernels).  normed: A comes from norm_into.  gemm() refuses an Fx at M <= 8, and the
    // plan sets no field there: it is passed only when it says something.  (The fp8 GEMM takes the V^T and cross-attention fields;
    // the plan leaves the LayerNorm fold, the row statistics and the prefetch unset in fp8 mode.)
    auto project = [&](const bf16_t* A, const Proj& P, const bf16_t* res, bf16_t* Cc, int N, int K, int ldres, int ldc, int epi, Fx fx,
                       bool normed = false) -> int {
        if (normed && plan.ln_fold) { fx.ln = &P; fx.stats_in = w.lnstats; }
        if (!plan.fp8) {
            UTRY(gemm(u, A, P.w, P.b, res, Cc, M, N, K, K, ldres, ldc, epi, s, fx.any() ? &fx : nullptr));
            return 0;
        }
        if (!normed) UTRY(launch_quant_fp8_rows(A, K, w.x8, K, w.xs, M, K, s));
        GemmArgs g{reinterpret_cast<const bf16_t*>(w.x8), reinterpret_cast<const bf16_t*>(P.q), P.b, res, Cc, M, N, K, K, K, ldres, ldc,
                   epi, NOCONV, nullptr, 0, 0};
        g.a_scale = w.xs; g.w_scale = P.s;
        g.partial = u->splitk; g.partial_floats = u->splitk_floats;
        apply_fx(g, fx);
        UTRY(launch_gemm_fp8(g, s));
        return 0;
    };
    // a -> b = a + out(attention(qkv(LayerNorm(a))))
    auto self_attention = [&](const TBlock& tb, const bf16_t* a, bf16_t* b) -> int {
        const bf16_t* A;
        UPASS(norm_into(a, tb.ln1, &A));
        Fx fx = chain(false, tb.o1.w, CC);
        if (plan.vt_epilogue) { fx.vt = w.vt; fx.vt_col0 = 2 * C; fx.vt_s = HW; fx.vt_spad = hwpad; }
        UPASS(project(A, tb.qkv, nullptr, w.qkv, 3 * C, C, 0, 3 * C, EPI_NONE, fx, true));
        if (!plan.vt_epilogue) {
            TransposeVArgs tv{w.qkv + 2 * C, (long)HW * 3 * C, (long)D, (long)3 * C, w.vt, Bn, t.heads, HW, D, hwpad};
            UTRY(launch_transpose_v(tv, s));
        }
        FlashArgs f{w.qkv, (long)HW * 3 * C, (long)D, (long)3 * C, w.qkv + C, (long)HW * 3 * C, (long)D, (long)3 * C, w.vt,
                    w.att, (long)HW * C, (long)D, (long)C, nullptr, Bn, t.heads, HW, HW, hwpad, D, 0, scale};
        UTRY(launch_flash_attn(f, s));
        return project(w.att, tb.o1, a, b, C, C, C, C, EPI_RESID, chain(true, operand(tb.q2), CC));
    };
    // b -> a = b + out(attention of to_q(LayerNorm(b)) over the cached context K / Vt)
    auto cross_attention = [&](const TBlock& tb, const bf16_t* b, bf16_t* a) -> int {
        const bf16_t* A;
        UPASS(norm_into(b, tb.ln2, &A));
        const bf16_t* kv = u->ctx_cache + tb.ctx_off + (size_t)hb * n * 2 * C;      // the cache holds both rows of the CFG pair
        const bf16_t* vt = u->ctx_cache + tb.ctx_off + (size_t)2 * n * 2 * C + (size_t)hb * C * npad;
        Fx fx = chain(false, tb.o2.w, CC);
        if (plan.cross_epilogue) {                       // to_q + the whole 64-key attention in one launch: writes w.att directly
            fx.cross_k = kv; fx.cross_vt = vt; fx.cross_ldk = 2 * C; fx.cross_n = n; fx.cross_npad = npad; fx.cross_rows = HW;
            fx.cross_scale = scale;
        }
        UPASS(project(A, tb.q2, nullptr, plan.cross_epilogue ? w.att : w.q2, C, C, 0, C, EPI_NONE, fx, true));
        if (!plan.cross_epilogue) {
            FlashArgs f{w.q2, (long)HW * C, (long)D, (long)C, kv, (long)n * 2 * C, (long)D, (long)2 * C, vt,
                        w.att, (long)HW * C, (long)D, (long)C, nullptr, Bn, t.heads, HW, n, npad, D, 0, scale};
            UTRY(launch_flash_attn(f, s));
        }
        return project(w.att, tb.o2, b, a, C, C, C, C, EPI_RESID, chain(true, operand(tb.gg), 8 * CC));
    };
    // a -> b = a + ff_out(GEGLU(LayerNorm(a))); its statistics feed the next block's first LayerNorm (none after the last block)
    auto feed_forward = [&](const TBlock& tb, const bf16_t* a, bf16_t* b, const TBlock* next) -> int {
        const bf16_t* A;
        UPASS(norm_into(a, tb.ln3, &A));
        UPASS(project(A, tb.gg, nullptr, w.ff, 8 * C, C, 0, 4 * C, EPI_GEGLU, chain(false, tb.ff.w, 4 * CC), true));
        return project(w.ff, tb.ff, a, b, C, 4 * C, C, C, EPI_RESID,
                       chain(next != nullptr, next ? operand(next->qkv) : (const void*)t.pow_, next ? 3 * CC : CC));
    };
    UTRY(launch_groupnorm(x, t.gng, t.gnb, w.gn, w.gnws, Bn, HW, C, u->cfg.groups, 1e-6f, 0, s));
    { const Fx fx = chain(true, plan.prefetch ? operand(t.blocks[0].qkv) : nullptr, 3 * CC);
      UTRY(gemm(u, w.gn, t.piw, t.pib, nullptr, w.tokA, M, C, C, C, 0, C, EPI_NONE, s, fx.any() ? &fx : nullptr)); }
    bf16_t *a = w.tokA, *b = w.tokB;
    for (size_t bi = 0; bi < t.blocks.size(); ++bi) {
        const TBlock& tb = t.blocks[bi];
        UPASS(self_attention(tb, a, b));
        UPASS(cross_attention(tb, b, a));
        UPASS(feed_forward(tb, a, b, bi + 1 < t.blocks.size() ? &t.blocks[bi + 1] : nullptr));
        std::swap(a, b);
    }
    UTRY(gemm(u, a, t.pow_, t.pob, x, out, M, C, C, C, C, C, EPI_RESID, s));
    return 0;
}

}  // namespace

extern "C" {

size_t emu_groupnorm_ws_bytes(int Bn, int HW, int C) { return gn_ws_floats(Bn, C, HW) * sizeof(float); }

int emu_groupnorm_nhwc_bf16(const void* x, const void* gamma, const void* beta, void* y, void* ws, int Bn, int HW, int C,
                            int groups, float eps, int silu, emu_stream_t s) {
    return launch_groupnorm(B16(x), B16(gamma), B16(beta), reinterpret_cast<bf16_t*>(y), reinterpret_cast<float*>(ws), Bn, HW, C,
                            groups, eps, silu, S(s));
}

int emu_conv3x3_nhwc_bf16(const void* x, const void* w, const void* bias, const void* bias2, int ld_bias2, const void* res,
                          void* y, int Bn, int Hin, int Win, int Cin, int Cout, int mode, emu_stream_t s) {
    return conv3(nullptr, B16(x), B16(w), B16(bias), B16(bias2), ld_bias2, B16(res), reinterpret_cast<bf16_t*>(y), Bn, Hin, Win,
                 Cin, Cout, mode, S(s));
}

int emu_unet_create(emu_ctx* ctx, const emu_unet_cfg* cfg, emu_unet** out) {
    if (!ctx || !cfg || !out) return -22;
    for (int i = 0; i < 3; ++i)
        if ((cfg->ch[i] & 63) || (cfg->attn[i] && cfg->ch[i] != cfg->heads[i] * 64)) return emu_ctx_fail(ctx, -22, "emu_unet_create: channels must be multiples of 64 and heads*64");
    if (cfg->kpad_in < 9 * cfg->in_ch || (cfg->kpad_in & 7) || cfg->out_ch != 4 || cfg->in_ch != 4) return emu_ctx_fail(ctx, -22, "emu_unet_create: bad conv_in/out config");
    emu_unet* u = new emu_unet();
    u->ctx = ctx; u->cfg = *cfg;
    *out = u;
    return 0;
}
void emu_unet_destroy(emu_unet* u) { delete u; }

int emu_unet_set_weight(emu_unet* u, const char* name, const void* ptr) {
    if (!u || !name || !ptr) return -22;
    u->w[name] = B16(ptr);
    const std::string nm(name);
    const bool f8name = (nm.size() > 4 && nm.compare(nm.size() - 4, 4, ".fp8") == 0) || (nm.size() > 5 && nm.compare(nm.size() - 5, 5, ".fp8s") == 0);
    if (!f8name) u->finalized = false;                  // (fp8 copies are resolved by emu_unet_use_fp8, not by finalize)
    return 0;
}

// W8A8 mode of the transformer blocks: every block's six packed matrices must have been registered a second time as
// "<name>.fp8" (e4m3 bytes of emu_quantize_fp8_rows) and "<name>.fp8s" (fp32 row scales) with emu_unet_set_weight.
// Changes emu_unet_workspace_bytes; invalidates captured graphs of the step (the caller's business).
int emu_unet_use_fp8(emu_unet* u, int enable) {
    if (!u || !u->finalized) return -22;
    if (!enable) { u->fp8 = false; return 0; }
    bool ok = true;
    each_transformer(u, [&](Transformer& t) {
        for (int k = 0; k < t.depth; ++k) resolve_block(u, t.blocks[k], t.name + "transformer_blocks." + std::to_string(k) + ".", true, &ok);
        return 0;
    });
    if (!ok) return emu_ctx_fail(u->ctx, -2, u->err.c_str());
    u->fp8 = true;
    return 0;
}

// Traversal order shared with emu_amd/unet.py (temb_proj_all concatenation): down i,j ; mid 0,1 ; up i,j.
int emu_unet_finalize(emu_unet* u) {
    if (!u) return -22;
    const emu_unet_cfg& c = u->cfg;
    bool ok = true;
    u->fusion_avail = 7;                               // resolve_transformer clears bit 0 when a packed tensor is missing
    int toff = 0;
    auto mk_res = [&](const std::string& name, int cin, int cout) {
        Resnet r{}; r.name = name; r.cin = cin; r.cout = cout; r.temb_off = toff; toff += cout;
        resolve_resnet(u, r, &ok);
        return r;
    };
    auto mk_tr = [&](const std::string& name, int ch, int depth, int heads) {
        Transformer t{}; t.name = name; t.c = ch; t.depth = depth; t.heads = heads;
        resolve_transformer(u, t, &ok);
        return t;
    };
    u->conv_in_w = find(u, "conv_in.w", true, &ok); u->conv_in_b = find(u, "conv_in.b", true, &ok);
    u->te1w = find(u, "time_embedding.linear_1.w", true, &ok); u->te1b = find(u, "time_embedding.linear_1.b", true, &ok);
    u->te2w = find(u, "time_embedding.linear_2.w", true, &ok); u->te2b = find(u, "time_embedding.linear_2.b", true, &ok);
    u->ae1w = find(u, "add_embedding.linear_1.w", true, &ok); u->ae1b = find(u, "add_embedding.linear_1.b", true, &ok);
    u->ae2w = find(u, "add_embedding.linear_2.w", true, &ok); u->ae2b = find(u, "add_embedding.linear_2.b", true, &ok);
    u->tpw = find(u, "temb_proj_all.w", true, &ok); u->tpb = find(u, "temb_proj_all.b", true, &ok);
    u->cno_g = find(u, "conv_norm_out.g", true, &ok); u->cno_b = find(u, "conv_norm_out.b", true, &ok);
    u->cout_w = find(u, "conv_out.w", true, &ok); u->cout_b = find(u, "conv_out.b", true, &ok);
    int cin = c.ch[0];
    for (int i = 0; i < 3; ++i) {
        u->down_res[i].clear(); u->down_tr[i].clear();
        for (int j = 0; j < c.layers_per_block; ++j) {
            const std::string p = "down_blocks." + std::to_string(i);
            u->down_res[i].push_back(mk_res(p + ".resnets." + std::to_string(j) + ".", j == 0 ? cin : c.ch[i], c.ch[i]));
            if (c.attn[i]) u->down_tr[i].push_back(mk_tr(p + ".attentions." + std::to_string(j) + ".", c.ch[i], c.depth[i], c.heads[i]));
        }
        if (i < 2) {
            const std::string p = "down_blocks." + std::to_string(i) + ".downsamplers.0.conv.";
            u->down_ds_w[i] = find(u, p + "w", true, &ok); u->down_ds_b[i] = find(u, p + "b", true, &ok);
        }
        cin = c.ch[i];
    }
    u->mid_res[0] = mk_res("mid_block.resnets.0.", c.ch[2], c.ch[2]);
    u->mid_tr = mk_tr("mid_block.attentions.0.", c.ch[2], c.depth[2], c.heads[2]);
    u->mid_res[1] = mk_res("mid_block.resnets.1.", c.ch[2], c.ch[2]);
    int out = c.ch[2];
    for (int i = 0; i < 3; ++i) {                      // up block i works at level 2-i
        const int lvl = 2 - i;
        const int prev = out; out = c.ch[lvl];
        const int inp = c.ch[lvl > 0 ? lvl - 1 : 0];
        u->up_res[i].clear(); u->up_tr[i].clear();
        for (int j = 0; j <= c.layers_per_block; ++j) {
            const int skip = (j == c.layers_per_block) ? inp : out;
            const int first = (j == 0) ? prev : out;
            const std::string p = "up_blocks." + std::to_string(i);
            u->up_res[i].push_back(mk_res(p + ".resnets." + std::to_string(j) + ".", first + skip, out));
            if (c.attn[lvl]) u->up_tr[i].push_back(mk_tr(p + ".attentions." + std::to_string(j) + ".", out, c.depth[lvl], c.heads[lvl]));
        }
        if (i < 2) {
            const std::string p = "up_blocks." + std::to_string(i) + ".upsamplers.0.conv.";
            u->up_us_w[i] = find(u, p + "w", true, &ok); u->up_us_b[i] = find(u, p + "b", true, &ok);
        }
    }
    u->temb_total = toff;
    if (!ok) return emu_ctx_fail(u->ctx, -2, u->err.c_str());
    u->fusion = u->fusion_avail;
    u->fp8 = false;                                    // the blocks were re-resolved: emu_unet_use_fp8 again
    u->finalized = true;
    return 0;
}

int emu_unet_set_fusion(emu_unet* u, int mask) {
    if (!u || !u->finalized) return -22;
    u->fusion = mask & u->fusion_avail;
    return u->fusion;
}

int emu_unet_block_plan(int fp8, int fusion, int M, int C, int HW, int n_ctx, int depth) {
    if ((fp8 | 1) != 1 || (fusion | 7) != 7 || HW < 1 || M < HW || M % HW || C < 1 || n_ctx < 1 || depth < 0) return -22;
    const BlockPlan p = unet_block_plan(fp8 != 0, fusion, M, C, HW, n_ctx, depth);
    return p.fp8 | p.ln_fold << 1 | p.vt_epilogue << 2 | p.cross_epilogue << 3 | p.prefetch << 4;
}

int emu_unet_temb_total(const emu_unet* u) { return u ? u->temb_total : 0; }

size_t emu_unet_workspace_bytes(const emu_unet* u, int H, int W) {
    if (!u || !u->finalized) return 0;
    return plan_ws(u, H, W, nullptr).total;
}

// context cache layout, per transformer block in traversal order: KV rows [B*n, 2C] then Vt [B, heads, 64, npad]
size_t emu_unet_context_bytes(const emu_unet* u, int n_ctx) {
    if (!u || !u->finalized) return 0;
    const size_t npad = (size_t)(n_ctx + 63) / 64 * 64;
    size_t el = 0;
    each_transformer(u, [&](const Transformer& t) { el += t.blocks.size() * ((size_t)2 * n_ctx * 2 * t.c + (size_t)2 * t.c * npad); return 0; });
    return el * 2 + (size_t)2 * u->cfg.temb_dim * 2 + 256;
}

// Once per generation (prompt fixed over all steps): cross-attention K / V^T of every transformer block from the
// prompt embeddings ctx [2, n, cross] (cond first), and aug_emb = add_embedding(cat(text_embeds, time_ids emb))
// from add_in [2, proj_class_in].  Results live in `cache` (emu_unet_context_bytes), owned by the caller.
int emu_unet_set_context(emu_unet* u, const void* ctx_tokens, int n_ctx, const void* add_in, int add_dim, void* cache,
                         size_t cache_bytes, void* workspace, size_t ws_bytes, emu_stream_t s_) {
    if (!u || !u->finalized || !ctx_tokens || !add_in || !cache) return -22;
    if (cache_bytes < emu_unet_context_bytes(u, n_ctx)) return ufail(u, -12, "emu_unet_set_context: cache too small");
    if (ws_bytes < (size_t)2 * u->cfg.temb_dim * 2) return ufail(u, -12, "emu_unet_set_context: workspace too small");
    hipStream_t s = S(s_);
    const int Bn = 2, cross = u->cfg.cross_dim;
    const int npad = (n_ctx + 63) / 64 * 64;
    bf16_t* base = reinterpret_cast<bf16_t*>(cache);
    size_t off = 0;
    u->n_ctx = n_ctx;
    UPASS(each_transformer(u, [&](Transformer& t) -> int {
        for (TBlock& tb : t.blocks) {
            tb.ctx_off = off;
            bf16_t* kv = base + off;
            bf16_t* vt = kv + (size_t)Bn * n_ctx * 2 * t.c;
            UTRY(gemm(u, B16(ctx_tokens), tb.kv2, nullptr, nullptr, kv, Bn * n_ctx, 2 * t.c, cross, cross, 0, 2 * t.c, EPI_NONE, s));
            TransposeVArgs tv{kv + t.c, (long)n_ctx * 2 * t.c, 64L, (long)2 * t.c, vt, Bn, t.heads, n_ctx, 64, npad};
            UTRY(launch_transpose_v(tv, s));
            off += (size_t)Bn * n_ctx * 2 * t.c + (size_t)Bn * t.c * npad;
        }
        return 0;
    }));
    bf16_t* aug = base + off;
    bf16_t* tmp = reinterpret_cast<bf16_t*>(workspace);
    UTRY(gemm(u, B16(add_in), u->ae1w, u->ae1b, nullptr, tmp, Bn, u->cfg.temb_dim, add_dim, add_dim, 0, u->cfg.temb_dim, EPI_SILU, s));
    UTRY(gemm(u, tmp, u->ae2w, u->ae2b, nullptr, aug, Bn, u->cfg.temb_dim, u->cfg.temb_dim, u->cfg.temb_dim, 0, u->cfg.temb_dim, EPI_NONE, s));
    u->ctx_cache = base;
    u->aug_emb = aug;
    return 0;
}

// The UNet forward on the im2col'ed, already scaled input in ws.colin; result (noise prediction, NHWC [2*HW, 4]) in out.
static int unet_body(emu_unet* u, const Ws& w, int H, int W, const bf16_t* temb_table, const int32_t* step, bf16_t* out, hipStream_t s) {
    const emu_unet_cfg& c = u->cfg;
    const int Bn = u->cfg_half < 0 ? 2 : 1;
    const bf16_t* aug = u->aug_emb + (u->cfg_half < 0 ? 0 : (size_t)u->cfg_half * c.temb_dim);
    // ---- time embedding: Timesteps row of this step -> MLP; + aug_emb; SiLU; every resnet's time_emb_proj in one GEMV
    UTRY(launch_gather_step_row(temb_table, step, w.temb_in, Bn, c.ch[0], s));
    UTRY(gemm(u, w.temb_in, u->te1w, u->te1b, nullptr, w.e1, Bn, c.temb_dim, c.ch[0], c.ch[0], 0, c.temb_dim, EPI_SILU, s));
    UTRY(gemm(u, w.e1, u->te2w, u->te2b, nullptr, w.emb, Bn, c.temb_dim, c.temb_dim, c.temb_dim, 0, c.temb_dim, EPI_NONE, s));
    UTRY(launch_add_silu(w.emb, aug, nullptr, w.semb, Bn * c.temb_dim, s));
    UTRY(gemm(u, w.semb, u->tpw, u->tpb, nullptr, w.temb_all, Bn, u->temb_total, c.temb_dim, c.temb_dim, 0, u->temb_total, EPI_NONE, s));
    // ---- conv_in
    int hs[3] = {H, (H + 1) / 2, (H + 3) / 4}, wsz[3] = {W, (W + 1) / 2, (W + 3) / 4};
    int k = 0;
    UTRY(gemm(u, w.colin, u->conv_in_w, u->conv_in_b, nullptr, w.skip[k], Bn * H * W, c.ch[0], c.kpad_in, c.kpad_in, 0, c.ch[0], EPI_NONE, s));
    const bf16_t* h = w.skip[k++];
    // ---- down
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < c.layers_per_block; ++j) {
            bf16_t* dst = c.attn[i] ? w.hA : w.skip[k];
            UPASS(run_resnet(u, u->down_res[i][j], h, dst, w, Bn, hs[i], wsz[i], s));
            if (c.attn[i]) UPASS(run_transformer(u, u->down_tr[i][j], dst, w.skip[k], w, Bn, hs[i], wsz[i], s));
            h = w.skip[k++];
        }
        if (i < 2) {
            UTRY(conv3(u, h, u->down_ds_w[i], u->down_ds_b[i], nullptr, 0, nullptr, w.skip[k], Bn, hs[i], wsz[i], c.ch[i], c.ch[i], CONV_3X3_S2, s));
            h = w.skip[k++];
        }
    }
    // ---- mid
    UPASS(run_resnet(u, u->mid_res[0], h, w.hA, w, Bn, hs[2], wsz[2], s));
    UPASS(run_transformer(u, u->mid_tr, w.hA, w.hB, w, Bn, hs[2], wsz[2], s));
    UPASS(run_resnet(u, u->mid_res[1], w.hB, w.hA, w, Bn, hs[2], wsz[2], s));
    bf16_t* cur = w.hA;
    bf16_t* oth = w.hB;
    int cur_c = c.ch[2];
    // ---- up
    for (int i = 0; i < 3; ++i) {
        const int lvl = 2 - i;
        for (size_t j = 0; j < u->up_res[i].size(); ++j) {
            const Resnet& r = u->up_res[i][j];
            const bf16_t* skip = w.skip[--k];
            const int skip_c = r.cin - cur_c;
            UTRY(launch_concat_channels(cur, skip, w.cat, Bn * hs[lvl] * wsz[lvl], cur_c, skip_c, s));
            UPASS(run_resnet(u, r, w.cat, oth, w, Bn, hs[lvl], wsz[lvl], s));
            if (c.attn[lvl]) UPASS(run_transformer(u, u->up_tr[i][j], oth, cur, w, Bn, hs[lvl], wsz[lvl], s));
            else std::swap(cur, oth);
            cur_c = r.cout;
        }
        if (i < 2) {
            UTRY(conv3(u, cur, u->up_us_w[i], u->up_us_b[i], nullptr, 0, nullptr, oth, Bn, hs[lvl], wsz[lvl], cur_c, cur_c, CONV_3X3_UP2, s));
            std::swap(cur, oth);
        }
    }
    // ---- out
    UTRY(launch_groupnorm(cur, u->cno_g, u->cno_b, w.gn, w.gnws, Bn, H * W, c.ch[0], c.groups, c.gn_eps, 1, s));
    UTRY(conv3(u, w.gn, u->cout_w, u->cout_b, nullptr, 0, nullptr, out, Bn, H, W, c.ch[0], c.out_ch, CONV_3X3, s));
    return 0;
}

int emu_unet_step(emu_unet* u, void* latents, int H, int W, const void* temb_table, const void* sigmas, int32_t* step_dev,
                  float guidance, void* workspace, size_t ws_bytes, emu_stream_t s_) {
    if (!u || !u->finalized || !latents || !temb_table || !sigmas || !step_dev) return -22;
    if (!u->ctx_cache) return ufail(u, -22, "emu_unet_step: emu_unet_set_context has not been called");
    if ((H & 3) || (W & 3)) return ufail(u, -22, "emu_unet_step: latent H, W must be multiples of 4");
    if (u->cfg_half >= 0) return ufail(u, -22, "emu_unet_step: one row of the CFG pair is set (emu_unet_set_cfg_half): emu_unet_forward + emu_unet_cfg_euler_step");
    const Ws w = plan_ws(u, H, W, workspace);
    u->splitk = w.splitk; u->splitk_floats = w.splitk_floats;
    if (w.total > ws_bytes) return ufail(u, -12, "emu_unet_step: workspace too small");
    hipStream_t s = S(s_);
    UTRY(launch_unet_prep_input(reinterpret_cast<bf16_t*>(latents), reinterpret_cast<const float*>(sigmas), step_dev, w.colin,
                                u->cfg.in_ch, H, W, u->cfg.kpad_in, s));
    bf16_t* eps = w.t1;                                  // [2*H*W, 4], t1 is free once the last resnet is done
    UPASS(unet_body(u, w, H, W, B16(temb_table), step_dev, eps, s));
    UTRY(launch_cfg_euler_step(eps, reinterpret_cast<bf16_t*>(latents), reinterpret_cast<const float*>(sigmas), step_dev, guidance,
                               u->cfg.in_ch, H * W, s));
    return 0;
}

// Bare UNet forward for parity tests: scaled NCHW input of ONE sample is taken from `latents` with sigma table entry
// sigmas[step] (pass sigma = 0 for no scaling), noise prediction returned as NHWC [2*H*W, 4] in eps_out.
int emu_unet_forward(emu_unet* u, const void* latents, int H, int W, const void* temb_table, const void* sigmas,
                     const int32_t* step_dev, void* eps_out, void* workspace, size_t ws_bytes, emu_stream_t s_) {
    if (!u || !u->finalized || !latents || !temb_table || !sigmas || !step_dev || !eps_out) return -22;
    if (!u->ctx_cache) return ufail(u, -22, "emu_unet_forward: emu_unet_set_context has not been called");
    const Ws w = plan_ws(u, H, W, workspace);
    u->splitk = w.splitk; u->splitk_floats = w.splitk_floats;
    if (w.total > ws_bytes) return ufail(u, -12, "emu_unet_forward: workspace too small");
    hipStream_t s = S(s_);
    UTRY(launch_unet_prep_input(B16(latents), reinterpret_cast<const float*>(sigmas), step_dev, w.colin, u->cfg.in_ch, H, W,
                                u->cfg.kpad_in, s));
    return unet_body(u, w, H, W, B16(temb_table), step_dev, reinterpret_cast<bf16_t*>(eps_out), s);
}

int emu_unet_set_cfg_half(emu_unet* u, int half) {
    if (!u || half < -1 || half > 1) return -22;
    u->cfg_half = half;
    return 0;
}

int emu_unet_cfg_euler_step(emu_unet* u, const void* eps_pair, void* latents, int H, int W, const void* sigmas, int32_t* step_dev,
                            float guidance, emu_stream_t s_) {
    if (!u || !eps_pair || !latents || !sigmas || !step_dev) return -22;
    UTRY(launch_cfg_euler_step(B16(eps_pair), reinterpret_cast<bf16_t*>(latents), reinterpret_cast<const float*>(sigmas), step_dev, guidance,
                               u->cfg.in_ch, H * W, S(s_)));
    return 0;
}

}  // extern "C"
