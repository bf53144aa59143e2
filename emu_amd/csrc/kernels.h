// Internal launch interface between the C-ABI layer (capi.cpp / engine.cpp) and the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/emu_hip.h"
#include "l2_warm.h"

typedef uint16_t bf16_t;

enum EmuEpilogue { EPI_NONE = 0, EPI_RESID = 1, EPI_SWIGLU = 2, EPI_SILU = 3, EPI_GELU = 4, EPI_GEGLU = 5 };

struct GemvArgs {
    const bf16_t* x;        // [M, ldx]
    const bf16_t* W;        // [N, ldw]   (K contiguous)
    const bf16_t* norm_w;   // [K] or null: fused RMSNorm prologue on x
    const bf16_t* bias;     // [N] or null
    const bf16_t* res;      // [M, ldres] (EPI_RESID)
    bf16_t* out;            // [M, ldo]   (EPI_SWIGLU: N/2 columns)
    int M, N, K;
    int ldx, ldw, ldres, ldo;
    float eps;
    int epi;
    const float* wscale;    // non-null: W holds OCP fp8 e4m3 bytes [N, ldw] with one fp32 scale per row (K % 16 == 0)
    // non-null: W holds MXFP4 element bytes [N, ldw] (two E2M1 codes per byte, ldw in bytes) and w4scale the E8M0 block scales
    // [N, lds], one per 32 elements (K % 32 == 0, M <= 2): gemv_fp4.hip
    const uint8_t* w4scale = nullptr;
    int lds = 0;
    // L2 warming of the launch that follows (l2_warm.h): the last workgroups of the one-row bf16 stream forms (head, preload,
    // single round trip) request the head of the successor's weights.  ntouch == 0: none; every other kernel ignores it.
    WarmPlan warm;
};
// The stream plan (gemv.hip): gemv_plan is everything launch_gemv decides between a shape and a launch -- pure host arithmetic, no
// HIP call, no global read (tune: the emu_gemm_tune mask) -- and launch_gemv is shape (gemv_shape_of) -> gemv_plan -> one launch of
// the plan.  The three matrix-core few-row streams (bf16 gemv_thin.hip, fp8 gemv_fp8_thin.hip, MXFP4 gemv_fp4_thin.hip) have one
// planner of the same kind inside it, gemv_thin_plan, which picks the kind from the shape's fp8 / fp4 flags: gemv_plan asks it for
// bf16 from 4 rows on, and launch_gemv_thin_stream is shape -> gemv_thin_plan -> the checks only pointers can answer (x, W, out,
// res under RESID, a 4-byte aligned w4scale) -> one launch of the plan, for any of the three kinds.  The C-ABI test hooks
// emu_gemv_plan / emu_gemv_thin_plan return the same (include/emu_hip.h describes the fields).
using GemvShape = emu_gemv_shape;
using GemvPlan = emu_gemv_plan_t;
enum GemvFamily { GEMV_FAM_BLOCK = 0, GEMV_FAM_RT = 1, GEMV_FAM_WAVE = 2, GEMV_FAM_MFMA = 3, GEMV_FAM_THIN = 4, GEMV_FAM_FP8_BLOCK = 5,
                  GEMV_FAM_FP8_RT = 6, GEMV_FAM_FP4_ROWS = 7, GEMV_FAM_FP8_THIN = 8, GEMV_FAM_FP4_THIN = 9, GEMV_FAM_PACK_THIN = 10 };
// the form of a one-row bf16 stream; workgroup j reads weight rows [j * rows, j * rows + rows)  (GEMV_FORM_WAVE: 4 waves x 4 whole rows)
enum GemvForm { GEMV_FORM_ROLLING = 0, GEMV_FORM_HEAD = 1, GEMV_FORM_PRELOAD = 2, GEMV_FORM_RT = 3, GEMV_FORM_WAVE = 4 };
GemvShape gemv_shape_of(const GemvArgs& a);
GemvShape gemv_one_row_shape(int N, int K, bool norm, int epi);   // one bf16 row on aligned, row-contiguous operands
GemvPlan gemv_plan(const GemvShape& shape, int tune);
int launch_gemv(const GemvArgs& a, hipStream_t s);
int launch_gemv_thin_stream(const GemvArgs& a, hipStream_t s);
// the plan of a one-row bf16 stream on aligned, row-contiguous operands under the current emu_gemm_tune mask, projected to
// {form, rows} (the successor geometry of l2_warm.h)
struct GemvGeom { int form, rows; };
GemvGeom emu_gemv_geometry(int N, int K, bool norm, int epi);
int emu_gemv_rows_per_block(int N, int K, bool norm);      // the one-row block kernel's heuristic (gemv.hip)
inline bool gemv_form_warms(int form) { return form == GEMV_FORM_HEAD || form == GEMV_FORM_PRELOAD || form == GEMV_FORM_RT; }
// 9..16 rows reach the stream family (the register-fed MFMA kernel, or the thin stream ahead of it) exactly when this holds; the
// callers that choose between launch_gemv and a GEMM ask here
bool gemv_rows_9_16_ok(int M, int K, int ldx, int ldw, bool norm, bool fp8, int epi);
// the family launchers of the other files, called with a plan of their family, each only the switch from plan fields to template
// arguments (-22: a combination that is not built): the MXFP4 weight stream of 1..2 rows (gemv_fp4.hip; plan_fp4: threads per row set
// and row sets per workgroup for rows of KB blocks) and the three LDS-DMA streams on the matrix cores (gemv_thin.hip,
// gemv_fp8_thin.hip: a.wscale set, W = e4m3 bytes, ldw in bytes; gemv_fp4_thin.hip: a.w4scale set, W = element bytes, ldw in bytes)
constexpr int GEMV_FP4_MAX_SETS = 16;
int launch_gemv_fp4(const GemvArgs& a, const GemvPlan& p, hipStream_t s);
void plan_fp4(int KB, int* threads_per_row_set, int* row_sets);
int launch_gemv_thin(const GemvArgs& a, const GemvPlan& p, hipStream_t s);
int launch_gemv_fp8_thin(const GemvArgs& a, const GemvPlan& p, hipStream_t s);
int launch_gemv_fp4_thin(const GemvArgs& a, const GemvPlan& p, hipStream_t s);
// the MXFP4 quantiser: bf16 [N, ldw] -> element bytes [N, ldq] + E8M0 scales [N, lds], bit-exact with
// emu_amd/mxfp4.py::quantize_rows; -22 for non-finite weights (the call waits for its own result)
int launch_quant_mxfp4_rows(const bf16_t* w, int ldw, uint8_t* q, int ldq, uint8_t* scales, int lds, int N, int K, hipStream_t s);
void plan_fp4(int KB, int* threads_per_row_set, int* row_sets);
// the 13-bit lossless bf16 weight format (bf16_pack.h).  launch_bf16_pack (bf16_pack.hip): bf16 [N, ldw] -> the planes and the flag
// bitmap for row groups of `rows` (2 / 4) rows, K % 32 == 0; *hb_out = the matrix's exponent base (the call waits for its own result).
// gemv_pack_rows: the set's rows per group if the bf16 plan of the one-row shape is a form the packed stream has a twin for (head
// form of 4 rows, preload form of 2, single round trip of 2 x 9 trips), else 0.  launch_gemv_pack (gemv_pack.hip): that twin; a.W = the
// bf16 matrix (flagged row groups read it), form = the plan's GemvForm; bit-identical to launch_gemv on the bf16 matrix
int launch_bf16_pack(const bf16_t* W, int ldw, int N, int K, int rows, void* lo, void* nib, void* sign, uint32_t* flags, int* hb_out,
                     hipStream_t s);
// the 12-bit format's packer: planes, patch records (8 slots of 32 bits per row group) and flags; *hb_out = the base of the matrix's
// 8-code window, *flagged_out = the flagged row groups (what the rule that picks a matrix's format reads).  launch_gemv_pack takes
// either format's set (PackSet::patch set = 12 bits)
int launch_bf16_pack12(const bf16_t* W, int ldw, int N, int K, int rows, void* lo, void* nib, void* patch, uint32_t* flags, int* hb_out,
                       int* flagged_out, hipStream_t s);
int gemv_pack_rows(const GemvPlan& p, const GemvShape& sh);
int launch_gemv_pack(const GemvArgs& a, const struct PackSet& p, int form, hipStream_t s);
// the few-row (4..16) twin (gemv_pack_thin.hip): the same sets through the bf16 thin stream's arithmetic at kch 32.  gemv_pack_thin_plan
// (gemv.hip): family GEMV_FAM_PACK_THIN with rows, mb, stages, kch, grid, block exactly when gemv_plan sends the bf16 shape (no fused
// norm) to GEMV_FAM_THIN with a kch that has a twin, set_rows is 2 or 4, 4 <= M <= 16 and the epilogue is NONE / RESID / SWIGLU; else
// status -22 and every other field 0.  launch_gemv_pack_thin: that plan's launch; a.W = the bf16 matrix (flagged workgroups stream
// it); bit-identical to launch_gemv on the bf16 matrix.  It takes either format's set under the same plan (PackSet::patch set = the
// 12-bit twin: sign null, 16-byte aligned records, hb 0..120, K / 8 < PACK12_MAX_KV)
GemvPlan gemv_pack_thin_plan(const GemvShape& shape, int set_rows, int tune);
int launch_gemv_pack_thin(const GemvArgs& a, const struct PackSet& p, const GemvPlan& plan, hipStream_t s);
// o_proj of a tensor-parallel shard's one-row step with the decode attention's split merge in its prologue (gemv_merge.hip):
// x = merge of the live splits in decode_fused_kernel's workspace (batch row 0), out = epi(x W^T [+ res]); bit-identical to
// decode_fused_combine_kernel followed by the wave-form GEMV.  K = H * 128 <= 1024, nsplit <= 8, N >= 1024 (gemv_merge_ok).
struct GemvMergeArgs {
    const float* ws;        // [H][nsplit][130] split states of the one batch row (decode_fused_ws_floats layout)
    const int32_t* slot;    // [1] cache slot of the new token: live splits = slot / 128 + 1
    int nsplit, H;          // splits the attention launch was sized for, local heads
    const bf16_t* W;        // [N, ldw]
    const bf16_t* res;      // [N] (EPI_RESID)
    bf16_t* out;            // [N]
    int N, K, ldw, epi;
    bf16_t* x_out;          // null, or [K]: the merged attention output (what the combine launch would have written)
};
bool gemv_merge_ok(int heads, int D, int N, int nsplit);
int launch_gemv_merge(const GemvMergeArgs& a, hipStream_t s);
// MXFP4 weights (a.w4scale set; W = element bytes, ldw in bytes) on the matrix cores: LDS-DMA stages, v_cvt_scalef32_pk_bf16_fp4 and
// v_mfma_f32_16x16x32_bf16, the stage layout and the epilogue shared (fp4_tile.h).  Both kernels fetch a stage's 8 scale bytes per
// row by 4-byte LDS-DMA, so a scale row spans whole stages: fp4_scale_stride(K) bytes at least -- K / 32 where K % 256 == 0, else
// 8 per started stage (K = 896: 32, K = 2240: 72); the padding bytes are read and never used (emu_amd/mxfp4.py::scale_stride).
inline int fp4_scale_stride(int K) { return K % 256 == 0 ? K / 32 : 8 * ((K + 255) / 256); }
// 1..16 rows: a weight stream, every converted fragment used by one MFMA (gemv_fp4_thin.hip), planned by gemv_thin_plan.
// 17 rows and more: a two-dimensional tile, each converted weight fragment feeding several MFMAs (gemm_fp4.hip); ragged M and N.
// fp4_mfma_ok (gemv.hip) is its argument check: the shape conditions of the few-row plan but for the row count -- K >= 256 and
// K % 32 == 0 (K % 256 != 0: the last stage partial), lds % 4 == 0 and lds >= fp4_scale_stride(K), 16-byte aligned W and x, no fused
// norm, epi NONE / RESID / SWIGLU -- and the same pointer checks
bool fp4_mfma_ok(const GemvArgs& a);
int launch_gemm_fp4(const GemvArgs& a, hipStream_t s);
// fp8 weights (a.wscale set; W = e4m3 bytes, ldw in bytes) for 17..64 rows on the matrix cores, W8A16 (gemm_fp8.hip: the tile of
// gemm_fp4.hip fed as gemv_fp8_thin.hip is fed; fp8_tile.h).  gemm_fp8w_plan (gemv.hip): pure host arithmetic from a shape to the form,
// the ring depth and the grid, or status -22 (the C-ABI test hook emu_gemm_fp8w_plan returns the same); launch_gemm_fp8w: the switch
// from a plan to template arguments; launch_gemm_fp8w_stream: shape -> plan -> the checks only pointers can answer -> one launch.
using GemmFp8wPlan = emu_gemm_fp8w_plan_t;
GemmFp8wPlan gemm_fp8w_plan(const GemvShape& shape, int tune);
int launch_gemm_fp8w(const GemvArgs& a, const GemmFp8wPlan& p, hipStream_t s);
int launch_gemm_fp8w_stream(const GemvArgs& a, hipStream_t s);
// The same kernel's form for 65 rows and more (64 weight rows x 128 activation rows, a two-dimensional grid, cached weight loads), with
// the same three steps: gemm_fp8t_plan (C ABI: emu_gemm_fp8t_plan), launch_gemm_fp8t, launch_gemm_fp8t_stream.
using GemmFp8tPlan = emu_gemm_fp8t_plan_t;
GemmFp8tPlan gemm_fp8t_plan(const GemvShape& shape, int tune);
int launch_gemm_fp8t(const GemvArgs& a, const GemmFp8tPlan& p, hipStream_t s);
int launch_gemm_fp8t_stream(const GemvArgs& a, hipStream_t s);

// Implicit-GEMM 3x3 convolution over an NHWC activation: A is [B, Hin, Win, Cin], the GEMM row m is the output
// pixel (b, yo, xo), K = 9*Cin ordered (ky, kx, ci) -- weights repacked to [Cout, 3, 3, Cin].  Cin % 64 == 0.
enum EmuConvMode { CONV_NONE = 0, CONV_3X3 = 1, CONV_3X3_S2 = 2, CONV_3X3_UP2 = 3 };
struct ConvGeom {
    int mode, Hin, Win, Hout, Wout, Cin;
    // set by launch_gemm (0 = off): the gather's fast form for the stride-1 / stride-2 modes.  A k tile (64 channels) lies inside one
    // filter tap; tap = k_tile / cpt is taken as (k_tile * cpt_magic) >> 16 (exact for the < 9 * cpt tiles of a conv), and a tap's
    // source is the output pixel's centre source + (ky - 1) * Win + (kx - 1) pixels, valid where a 9-bit mask computed once per row says
    int cpt = 0, cpt_magic = 0;
};

struct GemmArgs {
    const bf16_t* A;        // [M, lda]  activations (K contiguous)   (conv: NHWC input)
    const bf16_t* W;        // [N, ldw]  weights     (K contiguous)
    const bf16_t* bias;     // [N] or null
    const bf16_t* res;      // [M, ldres] (EPI_RESID)
    bf16_t* C;              // [M, ldc]  (EPI_SWIGLU / EPI_GEGLU: N/2 columns)
    int M, N, K;
    int lda, ldw, ldres, ldc;
    int epi;
    ConvGeom conv;          // mode 0 = plain GEMM
    const bf16_t* bias2;    // [M / rows_per_batch, ld_bias2] or null: per-batch bias added after the first rounding
    int rows_per_batch;     //   (ResnetBlock2D: conv1(x) + time_emb_proj(silu(temb))[:, :, None, None])
    int ld_bias2;
    // optional split-K scratch (fp32, caller-owned): few-tile long-K problems (UNet 32x32-level convs, ff-out) are cut
    // into ksplit K-slices of the big 256x128 tile so every CU gets one workgroup; slices land here and a second
    // launch sums them and applies the epilogue.  null = never split.
    float* partial = nullptr;
    size_t partial_floats = 0;
    int ksplit = 1;         // set by launch_gemm: K-slices of the tail tiles
    // fp8 GEMM (launch_gemm_fp8): A and W hold OCP e4m3 bytes (lda / ldw in elements = bytes), one fp32 scale per
    // activation row / weight row; the fp32 sum is multiplied by a_scale[m] * w_scale[n] ahead of the epilogue
    const float* a_scale = nullptr;
    const float* w_scale = nullptr;
    int full_tiles = 0;     // set by launch_gemm: tiles [0, full_tiles) run whole-K (workgroups [0, full_tiles)); every
                            // later tile t is cut into ksplit slices (workgroup full_tiles + (t - full_tiles) * ksplit + ks)
                            // whose fp32 tiles land compactly at partial[((t - full_tiles) * ksplit + ks) * BM * BN]
    int slice_rr = 0;       // A/B only (emu_gemm_tune bit 1): deal the slice workgroups tile by tile round-robin over the XCDs
                            // (the order before round 3) instead of the XCD-aware slice-major order
    // ---- fused LayerNorm (UNet transformer blocks: removes the LayerNorm launch between two GEMMs)
    // Producer side: besides C, emit per-row partial (sum, sum of squares) of the bf16-rounded outputs, one pair per
    // 128-column slot: row_stats_out[(slot * M + m) * 2 + {0, 1}], slot = n / 128 (N % 128 == 0; EPI_NONE / EPI_RESID).
    float* row_stats_out = nullptr;
    // Consumer side: A holds the UN-normalised rows x [M, K], W holds W * gamma (bf16), and the epilogue computes
    //   out[m, n] = rstd_m * (acc[m, n] - mean_m * ln_c[n]) + ln_d[n]
    // with mean_m / rstd_m from the ln_slots partial pairs of row m (LayerNorm over the K columns of A, eps ln_eps),
    // ln_c[n] = sum_k float(W'[n, k]) and ln_d[n] = sum_k W[n, k] * beta[k] + bias[n] (fp32; `bias` must be null).
    const float* ln_c = nullptr;
    const float* ln_d = nullptr;
    const float* ln_stats = nullptr;
    int ln_slots = 0;
    float ln_eps = 0.f;
    // ---- V^T epilogue (self-attention qkv projection): output columns n >= vt_col0 are the V heads; instead of row-major C
    // they are stored key-contiguous for the P.V MFMA: vt_out[((b * (N - vt_col0) + (n - vt_col0)) * vt_spad) + s],
    // m = b * vt_s + s  (= [B, H, 64, S_pad] with H * 64 = N - vt_col0).  EPI_NONE only.
    bf16_t* vt_out = nullptr;
    int vt_col0 = 0, vt_s = 0, vt_spad = 0;
    // ---- cross-attention epilogue (UNet attn2 over <= 64 fixed context tokens): this GEMM is the to_q projection of head-dim-64
    // heads (N = heads * 64); instead of writing q, every wave runs the whole attention of its (32 queries, 1 head) tile
    // against the cached K rows / V^T of the prompt -- S = K q^T, softmax over the keys, O = V^T P -- and C receives the
    // attention output (what the flash kernel would have written), so neither q nor a second launch exists.  128 x 64 tile only.
    //   cross_k  [B * cross_n, cross_ldk] K rows of every batch element (head h at columns h * 64 ..)
    //   cross_vt [B, N / 64, 64, cross_npad] V^T, key-contiguous (zero beyond cross_n)
    //   rows m of batch element b = m / cross_rows; scores scaled by cross_scale
    const bf16_t* cross_k = nullptr;
    const bf16_t* cross_vt = nullptr;
    int cross_ldk = 0, cross_n = 0, cross_npad = 0, cross_rows = 0;
    float cross_scale = 0.f;
    int sup_m = 0, sup_n = 0;   // set by launch_gemm (lock-step tiles, unsplit launches): every XCD owns one sup_m x sup_n block of
                            // tiles instead of a run of the column-major order (fewer distinct A + W rows per L2); 0 = off
    int stage_vt = 0;       // set by launch_gemm: whole V^T tiles leave through the transposed staging (gemm_tile.h::EpiStageT)
    int stage = 0;          // set by launch_gemm: the staged (LDS-transposed, 16-byte coalesced) epilogue may be taken (gemm_tile.h)
    // ---- per-workgroup timeline (tools/gemm_trace.py; written only by a library built with -DEMU_TRACE): 8 x u64 per workgroup
    unsigned long long* trace = nullptr;
    // ---- LLaMA prefill qkv projection with RoPE, KV append and V^T in the epilogue (256x256 tile only; N = 3 * rope_hl * 128,
    // columns [q heads | k heads | v heads], ONE batch element whose rows sit at cache slots rope_slot[m] = m): q is rotated and
    // stored to C, k is rotated and stored to rope_kc[head][slot][128], v goes to rope_vc[head][slot][128] and, key-contiguous, to
    // vt_out (GemmArgs::vt_* as above, vt_col0 = 2 * rope_hl * 128).  Same arithmetic as rope_kv_kernel (attention.hip).
    const bf16_t* rope_cos = nullptr;   // [max_pos, 128]
    const bf16_t* rope_sin = nullptr;
    const int32_t* rope_pos = nullptr;  // [M] rope position of every row
    const int32_t* rope_slot = nullptr; // [M] cache slot of every row
    bf16_t* rope_kc = nullptr;          // [rope_hl, rope_smax, 128] of this layer and batch element
    bf16_t* rope_vc = nullptr;
    int rope_hl = 0, rope_smax = 0;
    // ---- K-sliced GEMM whose slice sum also applies the RMSNorm that follows (LLaMA prefill: o_proj -> post-attention norm,
    // down_proj -> the next layer's input norm; 256x256 tile with EVERY tile K-sliced): the fp32 slices are laid out row-major
    // over the whole output (partial[(ks * M + m) * N + n], slab_rows = 1) and ONE workgroup per row sums them in slice order,
    // applies the epilogue (C), and writes norm_out = bf16(norm_w * bf16(C * rsqrt(mean(C^2) + eps))) with rmsnorm_kernel's
    // arithmetic -- the reduce launch and the rmsnorm launch in one, bit-identical to the pair.  The K-sliced 256 x 128 lock-step
    // tile has the same form (ViT fc2 -> LayerNorm + residual).
    const bf16_t* norm_w = nullptr;     // [N]
    const bf16_t* norm_b = nullptr;     // [N] or null.  Non-null: LayerNorm (layernorm_kernel's arithmetic) instead of RMSNorm, and
    const bf16_t* norm_res = nullptr;   //   norm_out = bf16(norm_res + bf16(LN(C))) when norm_res is set (ViT post-norm block); C may be null then
    int norm_ldres = 0;
    bf16_t* norm_out = nullptr;         // [M, norm_ld]
    int norm_ld = 0;
    float norm_eps = 0.f;
    int slab_rows = 0;                  // set by launch_gemm
    // ---- successor prefetch: the weights of the launch that FOLLOWS this one on the stream (a model forward knows them).  Every
    // thread requests up to two 128-byte lines of [pf_ptr, pf_ptr + pf_bytes) -- one dword each, consecutive lines on consecutive
    // threads, results discarded -- ahead of its own first k tile, so the matrix travels HBM -> infinity cache while this GEMM runs
    // and the successor finds it there (a GEMM over weights last touched a whole denoise step ago starts 1.5-4.7 us late and stalls
    // on every k tile of a short K otherwise: profiles/r04_mall_prefetch_probe.log).  Used by the UNet's transformer blocks, whose
    // matrices (3-26 MB) fit the two lines per thread: same-run 25.07 -> 24.19 ms per denoise step.  NOT used where a matrix is larger
    // than that (ViT fc1 / fc2 55 MB, the LLaMA prefill): whole-matrix requests queue ahead of the wave's own first tile (ViT +4 %),
    // and a capped k-major cover of every row's first tiles measured +1 % (ViT) / +2 % (prefill) and only -2 % on the UNet
    // (scattered lines): profiles/r05_prefetch_ab_*.log.  nullptr = off; emu_gemm_tune bit 16 switches it off globally (A/B).
    const void* pf_ptr = nullptr;
    size_t pf_bytes = 0;
};
int launch_gemm(const GemmArgs& a, hipStream_t s);
// tools hook: where the next GEMM launches of a -DEMU_TRACE build write their per-workgroup timelines (nullptr = off)
void emu_gemm_trace_set(unsigned long long* buf);
unsigned long long* emu_gemm_trace_get();
void emu_gemm_trace_select(long n);     // trace only the n-th GEMM launch from now on (-1: every launch)
// fp8 x fp8 -> bf16 on the block-scaled MFMA (256x256 ping-pong tile only): K % 128 == 0, a.a_scale / a.w_scale set
int launch_gemm_fp8(const GemmArgs& a, hipStream_t s);
// One planned launch of launch_gemm / launch_gemm_fp8 (gemm.hip::plan_gemm; the C-ABI test hook emu_gemm_plan returns the same).
using GemmPlan = emu_gemm_plan_entry;
enum GemmReduce { GEMM_REDUCE_NONE = 0, GEMM_REDUCE_SPLITK = 1, GEMM_REDUCE_PP = 2, GEMM_REDUCE_ROWS_NORM = 3 };
// the 256x256 tile (gemm256.hip) for a planned launch: `b` carries the plan's fields; -22 if the form is not instantiated
int launch_gemm256(const GemmArgs& b, const GemmPlan& p, hipStream_t s);
// its four-wave main loop (gemm_w4.hip): grid workgroups, the caller launches the reduce; -22 if the form is not instantiated
int launch_gemm_w4(const GemmArgs& b, hipStream_t s, int grid);
int gemm256_tiles(const GemmArgs& a);           // workgroups of a whole-K launch (the last row of tiles carries M % 256 <= 32)
bool gemm256_ok(const GemmArgs& a);             // K % 64 == 0 and operands within reach of 32-bit descriptor offsets
constexpr size_t EMU_GEMM256_SLICE_FLOATS = 288 * 256;
// scratch that always suffices: at most 256 slices (one per CU) of the largest tile (256 x 256 + 32 remainder rows, fp32)
constexpr size_t EMU_SPLITK_SCRATCH_FLOATS = (size_t)512 * 288 * 256;
// process-wide default split-K scratch for callers that do not pass one (the C-ABI primitives); caller-owned memory
void emu_gemm_set_splitk_scratch(float* ptr, size_t floats);
// test / bench hook: pin the tile configuration ('B', 'C', 'K', 'S', 'P'; 0 = heuristic)
void emu_gemm_force_config_set(int cfg);
// A/B switches of single dispatch decisions (include/emu_hip.h: emu_gemm_tune)
void emu_gemm_tune_set(int mask);
int emu_gemm_tune_get();

// ---- launch profiler (engine.hip; bench.py's per-kernel table of the denoise leg): HIP events around the MFMA-carrying launches
// (GEMM / conv / attention) while enabled -- eager launches only.  klass: a short static string.
bool emu_prof_on();
void emu_prof_begin(hipStream_t s);
void emu_prof_end(hipStream_t s, const char* klass, int M, int N, int K, int tag, double flops);
void emu_prof_drop();                   // the wrapped launch returned non-zero (not launched: -95 probe, -22): record nothing

// ---- row-wise / elementwise (elementwise.hip)
int launch_rmsnorm(const bf16_t* x, const bf16_t* w, bf16_t* y, int rows, int cols, int ldx, int ldy, float eps, hipStream_t s);
// y = (res ? res : 0) + LayerNorm(x) * w + b       (ViT post-norm residual, eva_vit.py:298-300)
int launch_layernorm(const bf16_t* x, const bf16_t* w, const bf16_t* b, const bf16_t* res, bf16_t* y,
                     int rows, int cols, float eps, hipStream_t s);
// the same + per-row e4m3 quantisation of the bf16 result in one pass (cols <= 2048; y may be null): q [rows, cols] bytes, scale [rows]
int launch_layernorm_q8(const bf16_t* x, const bf16_t* w, const bf16_t* b, const bf16_t* res, bf16_t* y, uint8_t* q, float* scale,
                        int rows, int cols, float eps, hipStream_t s);
int launch_embed_gather(const int32_t* ids, const bf16_t* table, bf16_t* out, int n_tok, int hidden, int vocab, hipStream_t s);
// out[dst_rows[i], :] = src[i, :]
int launch_scatter_rows(const bf16_t* src, const int32_t* dst_rows, bf16_t* out, int n_rows, int hidden, hipStream_t s);
int launch_argmax(const bf16_t* logits, int ld, int rows, int vocab, int suppress_id, int32_t* out, hipStream_t s);
// sample.hip: emu_sample_bf16 / emu_sample_trie_bf16 / emu_sample_ngram_bf16 (include/emu_hip.h); trie and node both null = no
// constraint; ngram = the no-repeat n-gram size over hist, 0 = off
int launch_sample(const bf16_t* logits, int ld, int rows, int vocab, const int32_t* hist, int hist_ld, int hist_rows,
                  const int32_t* step_dev, const float* uniforms, int uni_ld, int uni_rows, const emu_sample_params* p,
                  int32_t* unfinished, int32_t* out, float* probs_out, int ld_probs, const emu_token_trie* trie, int32_t* node,
                  int ngram, hipStream_t s);
// score.hip: emu_token_logprob_bf16 (include/emu_hip.h).  limit > 0: nothing is written once *step_dev >= limit; force_ids (may be
// null): force_ids[row] = the row's target, 0 for an ignored one (emu_llama_score_step's next input)
int launch_token_logprob(const bf16_t* logits, int ld, int rows, int vocab, const int32_t* targets, int tgt_ld, const int32_t* step_dev,
                         int limit, const bf16_t* ref_logits, int ref_ld, float* lp, float* lse, int32_t* top1, float* kl,
                         int32_t* agree, int out_ld, int32_t* force_ids, hipStream_t s);
// NCHW fp32/bf16 image -> [B*gh*gw, Kpad] bf16 patch matrix (k = c*p*p + i*p + j, zero padded to Kpad)
int launch_patchify(const void* image, int image_is_f32, bf16_t* out, int B, int C, int HW, int p, int Kpad, hipStream_t s);
// tokens [B, 1+g*g, C] (cls dropped) -> [B, (g/s)^2, C] average over s x s windows (emu.py:82-89)
int launch_avgpool_tokens(const bf16_t* x, bf16_t* out, int B, int g, int C, int s, hipStream_t s_);
// x[b, 0, :] = cls + pos[0]; x[b, 1+t, :] = patches[b, t, :] + pos[1+t]   (eva_vit.py:406-409)
int launch_vit_assemble(const bf16_t* patches, const bf16_t* cls, const bf16_t* pos, bf16_t* x, int B, int T, int C, hipStream_t s);
int launch_vit_assemble_rows(const bf16_t* patches, const bf16_t* cls, const bf16_t* pos, bf16_t* x, int t0, int t1, int C, hipStream_t s);  // one image, rows [t0, t1)

// ---- image front / back end (image.hip)
struct ImageResampleArgs {
    const uint8_t* src;     // [H, W, 3] interleaved, rows `pitch` bytes apart
    long pitch;
    int H, W;
    const int32_t* hcoef;   // [S, hk] horizontal coefficients (22 fractional bits); unused when W == S
    const int32_t* hbounds; // [S, 2]  first tap, tap count
    int hk;
    const int32_t* vcoef;   // [S, vk], [S, 2]; unused when H == S
    const int32_t* vbounds;
    int vk;
    int row0, nrows;        // source rows the vertical pass reads: [row0, row0 + nrows)
    const float* lut;       // [3, 256] ToTensor + Normalize
    void* out;              // [3, S, S] bf16 or fp32
    int out_is_f32;
    int S;
    void* ws;               // image_resample_ws_bytes(H, W, S)
    size_t ws_bytes;
};
size_t image_resample_ws_bytes(int H, int W, int S);
int launch_image_resample_norm(const ImageResampleArgs& a, hipStream_t s);
// bf16 [N, C, H, W] in [0, 1] -> uint8 [N, H, W, C] = rint(x * 255) (C <= 4)
int launch_image_to_u8(const bf16_t* x, uint8_t* out, int N, int C, int H, int W, hipStream_t s);

// ---- attention (attention.hip)
struct RopeKvArgs {
    bf16_t* qkv;            // [B*T, 3*Hl*D] rows; q at col 0, k at Hl*D, v at 2*Hl*D  (q, k rotated in place)
    const bf16_t* cos;      // [max_pos, D] bf16 (cat(freqs, freqs) layout)
    const bf16_t* sin;
    const int32_t* pos;     // [B*T] rope position of every row
    const int32_t* slot;    // [B*T] kv-cache slot of every row (absolute index into S_max)
    bf16_t* kcache;         // [B, Hl, S_max, D]
    bf16_t* vcache;         // [B, Hl, S_max, D]
    int B, T, Hl, D, S_max;
};
int launch_rope_kv(const RopeKvArgs& a, hipStream_t s);

// Vt[b, h, d, s] = V[b, h, s, d] for s < S (zero for S <= s < S_pad); strided source.
// Memory contract (tests/test_gpu_flash_kernel.py): V rows >= S are not read; EVERY element of [S, S_pad) is written as zero, whole
// extra tiles included -- this launch is the producer of the zero pad launch_flash_attn relies on.  -22, nothing written: D not a
// multiple of 64, S_pad not a multiple of 64 or below S, a stride that is not a multiple of 8.
struct TransposeVArgs {
    const bf16_t* v; long v_sb, v_sh, v_ss;    // element strides (batch, head, token); d contiguous
    bf16_t* vt;                                // [B, H, D, S_pad]
    int B, H, S, D, S_pad;
};
int launch_transpose_v(const TransposeVArgs& a, hipStream_t s);

// softmax(q k^T scale + mask) v; query i of row b sees the keys kstart[b] <= key (and, causal, key <= i + (Sk - Sq)).
// Memory contract, pinned bit for bit by tests/test_gpu_flash_kernel.py:
//  - may hold anything (NaN patterns included), because it is either not read or selected away, never multiplied: the K rows of keys
//    < kstart[b]; Q rows >= Sq and K rows >= Sk (loads are clamped to the last row); V^T columns >= ceil64(Sk) (Sk_pad may be larger:
//    further tiles are never touched);
//  - must be FINITE: the V rows of masked keys (key < kstart[b], or behind the causal limit inside a tile that is read).  Their weight
//    is an exact zero, but the row does reach the P.V MFMA as 0 * v: any finite value gives the bits that zero gives, NaN / Inf do not;
//  - must be ZERO: the V^T pad [Sk, ceil64(Sk)) inside the last key tile (launch_transpose_v writes it);
//  - a query row with no visible key comes out as exact zeros (l = 0 -> 1 / l is replaced by 0), in every form;
//  - nothing outside o[B, Sq, H, D] (by its strides) is written, by staged and by direct stores alike.
// -22, nothing written: Sq < 1, Sk < 1, Sk_pad not a multiple of 64 or below Sk, D not 64 / 128, a q / k stride that is not a
// multiple of 8, an o stride that is not a multiple of 4 (a multiple of 4 but not of 8, or an o that is not 16-byte aligned: direct stores).
struct FlashArgs {
    const bf16_t* q; long q_sb, q_sh, q_ss;    // element strides; d contiguous
    const bf16_t* k; long k_sb, k_sh, k_ss;
    const bf16_t* vt;                          // [B, H, D, Sk_pad]
    bf16_t* o; long o_sb, o_sh, o_ss;
    const int32_t* kstart;                     // [B] or null: keys < kstart[b] are masked (left padding)
    int B, H, Sq, Sk, Sk_pad, D;               // D in {64, 128}
    int causal;                                // query i attends keys <= i + (Sk - Sq)
    float scale;
    int xcd_remap = 1;                         // set by launch_flash_attn: XCD-aware (head, query block) order
    int stage_o = 0;                           // set by launch_flash_attn: O leaves through LDS as 16-byte row-contiguous stores
    int heavy_first = 0;    // set by launch_flash_attn: causal prefill, XCDs walk their heads' query blocks from the longest down
};
int launch_flash_attn(const FlashArgs& a, hipStream_t s);

// Two-segment flash attention (attention_prefix.hip), D = 128: query i of row b attends the prefix keys [kstart, P) -- one K / V^T per
// head, common to all B rows -- and its row's own keys j <= i + (Sk - Sq).  flash_kernel's tile arithmetic; prefix tiles first.
struct FlashPrefixArgs {
    const bf16_t* q; long q_sb, q_sh, q_ss;    // [B, H, Sq, D] by element strides; d contiguous
    const bf16_t* kp; long kp_sh, kp_ss;       // prefix K [H, P, D]
    const bf16_t* vtp;                         // prefix V^T [H, D, P_pad], zero padded
    const bf16_t* ko; long ko_sb, ko_sh, ko_ss; // own K [B, H, Sk, D]
    const bf16_t* vto;                         // own V^T [B, H, D, Sk_pad], zero padded
    bf16_t* o; long o_sb, o_sh, o_ss;
    const int32_t* kstart_dev;                 // device int32 [>= 1] or null: element 0 overrides kstart (the engine's left-pad count)
    int kstart;                                // prefix keys < kstart are masked; 0 <= kstart < P
    int B, H, Sq, P, P_pad, Sk, Sk_pad, D;
    float scale;
};
int launch_flash_attn_prefix(const FlashPrefixArgs& a, hipStream_t s);

struct DecodeAttnArgs {
    const bf16_t* q; long q_sb, q_sh;          // [B, H, D] strided
    const bf16_t* kcache;                      // [B, H, S_max, D]
    const bf16_t* vcache;
    bf16_t* o; long o_sb, o_sh;
    const int32_t* kstart;                     // [B] or null
    const int32_t* ctx_ptr;                    // device int32 or null: overrides ctx (graph replay)
    float* ws;                                 // workspace: B*H*nsplit*(D+2) floats
    int B, H, D, S_max, ctx;                   // keys [0, ctx) valid
    int ctx_max;                               // sizes the launch (>= ctx); 0 -> ctx
    float scale;
};
int decode_attn_nsplit(int ctx);
// out_ids[step, b] = cur_ids[b] (out_ids may be null); pos[b]++, slot[b]++; ctx++, step++   (greedy loop state, all on device).
// limit > 0: nothing happens once step >= limit (the teacher-forced loop, whose replays past the end must change no state)
int launch_greedy_advance(const int32_t* cur_ids, int32_t* pos, int32_t* slot, int32_t* ctx, int32_t* step,
                          int32_t* out_ids, int B, int limit, hipStream_t s);
int launch_decode_attn(const DecodeAttnArgs& a, hipStream_t s);
// out_all[step[0]] = prev = src ([B, cols] bf16); pos[b]++, slot[b]++, step[0]++   (generate_image's loop state, on the device)
int launch_regress_advance(const bf16_t* src, bf16_t* out_all, bf16_t* prev, int32_t* pos, int32_t* slot, int32_t* step, int B,
                           int cols, hipStream_t s);
// Step bookkeeping of the hipGraph-replayed beam and contrastive loops, from the device counter c = step_dev[0].  phase 0 (ahead of
// the decoder step): slot[i] = slot0 + c + bias, pos[i] = pos0[i] + c + bias for the `rows` rows; phase 1 (behind the step's last
// kernel): c += 1.  bias = -1: the step feeds token c - 1 (beam search); 0: it runs the candidates of token c (contrastive
// search).  From c >= L on nothing changes (replays beyond the length limit are no-ops).
int launch_step_advance(int32_t* step_dev, int32_t* pos, int32_t* slot, const int32_t* pos0, int slot0, int bias, int rows, int L,
                        int phase, hipStream_t s);

// Decode step, fused: RoPE of q and of the new k, KV-cache append of the new token, and single-query attention over
// the cache, in one launch (+ the split combine).  Context length of row b = slot[b] + 1, read on the device.
struct DecodeFusedArgs {
    const bf16_t* qkv;                         // [B, 3*H*D] projection rows (q | k | v), not yet rotated
    const bf16_t* cos; const bf16_t* sin;      // [max_pos, D]
    const int32_t* pos;                        // [B] RoPE position of the new token
    const int32_t* slot;                       // [B] cache slot of the new token
    bf16_t* kcache; bf16_t* vcache;            // [B, H, S_max, D]
    bf16_t* o; long o_sb, o_sh;
    const int32_t* kstart;                     // [B] or null
    float* ws;                                 // decode_fused_ws_floats(B, H, D, ctx_max)
    int B, H, D, S_max, ctx_max;               // ctx_max sizes the launch (>= max slot + 1)
    float scale;
    // Beam search: rows come in groups of share_nb beams of one prompt whose first share_len cache slots (the prompt) are
    // identical.  They are stored ONCE, in the group's first row, and read from there by every beam of the group (the
    // workgroups reading the same keys are dispatched onto one XCD so its L2 serves all but the first).  share_nb <= 1:
    // every row owns all of its slots.
    int share_nb = 0, share_len = 0;
    // Non-null (one-row path only): the last split workgroup of a head to arrive merges the head's live splits itself
    // (arrive[b * H + h]: zero between launches, the merging workgroup resets it) -- no decode_fused_combine_kernel launch.
    int* arrive = nullptr;
    // one-row path: leave the split states in ws and launch no combine -- the consumer merges them itself (launch_gemv_merge)
    bool skip_combine = false;
    // one-row launches (B == 1) with the combine launch: extra workgroups behind its H merging ones request the head of the launch
    // that follows (l2_warm.h; make_warm_plan with extra = true, pred_wgs = H, lanes = D).  ntouch == 0: none.
    WarmPlan warm;
};
constexpr int DECODE_SHARE_MAX = 8;            // beams per group the shared-prefix path takes
size_t decode_fused_ws_floats(int B, int H, int D, int ctx_max);
int launch_decode_fused(const DecodeFusedArgs& a, hipStream_t s);

// Chunk step (prompt-lookup speculative decoding): B sequences of T rows each (2 <= T <= DECODE_CHUNK_MAX) on top of the cache.  Row i
// of sequence b sits at cache slot slot0[b] + i and RoPE position pos0[b] + i and sees the keys kstart[b] <= key <= slot0[b] + i.
// One launch rotates the T queries and new keys, appends the T K / V rows and forms every row's 128-key split states with the
// arithmetic and summation order of the one-row path (a split's cache rows are loaded once for all T queries); the one-row path's
// combine launch merges them.  Row i's output and the cache rows have the bits of T successive launch_decode_fused calls.
struct DecodeChunkArgs {
    const bf16_t* qkv;                         // [B*T, 3*H*D] projection rows (q | k | v), not yet rotated
    const bf16_t* cos; const bf16_t* sin;      // [max_pos, D]
    const int32_t* pos0;                       // [B] RoPE position of row 0
    const int32_t* slot0;                      // [B] cache slot of row 0 (slot0 + T <= ctx_max: the caller's reservation)
    bf16_t* kcache; bf16_t* vcache;            // [B, H, S_max, D]
    bf16_t* o; long o_sb, o_sh;                // o[(b*T + i)*o_sb + h*o_sh + d]
    const int32_t* kstart;                     // [B] or null
    float* ws;                                 // decode_chunk_ws_floats(B, T, H, D, ctx_max)
    int B, T, H, D, S_max, ctx_max;            // ctx_max sizes the launch (>= max slot0 + T)
    float scale;
};
constexpr int DECODE_CHUNK_MAX = 8;
size_t decode_chunk_ws_floats(int B, int T, int H, int D, int ctx_max);
int launch_decode_chunk(const DecodeChunkArgs& a, hipStream_t s);

// Prompt-lookup speculative greedy decoding, one sequence (lookup.hip; what is computed: emu_amd/speculate.py).  st: the loop's
// scalars on the device, indexed by LOOKUP_*.
enum { LOOKUP_STEP = 0, LOOKUP_FINISHED = 1, LOOKUP_NDRAFT = 2, LOOKUP_HIST_LEN = 3, LOOKUP_STEPS_RUN = 4, LOOKUP_EMITTED = 5, LOOKUP_STATE_INTS = 8 };
struct LookupArgs {
    const bf16_t* logits; int ld, V;           // [T, V] rows of the chunk step
    int T;                                     // rows = 1 + k
    int32_t* amax;                             // [T] scratch: the rows' arg-maxes
    int32_t* cur;                              // [T] ids the next step feeds: the last emitted id, then the draft (0 beyond n_draft)
    int32_t* st;                               // [LOOKUP_STATE_INTS]
    int32_t *pos0, *slot0, *ctx;               // [1] each
    int32_t* out_ids;                          // [max_new]
    int32_t* hist; int hist_cap;               // the prompt's real ids followed by the generated ones
    const int32_t* drafts;                     // [max_new, T - 1] or null: row `step` replaces the lookup (tests, timing)
    int max_ngram, max_new, min_len, eos_id, stop_on_eos;
};
int launch_lookup_argmax(const LookupArgs& a, hipStream_t s);
int launch_lookup_select(const LookupArgs& a, hipStream_t s);
// sample.hip: the place of launch_lookup_argmax when the loop samples or penalises (emu_lookup_sample_bf16): one sampler workgroup
// per chunk row, amax[i] = the id row i picks as output index step + i with uniforms[min(step + i, uni_rows - 1)]; reads cur, st and
// out_ids.  lookup_sample_ok: what it takes (the vocabulary bound, the options, uniforms when sampling).
bool lookup_sample_ok(int vocab, const emu_sample_params* p, const float* uniforms, int uni_rows);
int launch_lookup_sample(const LookupArgs& a, const emu_sample_params* p, const float* uniforms, int uni_rows, hipStream_t s);

struct EmuP2p;
// ---- whole decoder layers of a single-row decode step in ONE launch (decode_layer.hip): qkv projection (+RMSNorm) -> RoPE / KV
// append / split attention + merge -> o_proj (+residual) -> [all-reduce] -> gate/up (+RMSNorm, SwiGLU) -> down (+residual) ->
// [all-reduce], for layers [layer0, layer0 + nlayers).  Workgroups are dealt roles by index (in dispatch order: every dependency
// points to a lower index), wait on arrival counters with their weight slice already requested, and hand results over with
// agent-scope (write-through) stores; every wait is bounded in wall-clock time (err counts give-ups; results are garbage then).
struct DecodeLayerPtrs { const bf16_t *wqkv, *wo, *wgu, *wdown, *ln1, *ln2; };
struct DecodeLayersArgs {
    const DecodeLayerPtrs* table;              // device memory, indexed by absolute layer
    int layer0, nlayers;
    bf16_t* hA;                                // [H] layer input / output (residual stream)
    bf16_t* hB;                                // [H] post-attention residual stream
    bf16_t* qkv;                               // [3 * Hl * 128]
    bf16_t* attn;                              // [Hl * 128]
    bf16_t* act;                               // [Fl]
    float* ws;                                 // decode_fused_ws_floats(1, Hl, 128, ctx_max)
    const bf16_t* cos; const bf16_t* sin;
    const int32_t* pos; const int32_t* slot; const int32_t* kstart;
    bf16_t* kcache; bf16_t* vcache;            // layer l at + l * kv_layer elements: [Hl, S_max, 128]
    size_t kv_layer;
    int H, Hl, Fl, S_max, ctx_max;
    float eps, scale;
    int epi_res;                               // 1: this rank adds the residual (rank 0, or no tensor parallelism)
    int* cnt;                                  // decode_layers_cnt_ints(layers, Hl) ints, ZERO at launch (all layers of the table)
    unsigned* err;                             // give-up counter (device)
    long long limit_ticks;                     // wait bound, 100 MHz ticks
    // tensor parallelism: the workgroup that completes o_proj / down_proj all-reduces the partial vector over the peers' comm
    // blocks (p2p.hip's protocol and sequence counters) before the consumers are released.  tp_n == 0: no all-reduce.
    char* tp_block[8];
    unsigned long long* tp_seq;
    int tp_n, tp_rank;
    // roles [role0, role1) of every layer run in this launch (0 q, 1 attention, 2 o_proj, 3 gate/up, 4 down; 0, 0 = all).  A partial
    // range covers ONE layer; its first role's input comes from the launch before (tensor parallelism without in-kernel all-reduce:
    // [q, attention, o_proj] -> all-reduce launch -> [gate/up, down] -> all-reduce launch).
    int role0, role1;
    unsigned long long* trace;                 // tools only (nullptr = off): 4 x u64 per workgroup {role | layer << 8, entry, input ready, exit}
    // set by launch_decode_layers
    int nQ, nA, nO, nG, nD, per_layer, cnt_stride, wave_od;
};
size_t decode_layers_cnt_ints(int layers, int Hl);
bool decode_layers_ok(const DecodeLayersArgs& a);
int launch_decode_layers(DecodeLayersArgs a, hipStream_t s);
// the comm blocks / sequence counters of an opened EmuP2p for DecodeLayersArgs::tp_* (false: peers not mapped)
bool emu_p2p_view(EmuP2p* p, char** block8, unsigned long long** seq, int* n, int* rank, long long* limit_ticks);
// the engine area of every mapped comm block (decode_engine.hip's in-launch all-reduce) and this rank's per-CU counters
bool emu_p2p_engine_view(EmuP2p* p, char** area8, unsigned int** seq, int* n, int* rank);

// ---- persistent weight-streaming engine for chains of one-row GEMVs (decode_engine.hip): one launch, one resident workgroup per CU
// (loader wave + three consumer waves on an LDS ring), op outputs handed between CUs through 4-byte {tag, bf16} granules
constexpr int ENG_MAX_OPS = 6;
constexpr int EMU_ENG_MAX_RANKS = 8;
constexpr int ENG_AR_BUFS = 4;                 // comm arrays per rank, reused round-robin (an array is rewritten four all-reduces later)
constexpr int ENG_AR_MAXLEN = 8192;            // granules per comm array
constexpr size_t EMU_P2P_ENG_BYTES = (size_t)ENG_AR_BUFS * ENG_AR_MAXLEN * 4;   // engine area at the end of every P2P comm block
struct EngOp {
    const bf16_t* W;                           // [N, K] row-major, K contiguous, K <= 6656
    int N, K;
    const bf16_t* gain;                        // RMSNorm gain [K] (fused prologue on the activation vector) or null
    float eps;
    int epi;                                   // EPI_NONE / EPI_RESID / EPI_SWIGLU (rows (2j, 2j + 1) = (gate_j, up_j))
    const bf16_t* res;                         // [N] (EPI_RESID)
    int vw;                                    // launch_gemv's column partition for this shape: 4 (block kernels) or 1 (wave kernel)
    // input vector: 0 = xg, a bf16 vector written BEFORE this launch; 1 = xgran, granules of an earlier op of this launch;
    // 2 = the tensor-parallel SUM of an earlier op's partial outputs: every CU reduces its share of the ranks' comm arrays (ar_k-th
    // all-reduce of the launch) in rank order (p2p.hip's arithmetic), publishes it to xgran, and gathers xgran like case 1
    int x_src;
    const bf16_t* xg;
    uint32_t* xgran;
    bf16_t* sum_out;                           // x_src 1 / 2: the gathered vector also goes here as plain bf16 (read by LATER launches), or null
    int keep_raw;                              // the gathered (un-normalised) vector stays in LDS for a later op's residual (res_src = 1)
    // output vector: 0 = out, plain bf16 (read by a LATER launch); 1 = ogran, granules (zero at launch); 2 = this rank's comm array
    // of the ar_k-th all-reduce of the launch (partial sums, read by every rank's reducers)
    int out_dst;
    bf16_t* out;
    uint32_t* ogran;
    int ar_k;                                  // out_dst 2 / x_src 2: which all-reduce of this launch
    int res_src;                               // EPI_RESID: 0 = res (global, written before this launch); 1 = the vector kept by keep_raw
    // set by launch_decode_engine: units (rows, or (gate, up) pairs) per CU = q (+ 1 for the first rem CUs), whole rows per 16 KiB fill,
    // bytes / LDS-DMA instructions per fill, fills that go to one consumer together, fills per CU (q / q + 1 units)
    int q, rem, rps, fill_bytes, ni, grp, nfills_lo, nfills_hi;
};
struct EngArgs {
    EngOp op[ENG_MAX_OPS];
    int nops;
    unsigned* err;                             // give-up counter (device)
    long long limit_ticks;                     // bound of every wait, 100 MHz ticks
    int ncu;                                   // workgroups = CUs of the device (all must be resident)
    // tensor parallelism (tp_n >= 1 with all-reduce ops): every rank's engine area inside its P2P comm block (p2p.hip), ENG_AR_BUFS
    // arrays of ar_len granules used round-robin by the all-reduces in launch order (a per-CU device counter numbers them: the tag)
    char* comm[EMU_ENG_MAX_RANKS];
    int tp_n, tp_rank, n_ar, ar_len;
    unsigned int* seq;                         // [ncu] all-reduces this CU has been through (device memory, owned by the comm block's creator)
    int nload;                                 // loader waves per workgroup (0 = default)
    int dbg;                                   // tools: bit 0 = consumers acknowledge fills without multiplying (loader ceiling)
    int nslot, xbytes;                         // set by launch_decode_engine
};
int launch_decode_engine(EngArgs a, hipStream_t s);
// the same plan's column partition (the engine mirrors it bit for bit): 1 = gemv_wave_kernel (one wave per row), 4 = the 256-thread
// block and single-round-trip kernels
int emu_gemv_partition(int N, int K, bool norm, int epi);

// One beam-search step on the device (beam.hip): see emu_beam_step_bf16 in include/emu_hip.h
struct BeamStepArgs {
    const bf16_t* logits;                      // row of (prompt b, beam j) = logits + b * ld_prompt + j * ld_beam
    long ld_prompt, ld_beam;                   // elements (step 0: ld_beam = 0, every beam continues the prompt)
    int V, B, nb, L, cur;                      // vocabulary, prompts, beams, max new tokens, tokens generated so far
    const int32_t* cur_dev;                    // non-null: the step index is read here instead (hipGraph replay); steps >= L are no-ops
    int min_len, eos_id;                       // EOS is masked while cur < min_len
    float length_penalty;
    int hf431;                                 // scorer conventions: 0 = transformers 5.x, 1 = transformers 4.31 (beam.hip)
    int32_t* running_seq; int32_t* sequences;  // [B, nb, L]
    float* running_scores; float* beam_scores; // [B, nb]
    unsigned char* finished; int32_t* seq_len; // [B, nb]
    unsigned char* heuristic_open;             // [B]
    int32_t* next_tok; long* beam_flat;        // [B * nb] out: token to feed / cache row it continues
    emu_token_trie trie = {};                  // constraint (emu_beam_step_trie_bf16), read only when node is set
    int32_t* node = nullptr;                   // [B * nb] in/out: the beams' trie nodes; null = no constraint
    int ngram = 0;                             // no-repeat n-gram size over running_seq[b, j, :cur] (ngram.h); 0 = off
};
// KV re-order of a hipGraph-replayed beam step (beam.hip)
int launch_beam_reorder(bf16_t* kc, bf16_t* vc, const long* beam_flat, const int32_t* cur_dev, int layers, int rows, int Hl, int s_max,
                        int D, int nb, int slot0, int L, hipStream_t s);
size_t beam_step_ws_floats(int B, int nb, int V);     // scratch of the two-launch step (chunk partials)
int launch_beam_step(const BeamStepArgs& a, float* ws, size_t ws_floats, hipStream_t s);
// One step of beam-search sampling / penalised beam search (beam_sample.hip): see emu_beam_sample_step_bf16 in include/emu_hip.h
struct BeamSampleArgs {
    BeamStepArgs st;                           // the step's logits, limits and state, as for launch_beam_step
    float penalty;                             // repetition penalty over running_seq[b, j, :cur]; 1 = off
    int do_sample; float temperature; int top_k; float top_p; int min_keep;
    int warp_accumulated;                      // 1: the warpers act on lp + running score and the draws are sorted ("4.31" order)
    const float* uniforms; int uni_rows;       // [uni_rows, B, 2 * nb]; the step's row is min(cur, uni_rows - 1)
    int32_t* draws_out;                        // optional [B, 2 * nb]: flat indices in draw order
    float* acc_out; long ld_acc;               // optional [B * nb] rows of V accumulated scores, ld_acc apart
};
size_t beam_sample_ws_floats(int B, int nb, int V);   // per row: the scores, their masses, the row maximum
int launch_beam_sample_step(const BeamSampleArgs& a, float* ws, size_t ws_floats, hipStream_t s);

// Contrastive search on the device (contrastive.hip): see emu_contrastive_pick_bf16 / emu_contrastive_score in include/emu_hip.h
struct ContrastivePickArgs {
    const bf16_t* logits; int ld; int vocab;   // [B * k] rows ld apart; prompt b reads row b * k + sel[b]
    int B, k, L;                               // prompts, candidates, max new tokens (steps >= L are no-ops)
    const int32_t* sel;                        // [B] or null (= 0)
    const int32_t* hist; int hist_ld;          // ids generated so far: hist[t * hist_ld + b], t < step; may be null
    const int32_t* step;                       // device int32[1]
    float penalty; int eos_id, min_len;        // EOS is masked while step < min_len
    int32_t* cand_ids; float* cand_p;          // [B * k] out
};
int launch_contrastive_pick(const ContrastivePickArgs& a, hipStream_t s);
struct ContrastiveScoreArgs {
    float* ctx_n;                              // [B, Lc, H] fp32 normalised context rows; row S + step is appended
    const bf16_t* cand;                        // [B * k, H] final-normed rows of the candidates
    const int32_t* cand_ids; const float* cand_p;
    const int32_t* kstart;                     // [B] first valid context row, or null (= 0)
    const int32_t* step;
    int B, k, H, S, L, Lc;
    float alpha, one_minus_alpha;
    int eos_id, pad_id;
    int32_t* out_ids; int32_t* unfinished; int32_t* sel; float* pen_out;
    float* ws; int nchunks;                    // per (prompt, chunk) partial maxima; nchunks is set by the launcher
};
size_t contrastive_ws_floats(int B, int k, int Lc);
int launch_contrastive_score(ContrastiveScoreArgs a, size_t ws_floats, hipStream_t s);
int launch_contrastive_keep(bf16_t* kc, bf16_t* vc, const int32_t* sel, const int32_t* step_dev, int layers, int rows, int Hl, int s_max,
                            int D, int k, int slot0, int L, hipStream_t s);

// ---- UNet denoise helpers (unet.hip); activations are NHWC: [B, H*W, C] bf16
// GroupNorm(groups, eps) (+ optional SiLU) over x [B, HW, C]: three launches (partial sums, finalize to per-(b, c)
// scale/shift, apply).  ws must hold gn_ws_floats(B, C, HW) floats.
size_t gn_ws_floats(int B, int C, int HW);
int launch_groupnorm(const bf16_t* x, const bf16_t* gamma, const bf16_t* beta, bf16_t* y, float* ws, int B, int HW, int C,
                     int groups, float eps, int silu, hipStream_t s);
// out[m, :C1] = a[m, :], out[m, C1:] = b[m, :]
int launch_concat_channels(const bf16_t* a, const bf16_t* b, bf16_t* out, int rows, int C1, int C2, hipStream_t s);
// latents NCHW [1, C, H, W] -> conv_in im2col matrix [2*H*W, Kpad] (both CFG halves identical), scaled by
// 1/sqrt(sigma[step]^2 + 1) (EulerDiscreteScheduler.scale_model_input); k = (ky*3 + kx)*C + c, zero padded
int launch_unet_prep_input(const bf16_t* latents, const float* sigmas, const int32_t* step, bf16_t* out, int C, int H, int W,
                           int Kpad, hipStream_t s);
// classifier-free guidance (cond first) + Euler step on NCHW latents, then step++ :
//   eps = u + g*(c - u); x += eps * (sigma[step+1] - sigma[step])   with the bf16 rounding points of the reference ops
int launch_cfg_euler_step(const bf16_t* eps_nhwc, bf16_t* latents, const float* sigmas, int32_t* step, float guidance, int C,
                          int HW, hipStream_t s);
// out[r, :] = bf16(silu(bf16(a[r, :] + b[r, :])))   (silu(emb + aug_emb) feeding every time_emb_proj)
int launch_add_silu(const bf16_t* a, const bf16_t* b, bf16_t* sum_out, bf16_t* silu_out, int n, hipStream_t s);
// out[r, :] = table[step[0], :] for r < rows
int launch_gather_step_row(const bf16_t* table, const int32_t* step, bf16_t* out, int rows, int cols, hipStream_t s);

// stand-alone touch (l2_warm.h::warm_touch): [ptr, ptr + bytes) -> infinity cache and the XCDs' L2s, workgroups x 256 threads
int launch_prefetch(const void* ptr, size_t bytes, int workgroups, hipStream_t s);
// in-place row softmax of x [rows, ld] over the first `cols` columns: x = bf16(softmax(float(x) * scale))
// (materialised-score attention for head dims the flash kernel does not cover: the VAE mid block, D = 512)
// per-row fp8 e4m3fn quantisation: scale[n] = amax_n / 448 (1 for an all-zero row), q = rne(w / scale)
int launch_quant_fp8_rows(const bf16_t* w, int ldw, uint8_t* q, int ldq, float* scale, int N, int K, hipStream_t s);
int launch_softmax_rows(bf16_t* x, const bf16_t* bias, int rows, int cols, int ld, int ld_bias, float scale, hipStream_t s);

// ---- one-shot peer-to-peer all-reduce over IPC-mapped comm blocks (p2p.hip)
constexpr int EMU_P2P_MAX_RANKS = 8;
constexpr size_t EMU_P2P_SLOT_BYTES = 256 * 1024;
// a message is cut into pieces of EMU_P2P_PIECE elements, each with its own sequence counter and flag per slot; the comm block is
// [slot 0 | slot 1 | flags: 2 x EMU_P2P_PIECES x u64]
constexpr int EMU_P2P_PIECE = 512 * 8;
constexpr int EMU_P2P_PIECES = (int)(EMU_P2P_SLOT_BYTES / (EMU_P2P_PIECE * 2));
struct EmuP2p;
EmuP2p* emu_p2p_create(int rank, int n, void* handle64_out);          // nullptr on failure
int emu_p2p_open(EmuP2p* p, const void* handles);                      // n x 64 bytes, rank order (own entry ignored)
void emu_p2p_destroy(EmuP2p* p);
void emu_p2p_set_timeout_ms(EmuP2p* p, int ms);
void emu_p2p_set_fenced(EmuP2p* p, int fenced);                        // 1 (default): system-scope fences around the exchange; 0: fence-free form
int emu_p2p_fenced(const EmuP2p* p);
int emu_p2p_allreduce(EmuP2p* p, bf16_t* x, size_t n, hipStream_t s);  // in place; > one slot goes through in chunks
unsigned int emu_p2p_giveups_read();
// ViT token-row exchange (p2p.hip, emu_vit_forward_tp): every rank's exchange region holds two sets [A: a_elems | B: wb x ldb] bf16
// + flags; one launch publishes my rows [rows[rank], rows[rank + 1]) of the token-major A and my 8-key groups of the token-minor B
// (null: none) and pulls every peer's rows into my local A / B.  Same protocol, give-up counter and forms as the all-reduce.
constexpr int VITX_PIECES = 64;
struct EmuVitX;
EmuVitX* emu_vitx_create(int rank, int n, size_t a_elems, int wb, int ldb, void* handle64_out);   // n >= 2; nullptr on failure
int emu_vitx_open(EmuVitX* p, const void* handles, int timeout_ms, int fenced);
void emu_vitx_destroy(EmuVitX* p);
int emu_vitx_exchange(EmuVitX* p, const int* rows, bf16_t* a, int lda, int wa, bf16_t* b, int ldb, hipStream_t s);
