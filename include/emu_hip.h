/* emu_hip.h -- C ABI of libemu_hip.so, the MI355X (gfx950) compute library behind emu_amd.
 *
 * The reference (baaivision/Emu, Emu2/) has no FFI layer: its hot path is Python calling torch /
 * transformers / diffusers ops.  This header is the operator interface those call sites bind to when the
 * arithmetic is replaced by hand-written HIP kernels; every entry cites the reference lines it replaces
 * (paths relative to the reference root).  INTEGRATION.md shows the ctypes stubs.
 *
 * Conventions
 *  - plain C symbols, raw device pointers + sizes, no torch types; bf16 tensors are `uint16_t` bit patterns,
 *    row-major, innermost dimension contiguous; all "ld*"/stride arguments are in ELEMENTS.
 *  - every launch takes an explicit HIP stream (`emu_stream_t` = hipStream_t) and is asynchronous;
 *    nothing here allocates, frees or synchronises device memory (hipGraph / stream-capture safe).
 *  - return value: 0 = OK, negative = -errno style (-22 = EINVAL: unsupported shape/alignment),
 *    positive = hipError_t / ncclResult_t (offset by 1000) of the failing runtime call.
 *  - one context per (process, device); thread-compatible, not thread-safe per context.
 *  - the caller owns all tensors (e.g. torch allocator); the library owns only its small host-side tables.
 */
#ifndef EMU_HIP_H
#define EMU_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* emu_stream_t;
typedef struct emu_ctx emu_ctx;
typedef struct emu_llama emu_llama;
typedef struct emu_vit emu_vit;

enum { EMU_EPI_NONE = 0, EMU_EPI_RESID = 1, EMU_EPI_SWIGLU = 2, EMU_EPI_SILU = 3, EMU_EPI_GELU = 4, EMU_EPI_GEGLU = 5 };

/* ---- context / tensor-parallel communicator ------------------------------------------------------------
 * Replaces the reference's layer-placement "model parallel" (Emu2/emu/mixin.py:14-85, chat.py:235-283): the
 * decoder is tensor-parallel, one process per GPU, partial sums exchanged with RCCL all-reduce over xGMI. */
int emu_version(void);
int emu_ctx_create(int device, int tp_rank, int tp_size, emu_ctx** out);
void emu_ctx_destroy(emu_ctx* ctx);
const char* emu_last_error(const emu_ctx* ctx);
int emu_tp_unique_id(void* out128);                      /* rank 0: 128-byte RCCL unique id           */
int emu_tp_init(emu_ctx* ctx, const void* id128);        /* all ranks: ncclCommInitRank               */
int emu_allreduce_bf16(emu_ctx* ctx, void* buf, size_t n, emu_stream_t s);   /* in-place sum          */
/* One-shot peer-to-peer all-reduce for the decode-sized messages (13 KB, 120 per token), emu_amd/csrc/p2p.hip: every rank
 * exports a comm block over HIP IPC (create: 64-byte handle out), maps every peer's (open: tp_size x 64 bytes in rank
 * order; timeout_ms bounds every device-side wait, <= 0 keeps the 10 s default), and reads the peers' partial vectors
 * straight over xGMI.  emu_allreduce_bf16 uses it for messages of at most 256 KiB once emu_tp_p2p_enable(ctx, 1) was
 * called (and for every message when no RCCL communicator exists); the host enables it only after a self-test through
 * emu_tp_p2p_allreduce_bf16 on every rank.  emu_tp_p2p_giveups: device-side waits that timed out since process start --
 * non-zero means sums since then are invalid. */
int emu_tp_p2p_create(emu_ctx* ctx, void* handle64_out);
int emu_tp_p2p_open(emu_ctx* ctx, const void* handles, int timeout_ms);
int emu_tp_p2p_allreduce_bf16(emu_ctx* ctx, void* buf, size_t n, emu_stream_t s);
int emu_tp_p2p_enable(emu_ctx* ctx, int on);
/* The exchange has two forms: fenced = 1 (the state of a fresh comm block) brackets it with system-scope release / acquire fences --
 * the HIP memory model's own guarantee --; fenced = 0 relies on write-through stores + acknowledgement and cache-bypassing loads alone
 * (3.3 instead of 6.8 us per 13 KB all-reduce).  The host selects 0 only after a soak of that form passed on every rank of the job
 * (emu_amd/llama.py::_init_p2p).  emu_tp_p2p_fenced: the current form (-1: no comm block). */
int emu_tp_p2p_set_fenced(emu_ctx* ctx, int fenced);
int emu_tp_p2p_fenced(const emu_ctx* ctx);
unsigned int emu_tp_p2p_giveups(void);

/* Optional fp32 scratch for split-K GEMMs / convolutions issued through the primitives below (emu_linear_bf16,
 * emu_conv3x3_nhwc_bf16): few-tile long-K problems are cut into up to 4 K-slices that land here before a second launch
 * applies the epilogue.  Caller-owned device memory, >= 4 * M * N * 4 bytes for the shapes that should split; NULL / 0
 * (the default) never splits.  One stream at a time may use it.  The UNet engine carries its own inside its workspace. */
void emu_set_splitk_scratch(void* ptr, size_t bytes);
/* Test / bench hook: pin the tile configuration of every following GEMM / conv launch of this process.  0 (default) =
 * the shape heuristic; 'B' 128x128, 'C' 256(n)x128(m), 'K' 128x64 with two k-groups, 'S' 256x128 K-sliced,
 * 'P' 256x256 ping-pong (K-sliced under half a round of tiles), 'Q' the same never sliced (both: K % 64 == 0 and
 * operands within 2 GiB, else the heuristic), 'H' whole rounds of the 256x256 tile + the remaining columns as a second
 * GEMM (where the tile count allows, else the heuristic).  The parity tests walk every configuration over the
 * bench's true shapes with it (tests/test_gpu_ops.py); production code never calls it. */
void emu_gemm_force_config(int cfg);
/* CPU test hook (tests/test_gemm_plan.py): what launch_gemm / launch_gemm_fp8 would launch for a problem of this shape under
 * force_cfg (emu_gemm_force_config) and tune (emu_gemm_tune) -- host arithmetic only, no HIP call, no global read.  The shape
 * stands for an argument block with row-contiguous operands (lda = ldw = K, or Cin for a conv; ldc = N, N / 2 for the GLU
 * epilogues) on aligned buffers.  fx: 1 LayerNorm folded into A (ln_*), 2 row statistics of C (row_stats_out), 4 V^T (vt_*),
 * 8 cross-attention (cross_*), 16 RoPE + KV append (with 4), 32 RMSNorm of C in the reduce (norm_*); rows: rows per batch
 * element of the V^T / cross-attention forms (0: M).  Fills *entries (two only for the hybrid split: whole rounds of the 256x256
 * tile, then the remaining columns) and returns launch_gemm's status: 0, -22 (refused), -95 (fused form not available). */
typedef struct {
    int M, N, K, epi;
    int conv_mode, Hin, Win, Hout, Wout, Cin;
    int fx, rows, vt_col0, fp8;
    size_t scratch_floats;      /* split-K scratch; 0 = none */
} emu_gemm_shape;
typedef struct {
    int tile;                   /* 'B' 128x128, 'C' 256(n)x128(m), 'K' 128(n)x64(m) with two k-groups, 256: the 256x256 tile */
    int w4;                     /* tile 256: the four-wave kernel (gemm_w4.hip) instead of the eight-wave ping-pong one */
    int col0, n;                /* output columns [col0, col0 + n) of this launch */
    int full_tiles, ksplit;     /* tiles [0, full_tiles) whole-K, every later tile in ksplit K-slices */
    int sup_m, sup_n;           /* XCD tile blocks (0: column-major runs) */
    int stage, stage_vt, slab_rows, slice_rr;   /* the GemmArgs flags of the same names */
    int no_prefetch;            /* the successor-weight prefetch is dropped */
    int reduce;                 /* the launch after it: 0 none, 1 split-K reduce, 2 256x256 slice reduce, 3 rows + norm */
} emu_gemm_plan_entry;
int emu_gemm_plan(const emu_gemm_shape* shape, int force_cfg, int tune, emu_gemm_plan_entry plan[2], int* entries);
/* CPU test hook (tests/test_gemv_plan.py): what launch_gemv (emu_linear_bf16 and its fp8 / MXFP4 twins at 1..16 rows) would launch
 * for an argument block of this shape under tune (emu_gemm_tune) -- host arithmetic only, no HIP call, no global read.  norm: fused
 * RMSNorm; fp8 / fp4: the weight kind (neither: bf16; ldw in elements of it, bytes for MXFP4; lds: the MXFP4 scale row stride);
 * w_aligned / x_aligned: W / x on a 16-byte boundary.  The plan: family 0 block kernel, 1 single round trip, 2 wave, 3 register-fed
 * MFMA, 4 thin LDS-DMA stream, 5 fp8 block kernel, 6 fp8 single round trip, 7 MXFP4 rows; form (one-row bf16 / fp8 round trip):
 * 0 rolling loop, 1 head, 2 preload, 3 single round trip, 4 wave; rows: weight rows per workgroup (grid = ceil(N / rows)); mb: the
 * built activation-row count; waves per workgroup (block = 64 * waves); trips: the block kernel's PRE, the round trip's KIT, the
 * wave form's KITW; stages / kch: the thin stream's ring depth and 16-byte slots per row and stage; vb: bytes per fp8 weight load;
 * tpr / row_sets / rpl: MXFP4 threads per row set, row sets per workgroup, weight rows per lane; partition: 1 one wave per row,
 * 4 thread t owns 16-byte columns t, t + 256, ... (0: neither).  Returns the status launch_gemv would: 0 or -22 (then the other
 * fields are 0). */
typedef struct {
    int M, N, K, ldx, ldw, lds, epi;
    int norm, fp8, fp4, w_aligned, x_aligned;
} emu_gemv_shape;
typedef struct {
    int status, family, form, rows, mb, waves, trips;
    int stages, kch, vb, tpr, row_sets, rpl;
    int grid, block, partition;
} emu_gemv_plan_t;
int emu_gemv_plan(const emu_gemv_shape* shape, int tune, emu_gemv_plan_t* out);
/* CPU test hook (tests/test_thin_plan.py): the one planner of the three few-row weight streams on the matrix cores -- what the
 * 3..16-row steps of a generation (emu_linear_fp8w_thin_bf16, emu_linear_fp4w_mfma_bf16 / emu_linear_fp4w_thin_bf16 up to 16 rows,
 * and emu_linear_bf16 where emu_gemv_plan answers family 4) launch for an argument block of this shape under tune -- host arithmetic
 * only.  The shape's fp8 / fp4 flags pick the weight kind (both: refused).  In the plan, family is 4 (bf16), 8 (fp8) or 9 (MXFP4);
 * rows: weight rows per workgroup (16 / 32; grid = ceil(N / rows)); mb: the built activation-row bucket (8 up to 8 rows, else 16);
 * stages: depth of the LDS ring; kch: 16-byte slots per staged weight row (bf16 32 / 64, fp8 16, MXFP4 8; a stage is kch * 8 * 2 /
 * bytes-per-weight = 256 k, 512 for kch 64); waves 4, block 256; the other fields 0.  LDS bytes of the ring: stages * (rows + mb) *
 * kch * 16 (bf16), stages * (rows * 256 + mb * 512) (fp8), stages * (rows * 128 + mb * 512 + 1024) (MXFP4, whose instantiation with
 * a partial last stage is the one launched iff K % 256 != 0).  tune: bits 8-11 (bf16 variants) and 28-29 (fp8 / MXFP4: 1 / 2 pin
 * 16 / 32 weight rows); no other bit is read -- bit 2 is emu_gemv_plan's routing.  Returns 0, or -22 (then the other fields are 0):
 *   bf16   M outside 2..16, K < 256 or K % 256 != 0, ldw % 8 or ldx % 8 != 0, an epilogue outside NONE .. GELU;
 *   fp8    M outside 1..16, K < 256 or K % 256 != 0, ldw % 16 or ldx % 8 != 0, a stride below K, an epilogue other than NONE /
 *          RESID / SWIGLU;
 *   MXFP4  M outside 1..16, K < 256 or K % 32 != 0, ldw % 16, ldx % 8 or lds % 4 != 0, ldw < K / 2, ldx < K, lds below 8 bytes per
 *          started 256-wide stage (K / 32 where K % 256 == 0), an epilogue other than NONE / RESID / SWIGLU;
 *   all    N < 1, a fused norm, W or x off a 16-byte boundary, an odd N under SWIGLU. */
int emu_gemv_thin_plan(const emu_gemv_shape* shape, int tune, emu_gemv_plan_t* out);
/* CPU test hook (tests/test_pack_thin_plan.py): the plan of the 13-bit packed twin of the bf16 few-row stream (family 4 above) for
 * a set of set_rows (2 / 4) rows per group -- what emu_linear_bf16pack_thin and the engine's 4..16-row steps under
 * emu_llama_use_bf16_pack_wide launch.  Succeeds exactly when emu_gemv_plan sends the shape (bf16, no fused norm) to family 4 with
 * a kch that has a twin (32), set_rows is 2 or 4, 4 <= M <= 16 and the epilogue is NONE / RESID / SWIGLU.  The plan: family 10;
 * mb 8 / 16; kch 32; waves 4, block 256; (rows = weight rows per workgroup, stages) one of the built tiles, listed with the
 * workgroups that share a CU's LDS -- mb 8: (16, 4: 3), (32, 4: 2), (16, 6: 2), (32, 3: 3); mb 16: (16, 3: 3), (32, 3: 2), (16, 5: 2) --
 * namely the one whose grid = ceil(N / rows) fills the largest share of its whole rounds of 256 x (workgroups per CU) places, the
 * first of equals in that order; tune bits 28-29 = 1 / 2 leave only the tiles of 16 / 32 rows; the other fields 0.  LDS bytes: the
 * larger of stages * (rows / 4 + rows / 8 + 1 + mb / 2) KiB and the bf16 ring of a flagged workgroup, 3 stages of (rows + mb) * 512
 * bytes where they fit the former, else 2.  Returns 0, or -22 (then the other fields are 0). */
int emu_gemv_pack_thin_plan(const emu_gemv_shape* shape, int set_rows, int tune, emu_gemv_plan_t* out);
/* The older view of the fp8 branch of emu_gemv_thin_plan (tests/test_fp8_wide_host.py): M rows over an fp8 matrix [N, K] (ldx in bf16
 * elements, ldw in bytes) on aligned buffers.  rows, mb, stages, grid, block: the plan's; kc = 256: k per stage; lds_bytes = stages *
 * (rows * kc + mb * kc * 2).  Returns 0, or -22 (then the other fields are 0). */
typedef struct {
    int status, rows, mb, kc, stages, lds_bytes, grid, block;
} emu_gemv_fp8_thin_plan_t;
int emu_gemv_fp8_thin_plan(int M, int N, int K, int ldx, int ldw, int epi, int tune, emu_gemv_fp8_thin_plan_t* out);
/* CPU test hook (tests/test_fp8_mid_host.py): what emu_linear_fp8w_gemm_bf16 and the engine's 17..64-row steps under fp8 modes 5 / 6
 * launch (gemm_fp8.hip) for M rows over an fp8 matrix [N, K] (ldx in bf16 elements, ldw in bytes) on aligned buffers -- host arithmetic
 * only.  form: 1 narrow (64 weight rows x 32 activation rows, M 17..32), 2 one tile (64 x 64, M 33..64); bm: activation rows of the
 * tile (32 / 64); kc = 256: k per stage; stages: depth of the LDS ring (narrow 4, one tile 3; tune bit 20 (emu_gemm_tune): narrow 2,
 * which lets two workgroups share a CU's LDS); lds_bytes = stages * (64 * kc + bm * kc * 2), at most 160 KiB; grid = ceil(N / 64);
 * block 256.  Returns 0, or -22 (then the other fields are 0): M outside 17..64, N < 1, K < 256 or K % 256 != 0, ldw % 16 or
 * ldx % 8 != 0, a stride below K, an epilogue other than NONE / RESID / SWIGLU, an odd N under SWIGLU. */
typedef struct {
    int status, form, bm, kc, stages, lds_bytes, grid, block;
} emu_gemm_fp8w_plan_t;
int emu_gemm_fp8w_plan(int M, int N, int K, int ldx, int ldw, int epi, int tune, emu_gemm_fp8w_plan_t* out);
/* CPU test hook (tests/test_fp8_all_host.py): what emu_linear_fp8w_tile_bf16 and the engine's calls of 65 rows and more under
 * emu_llama_use_fp8_all launch (gemm_fp8.hip, the third form of the same kernel) -- host arithmetic only.  form 3: a workgroup owns 64
 * weight rows x bm = 128 activation rows (four waves 2 x 2, a converted weight fragment feeds four MFMAs); kc = 256: k per stage;
 * stages 2: the LDS ring; lds_bytes = stages * (64 * kc + bm * kc * 2) = 163840, a CU's whole LDS; grid_x = ceil(M / 128) walks the
 * row tiles (the workgroups in flight share weight rows in L2), grid_y = ceil(N / 64) the column tiles; block 256.  tune: no bit is
 * read.  Returns 0, or -22 (then the other fields are 0): M < 65, more than 65535 column tiles, and whatever emu_gemm_fp8w_plan
 * refuses apart from the row count. */
typedef struct {
    int status, form, bm, kc, stages, lds_bytes, grid_x, grid_y, block;
} emu_gemm_fp8t_plan_t;
int emu_gemm_fp8t_plan(int M, int N, int K, int ldx, int ldw, int epi, int tune, emu_gemm_fp8t_plan_t* out);
/* Bench hook: A/B switches of single dispatch decisions (0 = the shipped heuristic).  Bits 0, 4, 5, 14, 17 and 18: retired,
 * ignored.  Bit 1: the K-slice workgroups of a split GEMM are dealt tile by tile round-robin over the XCDs (the order before
 * round 3) instead of the XCD-aware slice-major order.  Bit 2: 4..16-row linears skip the LDS-DMA + MFMA stream (gemv_thin.hip)
 * and run on the v_dot2c / register-fed MFMA kernels as before round 3; bit 3: the GEMM / conv epilogues store straight from the
 * accumulator layout (8 bytes per lane to 32 rows per instruction, as before round 4) instead of through the LDS-staged,
 * row-contiguous 16-byte form; bit 6: the attention kernel deals its workgroups in launch order (query blocks of a head on 8
 * different XCDs); bit 7: it stores O straight from the accumulator layout; bits 12-13: 1 / 2 = attention always on 4 / 8 waves;
 * bit 15: causal attention launches keep the (head, query block) order instead of walking every XCD's heads from the longest query
 * block down; bits 8-11: variant of the thin stream (tools/thin_ab.py); bit 16: no successor-weight prefetch from inside the GEMM
 * kernels; bit 20: the narrow form of the fp8 W8A16 GEMM (gemm_fp8.hip, 17..32 rows) runs a ring of 2 stages instead of 4, so that
 * two workgroups share a CU's LDS (tools/fp8_mid_time.py --ab); bit 19 (opt-in): a short tensor-parallel shard's one-row step merges the decode attention's splits in the o_proj
 * launch's prologue instead of a combine launch ahead of it (gemv_merge.hip: bit-identical, measured level);
 * bits 21-23 (round 6, the four-wave 256x256 tile of gemm_w4.hip): 21 = never take it (the eight-wave ping-pong
 * tile everywhere: the same-run A/B twin), 22 = take it wherever it is instantiated (tests: bf16 plain GEMMs and convs of the
 * 256x256 configuration, whatever epilogue, slices and raggedness), 23 = its fp32 K-slices leave by direct stores instead of
 * through LDS; bits 24-25 (the MXFP4 weight stream, gemv_fp4.hip; tools/fp4_time.py --ab): 1 / 2 / 3 = 1 / 2 / 4 row sets per
 * workgroup instead of the planned number, bits 26-27: 1 / 2 = 4 / 8 weight rows per lane; bits 28-29 (the few-row MXFP4 stream,
 * gemv_fp4_thin.hip; tools/fp4_wide_time.py --ab) and the few-row fp8 stream (gemv_fp8_thin.hip; tools/fp8_wide_time.py --ab): 1 / 2 =
 * 16 / 32 weight rows per workgroup instead of the heuristic;
 * bit 17 (tests): one-row bf16 streams skip the wave and single-round-trip forms, so a small matrix reaches the block kernel's head /
 * preload form; bit 30: no L2 warming anywhere (emu_llama_set_l2_warm's plans are all empty: the same-build twin of a warmed run). */
void emu_gemm_tune(int mask);

/* Tools hook (tools/gemm_trace.py): per-workgroup timelines of the following GEMM launches -- 8 x uint64 per workgroup at
 * buf[blockIdx * 8]: entry, first k tile landed, main loop done, stores complete (s_memrealtime, 100 MHz), XCC / HW id, shader
 * clock at entry / loop end, unused.  Written only by a library built with -DEMU_TRACE (`python -m emu_amd.build --trace` ->
 * libemu_hip_trace.so; emu_gemm_trace_built() says which one is loaded); NULL = off.  The production library ignores it. */
void emu_gemm_trace(void* buf);
void emu_gemm_trace_nth(long n);     /* trace only the n-th GEMM / conv launch from now on (a launch INSIDE a model's forward); -1: all */
int emu_gemm_trace_built(void);

/* Measurement hook (bench.py roofline leg): HIP-event timing of every M<=8 weight-streaming GEMV launched while
 * enabled (eager launches only, not inside stream capture).  read: sum of launch durations (ms), algorithmic
 * weight bytes (2*N*K per launch) and launch count since the last enable. */
int emu_profile_gemv(int enable);
int emu_profile_gemv_read(double* total_ms, double* weight_bytes, long* launches);

/* Measurement hook (bench.py: per-kernel table of the denoise leg): HIP events around every MFMA-carrying launch -- GEMM, implicit-
 * GEMM convolution, attention -- issued while enabled (eager launches only, not inside stream capture).  read: the launches since
 * the last enable, aggregated by (class, M, N, K, tag): klass "gemm" / "conv" / "attn"; for attn M = Sq, N = Sk, K = head dim and
 * tag = batch x heads; for gemm / conv tag = epilogue | fused-epilogue mask << 8.  Returns the number of rows written (<= cap). */
typedef struct {
    char klass[16];
    int M, N, K, tag, launches;
    double ms, flops;
} emu_prof_row;
int emu_profile_launches(int enable);
int emu_profile_launches_read(emu_prof_row* rows, int cap);

/* ---- primitive operators -------------------------------------------------------------------------------*/
/* torch.nn.functional.linear on the hot path (eva_vit.py:106,112,198,250; LlamaAttention/LlamaMLP linears
 * reached from emu.py:133-138,213-229; project_up/down emu.py:53,55,131,147,201).
 * C[m,n] = epi(sum_k A[m,k] W[n,k] (+bias[n])).  M <= 8 streams W once (HBM-bound GEMV, optional fused
 * LLaMA RMSNorm of A via norm_w/eps); M > 8 runs the MFMA GEMM (norm_w must be NULL).
 * EPI_RESID: C = bf16(res + bf16(.)).  EPI_SWIGLU/GEGLU: W rows interleaved (2j, 2j+1), C has N/2 columns. */
int emu_linear_bf16(const void* A, const void* W, const void* bias, const void* res, const void* norm_w,
                    void* C, int M, int N, int K, int lda, int ldw, int ldres, int ldc, float eps, int epi,
                    emu_stream_t s);
/* emu_linear_bf16 with an fp8 (e4m3fn) weight stream: W8 [N, ldw] bytes, wscale fp32 [N]; M <= 2, K % 16 == 0,
 * epi in {NONE, RESID, SWIGLU}.  out = epi(bf16((sum_k fp8(W8[n,k]) * x[k]) * wscale[n] + bias[n])) */
int emu_quantize_fp8_rows(const void* w_bf16, int ldw, void* q_fp8, int ldq, float* scale, int N, int K,
                          emu_stream_t s);   /* scale[n] = amax_n / 448 (1 if the row is zero); q = rne_e4m3fn(w / scale) */
/* fp8 x fp8 GEMM on the block-scaled matrix instruction (v_mfma_scale_f32_32x32x64_f8f6f4, twice the bf16 MFMA rate) for
 * the MFMA-bound shapes of BASELINE configs[4] ("fp8 MFMA weights"): A8 [M, lda] and W8 [N, ldw] hold OCP e4m3fn bytes
 * (both from emu_quantize_fp8_rows: one fp32 scale per row), K % 128 == 0, lda / ldw % 16 == 0.
 *   C[m, n] = epi(bf16(a_scale[m] * w_scale[n] * sum_k fp8(A8[m,k]) * fp8(W8[n,k]) + bias[n]))   (fp32 accumulation)
 * epi in {NONE, RESID, SWIGLU, GELU, GEGLU}.  Not a reference feature (the reference computes in bf16). */
int emu_linear_fp8_bf16(const void* A8, const float* a_scale, const void* W8, const float* w_scale, const void* bias,
                        const void* res, void* C, int M, int N, int K, int lda, int ldw, int ldres, int ldc, int epi,
                        emu_stream_t s);
int emu_linear_fp8w_bf16(const void* A, const void* W8, const float* wscale, const void* bias, const void* res,
                         const void* norm_w, void* C, int M, int N, int K, int lda, int ldw, int ldres, int ldc,
                         float eps, int epi, emu_stream_t s);
/* The same weights for 1 <= M <= 16 rows on the matrix cores (gemv_fp8_thin.hip: LDS-DMA stages, the e4m3 bytes converted to bf16
 * in registers -- lossless --, v_mfma_f32_16x16x32_bf16, fp32 accumulation; the activations stay bf16):
 *   C[m, n] = epi(bf16(wscale[n] * sum_k fp8(W8[n,k]) * A[m,k] + bias[n]))
 * epi in {NONE, RESID, SWIGLU}; the row scale is multiplied in fp32 ahead of the bias, the sum is rounded to bf16 after the bias, then
 * the residual is added or SiLU(gate) * up formed (the rounding points of the bf16 few-row stream; they may differ in the last bit from
 * emu_linear_fp8w_bf16's kernel).  No fused RMSNorm (normalise first).  N >= 1, K >= 256 and K % 256 == 0, ldw % 16 == 0 (bytes),
 * lda % 8 == 0, both at least K, A / W8 16-byte aligned, N even under SWIGLU; anything else -22, nothing is launched and nothing
 * falls back.  emu_linear_fp8w_bf16 keeps answering -22 for M > 2.  Not a reference feature. */
int emu_linear_fp8w_thin_bf16(const void* A, const void* W8, const float* wscale, const void* bias, const void* res, void* C,
                              int M, int N, int K, int lda, int ldw, int ldres, int ldc, int epi, emu_stream_t s);
/* The same product, arguments, epilogues, rounding points and requirements for 17 <= M <= 64 rows (gemm_fp8.hip: a workgroup owns 64
 * weight rows x 32 / 64 activation rows, every converted weight fragment feeds 2 or 4 MFMAs; ragged M and N; emu_gemm_fp8w_plan names
 * the launch).  M outside 17..64 and every violated requirement: -22, nothing is launched.  It computes what emu_linear_bf16 computes
 * on the dequantised weights, up to fp32 summation order.  emu_linear_fp8w_thin_bf16 keeps answering -22 for M > 16.  Not a reference
 * feature. */
int emu_linear_fp8w_gemm_bf16(const void* A, const void* W8, const float* wscale, const void* bias, const void* res, void* C,
                              int M, int N, int K, int lda, int ldw, int ldres, int ldc, int epi, emu_stream_t s);
/* The same product, arguments, epilogues, rounding points and requirements for M >= 65 rows (the third form of gemm_fp8.hip's kernel:
 * a workgroup owns 64 weight rows x 128 activation rows, every converted weight fragment feeds four MFMAs, grid = row tiles x column
 * tiles, at most 65535 of the latter; ragged M and N; emu_gemm_fp8t_plan names the launch).  Every output element sums the same 32-k
 * products in the same order as in emu_linear_fp8w_gemm_bf16's 64 x 64 form, so a row's result is that call's, bit for bit, and does
 * not depend on how many rows share the call.  M < 65 and every violated requirement: -22, nothing is launched.
 * emu_linear_fp8w_gemm_bf16 keeps answering -22 for M > 64.  No fused RMSNorm, no RoPE epilogue, no K-slicing.  Not a reference
 * feature. */
int emu_linear_fp8w_tile_bf16(const void* A, const void* W8, const float* wscale, const void* bias, const void* res, void* C,
                              int M, int N, int K, int lda, int ldw, int ldres, int ldc, int epi, emu_stream_t s);
/* MXFP4 (OCP microscaling) weights, the 4-bit weight-only stream; emu_amd/mxfp4.py is the definition of the format.
 *   elements  uint8 [N, K/2]: element 2j in the low nibble of byte j, 2j+1 in the high nibble; a code is a sign bit (8) and an
 *             E2M1 magnitude index into {0, 0.5, 1, 1.5, 2, 3, 4, 6}
 *   scales    uint8 [N, K/32], E8M0: one per 32 consecutive elements of a row, 2^(byte - 127)
 * emu_quantize_mxfp4_rows: round-to-nearest of a bf16 matrix [N, ldw], K % 32 == 0, ldq % 16 == 0.  Per block, amax > 0:
 * e = floor(log2(amax)) - 2 clamped to [-126, 125], magnitudes rounded to the nearest grid point of w / 2^e (ties to the even code,
 * above 6 saturates), sign kept; an all-zero block gets byte 127; byte 255 is never produced.  Non-finite weights: -22 (the call
 * waits for its own result, so it must not be issued into a stream capture).
 * emu_linear_fp4w_bf16: emu_linear_bf16 over such a weight, M <= 2 and K % 32 == 0 (else -22), ldw in bytes (% 16 == 0), epi in
 * {NONE, RESID, SWIGLU}, optional bias and fused RMSNorm (norm_w, eps) as emu_linear_fp8w_bf16:
 *   out = epi(bf16(sum_k fp4(W4[n,k]) * 2^(scales[n,k/32] - 127) * x[k] + bias[n]))   (fp32 accumulation, scale applied per block)
 * emu_linear_fp4w_thin_bf16: the same product for 1 <= M <= 16 rows on the matrix cores (gemv_fp4_thin.hip: LDS-DMA stages, the block
 * scale applied by v_cvt_scalef32_pk_bf16_fp4, v_mfma_f32_16x16x32_bf16, fp32 accumulation), same epilogues and rounding points, no
 * fused RMSNorm (normalise first).  N >= 1, K >= 256 and K % 256 == 0, ldw % 16 == 0 (bytes), lda % 8 == 0, lds % 4 == 0, A / W4
 * 16-byte aligned, N even under SWIGLU; anything else -22.  emu_linear_fp4w_bf16 keeps answering -22 for M > 2.
 * emu_linear_fp4w_gemm_bf16: the same product, arguments, epilogues, rounding points and requirements for M >= 17 rows
 * (gemm_fp4.hip: a workgroup owns 64 weight rows x 32 / 64 / 128 activation rows, every converted weight fragment feeds 2 or 4
 * MFMAs; ragged M and N); M < 17 and every violated requirement: -22.  It computes what emu_linear_bf16 computes on the
 * dequantised weights, up to fp32 summation order.
 * emu_linear_fp4w_mfma_bf16: the same product, arguments, epilogues and rounding points for every M >= 1 (the kernel of
 * emu_linear_fp4w_thin_bf16 up to 16 rows, that of emu_linear_fp4w_gemm_bf16 above, the same tiles) and every K >= 256 with
 * K % 32 == 0: a K that is no multiple of 256 ends in a partial stage of (K % 256) / 32 blocks; nothing is read past a row's K
 * elements and nothing past K contributes.  Both kernels fetch a K stage's 8 scale bytes per row by 4-byte DMA, so a scale row must
 * span whole stages: lds % 4 == 0 and lds >= K / 32 where K % 256 == 0, else lds >= 8 * ceil(K / 256) (K = 896: 32, K = 2240: 72;
 * emu_amd/mxfp4.py::scale_stride / pad_scales).  The bytes past K / 32 are read and never used, whatever they are.  With
 * K % 256 == 0 it runs the two entry points above, bit for bit; they keep refusing any other K.
 * Not a reference feature; what round-to-nearest MXFP4 does to a trained checkpoint is NOT measured by this project. */
int emu_quantize_mxfp4_rows(const void* w_bf16, int ldw, void* q, int ldq, void* scales, int lds, int N, int K, emu_stream_t s);
int emu_linear_fp4w_bf16(const void* A, const void* W4, const void* scales, const void* bias, const void* res,
                         const void* norm_w, void* C, int M, int N, int K, int lda, int ldw, int lds, int ldres, int ldc,
                         float eps, int epi, emu_stream_t s);
int emu_linear_fp4w_thin_bf16(const void* A, const void* W4, const void* scales, const void* bias, const void* res, void* C, int M, int N,
                              int K, int lda, int ldw, int lds, int ldres, int ldc, int epi, emu_stream_t s);
int emu_linear_fp4w_gemm_bf16(const void* A, const void* W4, const void* scales, const void* bias, const void* res, void* C, int M, int N,
                              int K, int lda, int ldw, int lds, int ldres, int ldc, int epi, emu_stream_t s);
int emu_linear_fp4w_mfma_bf16(const void* A, const void* W4, const void* scales, const void* bias, const void* res, void* C, int M, int N,
                              int K, int lda, int ldw, int lds, int ldres, int ldc, int epi, emu_stream_t s);
/* emu_linear_bf16 (M > 8, epi in {NONE, RESID, GEGLU}) with the fused epilogues of the UNet transformer blocks -- what
 * diffusers' BasicTransformerBlock computes as LayerNorm -> Linear (norm1/2/3 ahead of attn1.to_q/k/v, attn2.to_q,
 * ff.net.0.proj; Emu2/emu/diffusion.py:136-141), without a LayerNorm launch in between:
 *   row_stats_out  producer side: besides C, per-row partial (sum, sum of squares) of the bf16 outputs, one fp32 pair per
 *                  128-column slot: row_stats_out[(slot * M + m) * 2 + {0,1}], slot = n / 128   (N % 128 == 0)
 *   ln_c/ln_d/ln_stats/ln_slots/ln_eps  consumer side: A is the UN-normalised activation, W = W0 * gamma, and
 *                  C[m,n] = epi(bf16(rstd_m * (sum_k A[m,k] W[n,k] - mean_m * ln_c[n]) + ln_d[n])) with mean / rstd of row m
 *                  from its ln_slots (= K / 128 <= 10) partial pairs, ln_c[n] = sum_k W[n,k], ln_d[n] = sum_k W0[n,k] beta[k] + bias[n]
 *   vt_out/vt_col0/vt_s/vt_spad  output columns n >= vt_col0 (the V heads of a fused qkv projection) are stored
 *                  key-contiguous, vt_out[(b * (N - vt_col0) + n - vt_col0) * vt_spad + s] for row m = b * vt_s + s,
 *                  instead of row-major (what the attention kernel's P.V MFMA reads; replaces a transpose launch)
 *   cross_k/cross_vt/...  this GEMM is attn2.to_q (head dim 64, N = heads * 64, no bias) and its epilogue runs the whole
 *                  cross-attention over the <= 64 cached context tokens: C receives softmax(q K^T * cross_scale) V per head
 *                  (what the attention kernel would have written from q), q itself is never stored.  cross_k [B * cross_n,
 *                  cross_ldk] K rows (head h at columns h * 64), cross_vt [B, heads, 64, cross_npad] V^T (zero beyond cross_n),
 *                  batch element of row m = m / cross_rows (cross_rows % 64 == 0).  Combines with ln_* only.
 * All pointers optional (NULL = feature off). */
typedef struct {
    float* row_stats_out;
    const float* ln_c;
    const float* ln_d;
    const float* ln_stats;
    int ln_slots;
    float ln_eps;
    void* vt_out;
    int vt_col0, vt_s, vt_spad;
    const void* cross_k;
    const void* cross_vt;
    int cross_ldk, cross_n, cross_npad, cross_rows;
    float cross_scale;
} emu_linear_fx;
int emu_linear_fused_bf16(const void* A, const void* W, const void* bias, const void* res, void* C, int M, int N, int K,
                          int lda, int ldw, int ldres, int ldc, int epi, const emu_linear_fx* fx, emu_stream_t s);

/* LlamaRMSNorm (transformers; emu.py:133-138): y = bf16(w * bf16(x * rsqrt(mean(x^2) + eps))) */
int emu_rmsnorm_bf16(const void* x, const void* w, void* y, int rows, int cols, int ldx, int ldy, float eps,
                     emu_stream_t s);
/* nn.LayerNorm + post-norm residual (eva_vit.py:298-300): y = (res ? res + : ) bf16(LN(x) * w + b) */
int emu_layernorm_bf16(const void* x, const void* w, const void* b, const void* res, void* y, int rows,
                       int cols, float eps, emu_stream_t s);
/* The same in one pass with the per-row e4m3 quantisation of the bf16 result (emu_quantize_fp8_rows' definition: scale = amax / 448,
 * 1 for a zero row), bit-identical to the two launches: q [rows, cols] bytes, scale [rows]; y may be null; cols <= 2048.  The
 * LayerNorm in front of a GEMM of the W8A8 modes (emu_vit_use_fp8, emu_unet_use_fp8) hands over the GEMM's fp8 operand itself. */
int emu_layernorm_q8_bf16(const void* x, const void* w, const void* b, const void* res, void* y, void* q, float* scale, int rows,
                          int cols, float eps, emu_stream_t s);
/* in-place row softmax x = bf16(softmax(x * scale [+ bias])) over [rows, cols] (row stride ld): materialised-score
 * attention for the VAE mid block (AutoencoderKL attention, 1 head of 512; Emu2/emu/diffusion.py:216) and, with the additive
 * bf16 bias [rows, cols] (relative-position bias + causal mask), T5Attention of Emu1's CausalFormer
 * (Emu1/models/modeling_t5.py:629-666) */
int emu_softmax_rows_bf16(void* x, const void* bias, int rows, int cols, int ld, int ld_bias, float scale, emu_stream_t s);
/* A chain of one-row projections  y_i = epi_i(W_i . norm_i(x_i))  in ONE persistent launch (emu_amd/csrc/decode_engine.hip: a loader
 * wave per CU streams every op's weights through an LDS ring ahead of the activations, op outputs cross the chip as 4-byte
 * granules): the LlamaDecoderLayer linears of a decode step (transformers, reached from Emu2/emu/emu.py:213-229) between two
 * all-reduces of a tensor-parallel shard.  x_i is either a bf16 vector written before the call (x_from_prev = 0) or the output of
 * op i - 1 (x_from_prev = 1; that op's output then exists only as granules in `granules`, caller-owned device memory of
 * emu_gemv_chain_granule_bytes(ops, nops) bytes, zeroed by this call).  Bit-identical to the same ops through emu_linear_bf16.
 * K <= 6656, N >= 2 x CUs, at most 6 ops; -95 = shape not covered (use the launches); err: device counter of bounded waits that gave
 * up (non-zero = invalid results).  Needs the device to itself (one resident workgroup per CU). */
typedef struct {
    const void* W; int N, K;
    const void* gain; float eps;       /* fused RMSNorm on the input vector, or NULL */
    int epi;                           /* EMU_EPI_NONE / EMU_EPI_RESID / EMU_EPI_SWIGLU */
    const void* res;                   /* [N] for EMU_EPI_RESID */
    const void* x;                     /* [K] input vector (x_from_prev = 0) */
    int x_from_prev;
    void* out;                         /* [N] (SWIGLU: N / 2) bf16, or NULL when the next op takes it (x_from_prev = 1 there) */
} emu_chain_op;
size_t emu_gemv_chain_granule_bytes(const emu_chain_op* ops, int nops);
int emu_gemv_chain_bf16(emu_ctx* ctx, const emu_chain_op* ops, int nops, void* granules, size_t granule_bytes, unsigned int* err,
                        emu_stream_t s);
/* Touch [ptr, ptr + bytes) -- the weight matrix of a launch that FOLLOWS on the stream -- into the 256 MB infinity cache with
 * `workgroups` x 256 threads, one dword per 128-byte line, nothing waited for.  The stand-alone form of the successor prefetch the
 * one-row decode step can carry inside its own launches (emu_llama_set_l2_warm): the reference's nn.Linear weights
 * (transformers LlamaDecoderLayer reached from Emu2/emu/emu.py:213-229) are read once per token, and every kernel of a layer that
 * leaves HBM idle (attention, split merge, all-reduce) pulls the next projection's rows on-die meanwhile.  tools / tests. */
int emu_prefetch(const void* ptr, size_t bytes, int workgroups, emu_stream_t s);

/* ---- L2 warming across a kernel boundary (csrc/l2_warm.h has the story).  emu_warm_plan is the plan as it travels in the
 * kernel-argument segment: toucher workgroups [first, first + ntouch) of the predecessor request 128-byte lines of the successor,
 * each from a workgroup of the reader's linear id % xcds.  emu_l2_warm_plan_make: the host planner (successor: `rows` rows of
 * row_bytes stride per workgroup, used_bytes read per row, nrows rows -- per group when gx > 0: gx blocks per group, `groups` groups;
 * twin: byte distance to a second array of the same geometry or 0; predecessor: pred_wgs working workgroups whose last ones touch, or
 * with extra != 0 ntouch workgroups behind them; shape 0 = whole blocks, 1 = the first 4 KiB of every row).  An empty plan has
 * ntouch == 0.  emu_l2_warm_enumerate: byte offsets (from base) of the lines workgroup wg requests, through the function the kernels
 * run; returns their number (offsets may be NULL, at most cap are written).  emu_gemv_geometry_query: out = {form, rows per workgroup,
 * the block kernels' rows-per-workgroup heuristic, the column partition} of a one-row bf16 stream, the rule the launch applies
 * (form 0 rolling, 1 head, 2 preload, 3 single round trip, 4 wave).  emu_l2_warm_test_plan (tests): the plan emu_linear_bf16 (one row)
 * and emu_decode_fused_bf16 (one row, combine launch) attach to their launches until it is cleared with NULL. */
typedef struct {
    const char* base;
    long long twin;
    unsigned long long limit, group_bytes;
    unsigned int block_bytes, row_bytes, head_bytes, nsucc, gx, first, ntouch, lanes, xcds;
} emu_warm_plan;
int emu_l2_warm_plan_make(const void* base, long twin, unsigned rows, unsigned row_bytes, unsigned used_bytes, unsigned long long nrows,
                          unsigned gx, unsigned groups, unsigned pred_wgs, int extra, unsigned lanes, unsigned long long budget_bytes,
                          int shape, emu_warm_plan* out);
long emu_l2_warm_enumerate(const emu_warm_plan* plan, unsigned wg, long long* offsets, long cap);
int emu_gemv_geometry_query(int N, int K, int norm, int epi, int out[4]);
void emu_l2_warm_test_plan(const emu_warm_plan* plan);
/* embed_tokens (emu.py:119,193) and the masked row overwrite text_embeds[ids == IMAGE] = ... (emu.py:202-203) */
int emu_embed_gather_bf16(const int32_t* ids, const void* table, void* out, int n_tok, int hidden, int vocab,
                          emu_stream_t s);
int emu_scatter_rows_bf16(const void* src, const int32_t* dst_rows, void* out, int n_rows, int hidden,
                          emu_stream_t s);
/* greedy next-token selection of lm.generate(num_beams=1, do_sample=False) (emu.py:213-229); suppress_id =
 * EOS while fewer than min_length tokens exist, else -1.  First index wins ties. */
int emu_argmax_bf16(const void* logits, int ld, int rows, int vocab, int suppress_id, int32_t* out,
                    emu_stream_t s);
/* Next-token selection with the logits pipeline of lm.generate(num_beams=1, do_sample=..., temperature, top_k, top_p,
 * repetition_penalty, min_length) (emu.py:213-229; the chat demo's chat.py:86-148 runs it with temperature 0.7, top_p 0.9) in ONE
 * launch, one workgroup per row; the specification is emu_amd/sampling.py.  In transformers' order: s = float(logit); repetition
 * penalty once per distinct id of the row's history (s < 0 ? s * pen : s / pen, ids outside [0, vocab) ignored); s[suppress_id] = -inf
 * while step < min_len; then do_sample = 0: first index of the maximum; do_sample = 1: s / temperature, top-k with k' = min(max(top_k,
 * min_keep), vocab) (ties with the k'-th value stay; top_k <= 0 = off), top-p (token i stays iff the softmax mass of {j: s_j <= s_i}
 * exceeds 1 - top_p, or s_i >= the min_keep-th largest value; ties at the threshold stay as a group; top_p >= 1 = off), and the draw:
 * the lowest id whose inclusive cumulative probability over the kept tokens in ascending id order exceeds u (rounding left u at or
 * beyond the total: the highest kept id). */
typedef struct emu_sample_params {
    float repetition_penalty;      /* 1 = off */
    int suppress_id, min_len;      /* suppress_id < 0 = off */
    int do_sample;
    float temperature;             /* > 0 */
    int top_k;
    float top_p;                   /* (0, 1]; >= 1 = off */
    int min_keep;                  /* >= 1 */
    int eos_id, pad_id;
} emu_sample_params;
#define EMU_SAMPLE_MAX_VOCAB 40000 /* the row is held as 4 bytes per token in the CU's 160 KiB of LDS */
/* logits: bf16 rows `ld` elements apart, any 2-byte-aligned base.  step_dev: device int32[1], read by the kernel (never a host
 * scalar, so one captured graph serves every step): the row's history is hist[t * hist_ld + row] for t < min(step, hist_rows) (hist
 * may be NULL), its uniform is uniforms[min(step, uni_rows - 1) * uni_ld + row] (fp32 in [0, 1); needed when do_sample), and the
 * min-length suppress applies while step < min_len.  unfinished (device int32 [rows], may be NULL): a row whose flag is 0 emits
 * pad_id and nothing else of it is written; a row that selects eos_id clears its flag.  out: int32 [rows].  probs_out (may be NULL;
 * do_sample only): fp32 rows ld_probs apart receive the probabilities the draw was made from, exactly 0 for removed tokens.
 * No allocation, no synchronisation: capturable.  The same inputs give the same outputs bit for bit.
 * -22: vocab > EMU_SAMPLE_MAX_VOCAB (nothing is launched or written), or an argument out of range. */
int emu_sample_bf16(const void* logits, int ld, int rows, int vocab, const int32_t* hist, int hist_ld, int hist_rows,
                    const int32_t* step_dev, const float* uniforms, int uni_ld, int uni_rows, const emu_sample_params* params,
                    int32_t* unfinished, int32_t* out, float* probs_out, int ld_probs, emu_stream_t s);
/* Constrained decoding: a token trie over a closed set of answers, as flat tables on the device (emu_amd/constrain.py builds them).
 * The reference forwards **kwargs from generate to lm.generate (Emu2/emu/emu.py:175,228, Emu1/models/modeling_emu.py:116,178), and its
 * evaluation model uses that for trie-constrained generation: a Trie over the ids of "yes." / "no." + EOS handed over as
 * prefix_allowed_tokens_fn with 5 beams (Emu1/mm_eval/models/emu.py:96-109, Emu1/mm_eval/models/trie.py:16-79).  A Python callable
 * cannot run inside a captured step; the tables can be read by the selection kernels.
 * Node 0 is the root.  The edges of node n are tok[first[n] .. first[n + 1]) (ids ascending) and lead to child[...]; child -1 =
 * "exhausted or off the trie" (an EOS edge leads there).  A row's state is one int32 node: at node n the ids tok[...] are allowed; at
 * a node outside [0, nodes) (or one without edges) only eos_id is.  Masked ids are -inf.  After a selection the row moves to
 * child(node, chosen id), -1 if that id is no edge.  The kernels clamp what they read from `first` to [0, edges] and take a node
 * outside [-1, nodes) as exhausted, so no table value leads to a read out of bounds. */
typedef struct emu_token_trie {
    const int32_t *first, *tok, *child; /* device: int32 [nodes + 1], [edges], [edges] */
    int nodes, edges;
} emu_token_trie;
/* emu_sample_bf16 under a constraint: the mask is applied to the row after the min-length suppress (the place of the library's
 * PrefixConstrainedLogitsProcessor: after the processors, ahead of the warpers), so the arg-max, the thresholds and the softmax run
 * over the allowed ids; the exhausted node allows params->eos_id.  node: device int32 [rows], in/out: the row's node is advanced by
 * the selected id in the same launch; a finished row (unfinished[row] == 0) emits pad_id and keeps its node.  With every id an edge
 * of the row's node the outputs are emu_sample_bf16's bit for bit.
 * -22, nothing launched: emu_sample_bf16's bounds, trie or node NULL, a table NULL, nodes < 1, edges < 0. */
int emu_sample_trie_bf16(const void* logits, int ld, int rows, int vocab, const int32_t* hist, int hist_ld, int hist_rows,
                         const int32_t* step_dev, const float* uniforms, int uni_ld, int uni_rows, const emu_sample_params* params,
                         int32_t* unfinished, int32_t* out, float* probs_out, int ld_probs, const emu_token_trie* trie, int32_t* node,
                         emu_stream_t s);
/* emu_sample_bf16 with the library's no-repeat n-gram ban (NoRepeatNGramLogitsProcessor; Emu1's generate takes no_repeat_ngram_size
 * and hands it to lm.generate, Emu1/models/modeling_emu.py:115,177); the specification is emu_amd/sampling.py::banned_ngram_mask.
 * With h[0 .. nh) the row's history (nh = min(step, hist_rows) ids of hist, as for the penalty) an id v gets -inf iff
 * nh + 1 >= ngram and the last ngram - 1 ids of the history occur earlier in it followed by v: some i in [0, nh - ngram + 1) has
 * h[i .. i + ngram - 1) == h[nh - ngram + 1 .. nh) and h[i + ngram - 1] == v (ngram = 1: every id of the history).  A would-be
 * banned id outside [0, vocab) is ignored.  The ban stands after the repetition penalty and ahead of the min-length suppress, the
 * library's processor order.  ngram = 0 (or hist NULL): emu_sample_bf16's outputs bit for bit.  The caller keeps vocab large enough
 * that the ban and the suppress together leave a finite score (at most nh + 1 ids go): a row without one has no defined draw.
 * -22, nothing launched: ngram < 0, emu_sample_bf16's bounds. */
int emu_sample_ngram_bf16(const void* logits, int ld, int rows, int vocab, const int32_t* hist, int hist_ld, int hist_rows,
                          const int32_t* step_dev, const float* uniforms, int uni_ld, int uni_rows, const emu_sample_params* params,
                          int32_t* unfinished, int32_t* out, float* probs_out, int ld_probs, int ngram, emu_stream_t s);
/* The log-probability of a FORCED token under each row of logits (the specification is emu_amd/scoring.py): what the reference's LM
 * loss is made of (Emu1/models/modeling_llama.py:110-116: CrossEntropyLoss over shifted logits / labels) and what its `predict` ranks
 * candidate answers by (Emu1/models/prediction_mixin.py:36-131).  Per row, in fp32: m = max x, lse = m + log(sum exp(x - m)),
 * lp = x[t] - lse for the row's target t (a target outside [0, vocab) -- the reference's ignore value is -100 -- gives lp = 0;
 * x[t] = -inf gives -inf), top1 = the first index of the maximum (emu_argmax_bf16's tie rule), and with a reference row r:
 * kl = sum_j p_r[j] * (logp_r[j] - logp_x[j]) (terms with p_r[j] == 0 left out; +inf where x rules out what r allows) and
 * agree = (top1(x) == top1(r)).
 * logits / ref_logits: bf16 rows ld / ref_ld elements apart, any 2-byte-aligned base, any vocabulary (the row is streamed, not held
 * in LDS).  With step = step_dev ? *step_dev : 0 (device int32[1], never a host scalar: one captured graph serves every step) the
 * target of row r is targets[step * tgt_ld + r] and every output is written at out[step * out_ld + r].  Every output pointer may be
 * NULL; without ref_logits, kl and agree are not written.  One workgroup per row; every sum is a fixed-order blocked sum (no
 * floating-point atomics): the same inputs give the same bits.  No allocation, no synchronisation: capturable.
 * -22 (nothing is launched or written): logits or targets NULL, ld < vocab, ref_logits with ref_ld < vocab, rows < 1, vocab < 1,
 * tgt_ld < rows or out_ld < rows. */
int emu_token_logprob_bf16(const void* logits, int ld, int rows, int vocab, const int32_t* targets, int tgt_ld,
                           const int32_t* step_dev, const void* ref_logits, int ref_ld, float* lp, float* lse, int32_t* top1,
                           float* kl, int32_t* agree, int out_ld, emu_stream_t s);
/* PatchEmbed conv as im2col (eva_vit.py:327-335): image NCHW (fp32 or bf16) -> [B*g*g, Kpad] bf16 */
int emu_patchify(const void* image, int image_is_f32, void* out, int B, int C, int HW, int patch, int Kpad,
                 emu_stream_t s);
/* Image front end: torchvision Resize((S, S), BICUBIC) -> ToTensor -> Normalize of one uint8 RGB image (Emu2/emu/chat.py:35-39,
 * Emu2/emu/diffusion.py:58-63), bit-exact with Pillow's 8-bit resample.  src [H, W, 3] interleaved on the device, rows `pitch` bytes
 * apart.  hcoef / vcoef int32 [S, hk] / [S, vk] (22 fractional bits) and hbounds / vbounds int32 [S, 2] (first tap, tap count) are
 * Pillow's precompute_coeffs + normalize_coeffs_8bpc tables (emu_amd/preprocess.py::resample_coeffs); the vertical pass reads source
 * rows [row0, row0 + nrows) = [vbounds[0][0], vbounds[S-1][0] + vbounds[S-1][1]) and the horizontal pass is made over those rows only.
 * A pass whose input size equals S is skipped and its tables may be NULL.  lut fp32 [3, 256] = (v / 255 - mean[c]) / std[c];
 * out = image [3, S, S] of an [N, 3, S, S] batch, bf16 (round to nearest even of the table value) or fp32.  ws: at least
 * emu_image_resample_ws_bytes.  No allocation, no synchronisation: capturable.  -22: H or W above EMU_IMAGE_MAX_SIDE, S above
 * EMU_IMAGE_MAX_OUT, more than EMU_IMAGE_MAX_TAPS taps, pitch < 3 * W, rows outside the image, a workspace too small. */
#define EMU_IMAGE_MAX_SIDE 16384
#define EMU_IMAGE_MAX_OUT 4096
#define EMU_IMAGE_MAX_TAPS 1024
size_t emu_image_resample_ws_bytes(int H, int W, int S);
int emu_image_resample_norm(const uint8_t* src, long pitch, int H, int W, const int32_t* hcoef, const int32_t* hbounds, int hk,
                            const int32_t* vcoef, const int32_t* vbounds, int vk, int row0, int nrows, const float* lut, void* out,
                            int out_is_f32, int S, void* ws, size_t ws_bytes, emu_stream_t s);
/* Image back end: numpy_to_pil's (images * 255).round().astype("uint8") (Emu2/emu/diffusion.py:214-234) on the decoded image while
 * it is still on the device: x bf16 [N, C, H, W] with values in [0, 1] -> out uint8 [N, H, W, C] = rint(float(x) * 255.0f), round
 * half to even (values outside [0, 1] saturate).  C <= 4.  -22: sizes out of range. */
int emu_image_to_u8_nhwc(const void* x, uint8_t* out, int N, int C, int H, int W, emu_stream_t s);
/* cat(cls, patches) + pos_embed (eva_vit.py:406-409) */
int emu_vit_assemble_bf16(const void* patches, const void* cls, const void* pos, void* x, int B, int T, int C,
                          emu_stream_t s);
/* encode_image pooling (emu.py:82-89): tokens [B, 1+g*g, C] -> [B, (g/s)^2, C] */
int emu_avgpool_tokens_bf16(const void* x, void* out, int B, int g, int C, int stride, emu_stream_t s);
/* apply_rotary_pos_emb on q,k in place + KV-cache append (transformers LlamaAttention; emu.py:213-229).
 * qkv rows [B*T, 3*H*D] (q | k | v); cos/sin tables [max_pos, D] bf16; caches [B, H, S_max, D]. */
int emu_rope_kv_append_bf16(void* qkv, const void* cos, const void* sin, const int32_t* pos,
                            const int32_t* slot, void* kcache, void* vcache, int B, int T, int H, int D,
                            int S_max, emu_stream_t s);
/* Vt[b,h,d,s] = V[b,h,s,d], zero padded to S_pad (multiple of 64) */
int emu_transpose_v_bf16(const void* v, long v_sb, long v_sh, long v_ss, void* vt, int B, int H, int S, int D,
                         int S_pad, emu_stream_t s);
/* softmax(Q K^T * scale + causal/left-pad mask) V, fused (LlamaAttention prefill; eva_vit.py:227-248;
 * diffusers attention).  D in {64, 128}.  kstart[b]: keys < kstart[b] masked (left padding), may be NULL. */
int emu_flash_attn_bf16(const void* q, long q_sb, long q_sh, long q_ss, const void* k, long k_sb, long k_sh,
                        long k_ss, const void* vt, void* o, long o_sb, long o_sh, long o_ss,
                        const int32_t* kstart, int B, int H, int Sq, int Sk, int Sk_pad, int D, int causal,
                        float scale, emu_stream_t s);
/* Two-segment ("cascade") flash attention, D = 128: B rows of Sq queries behind ONE shared prefix -- candidate ranking, where the
 * reference runs prompt + candidate through the model once per candidate (Emu1/models/prediction_mixin.py:36-131).  Query i of row b
 * attends the prefix keys [kstart, P) (kprefix [H, P, D] by kp_sh / kp_ss, vtprefix [H, D, P_pad], common to all rows) and its own
 * keys j <= i + (Sk - Sq) (k [B, H, Sk, D] strided, vt [B, H, D, Sk_pad]): one online softmax over both segments with
 * emu_flash_attn_bf16's tile arithmetic, prefix tiles first -- for P a multiple of 64 bit-identical to emu_flash_attn_bf16 on the
 * concatenated keys.  Both V^T pads are zero (emu_transpose_v_bf16).  -22, nothing written: D != 128, P < 1, kstart outside [0, P),
 * Sk < Sq, pads that are not multiples of 64 covering P / Sk. */
int emu_flash_attn_prefix_bf16(const void* q, long q_sb, long q_sh, long q_ss, const void* kprefix, long kp_sh, long kp_ss,
                               const void* vtprefix, const void* k, long k_sb, long k_sh, long k_ss, const void* vt, void* o,
                               long o_sb, long o_sh, long o_ss, int kstart, int B, int H, int Sq, int P, int P_pad, int Sk,
                               int Sk_pad, int D, float scale, emu_stream_t s);
/* one-query attention over the KV cache (decode step).  ctx_dev (device int32, may be NULL) overrides ctx so a
 * captured graph can be replayed while the context grows; ctx_max sizes the launch. */
size_t emu_decode_attn_ws_bytes(int B, int H, int D, int ctx_max);
int emu_decode_attn_bf16(const void* q, long q_sb, long q_sh, const void* kcache, const void* vcache, void* o,
                         long o_sb, long o_sh, const int32_t* kstart, const int32_t* ctx_dev, int ctx,
                         int ctx_max, void* ws, int B, int H, int D, int S_max, float scale, emu_stream_t s);
/* The decode step's attention launch (transformers LlamaAttention with a KV cache, one new token per row; emu.py:213-229): RoPE of
 * q and of the new key at pos[b], append of the new key / value at cache slot[b], attention of the rotated q over the keys
 * kstart[b] <= key <= slot[b] in splits of 128 keys, and the merge of the splits.  qkv [B, 3*H*D] (q | k | v, not rotated, left as
 * it is); caches [B, H, S_max, D]; o[b*o_sb + h*o_sh + d]; kstart may be NULL; ws: emu_decode_fused_ws_bytes; ctx_max sizes the
 * launch (max slot + 1 <= ctx_max <= S_max).  share_nb in 2..8: the rows are groups of share_nb beams whose first share_len
 * slots are stored in the group's first row only (B % share_nb == 0, 0 <= share_len < ctx_max, share_len <= every slot).
 * arrive (share_nb <= 1 only; may be NULL): B*H zeroed int32 counters -- the last split of a head to arrive merges the head, the
 * counters are zero again afterwards.  D in {64, 128}.  -22: refused, nothing was launched. */
size_t emu_decode_fused_ws_bytes(int B, int H, int D, int ctx_max);
int emu_decode_fused_bf16(const void* qkv, const void* cos, const void* sin, const int32_t* pos, const int32_t* slot,
                          void* kcache, void* vcache, void* o, long o_sb, long o_sh, const int32_t* kstart, void* ws, int B,
                          int H, int D, int S_max, int ctx_max, float scale, int share_nb, int share_len, int32_t* arrive,
                          emu_stream_t s);
/* The same for a CHUNK of T rows per sequence (2 <= T <= 8; the verify step of prompt-lookup speculative decoding): qkv [B*T, 3*H*D];
 * row i of sequence b has cache slot slot0[b] + i and RoPE position pos0[b] + i (slot0, pos0: device int32 [B], so a captured launch
 * replays while the context grows) and attends over kstart[b] <= key <= slot0[b] + i.  One launch rotates the T queries and new keys,
 * appends the T K / V rows and forms every row's split states (a split's cache rows are loaded once for all T rows; the chunk's own
 * slots are taken from the freshly rotated rows, never read back); the one-row merge launch follows.  o[(b*T + i)*o_sb + h*o_sh + d].
 * Row i's output bits and the cache rows equal those of T successive emu_decode_fused_bf16 launches with slot = slot0 + i.  The caller
 * guarantees slot0[b] + T <= ctx_max <= S_max.  -22: refused (T outside 2..8, D not 64 / 128, ctx_max outside [1, S_max]), nothing
 * was launched. */
size_t emu_decode_chunk_ws_bytes(int B, int T, int H, int D, int ctx_max);
int emu_decode_chunk_bf16(const void* qkv, const void* cos, const void* sin, const int32_t* pos0, const int32_t* slot0, void* kcache,
                          void* vcache, void* o, long o_sb, long o_sh, const int32_t* kstart, void* ws, int B, int T, int H, int D,
                          int S_max, int ctx_max, float scale, emu_stream_t s);
/* The selection behind a chunk step of T = 1 + k rows, one sequence (csrc/lookup.hip; specified in emu_amd/speculate.py): the rows'
 * arg-maxes (EOS suppressed in row i while step + i < min_len), then ONE workgroup accepts the draft's leading matches, appends the
 * emitted ids to out_ids [max_new] and to hist (the prompt's real ids, then the generated ones; hist_cap ints), finds the next draft
 * (or takes row `step` of drafts [max_new, k] when that is not NULL: tests and timing) and advances cur [T] (last emitted id, then the
 * draft, 0 beyond it), pos0 / slot0 / ctx_dev [1] and st.  st: int32 [8] = {step, finished, n_draft, hist_len, steps_run,
 * tokens_emitted, -, -}.  amax: int32 [T] scratch.  A call at step >= max_new or after finished changes nothing. */
int emu_lookup_select_bf16(const void* logits, int ld, int V, int T, int32_t* amax, int32_t* cur, int32_t* st, int32_t* pos0,
                           int32_t* slot0, int32_t* ctx_dev, int32_t* out_ids, int32_t* hist, int hist_cap, const int32_t* drafts,
                           int max_ngram, int max_new, int min_len, int eos_id, int stop_on_eos, emu_stream_t s);
/* emu_lookup_select_bf16 with emu_sample_bf16's selection in the place of the arg-maxes (prompt lookup together with do_sample or a
 * repetition penalty: transformers' _assisted_decoding runs the processors and warpers on every row with the history extended by the
 * draft ids before it, draws one token per row and keeps the draft while each drawn token equals the next draft id; specified in
 * emu_amd/speculate.py: row_select).  One 1024-thread workgroup per chunk row i <= n_draft picks amax[i] exactly as emu_sample_bf16
 * picks output index step + i: history = out_ids[0 .. step) followed by cur[1 .. 1 + i) (the penalty acts once per distinct id, from
 * the original logit; ids outside [0, V) are ignored), params->suppress_id suppressed while step + i < params->min_len, the uniform
 * uniforms[min(step + i, uni_rows - 1)] (fp32 [uni_rows], one per output index; may be NULL without do_sample).  No unfinished flags,
 * no constraint, no n-gram ban.  With the same uniforms the loop therefore emits the ids the one-row loop of emu_llama_sample_step
 * emits, wherever both see the same logits.  Then emu_lookup_select_bf16's one workgroup, unchanged.  A call at step >= max_new or
 * after finished changes nothing; rows behind the draft are not written (amax there is never read).  No floating-point atomics:
 * results repeat bit for bit.  -22, nothing launched: V > EMU_SAMPLE_MAX_VOCAB, do_sample without uniforms, options emu_sample_bf16
 * refuses, emu_lookup_select_bf16's own refusals. */
int emu_lookup_sample_bf16(const void* logits, int ld, int V, int T, int32_t* amax, int32_t* cur, int32_t* st, int32_t* pos0,
                           int32_t* slot0, int32_t* ctx_dev, int32_t* out_ids, int32_t* hist, int hist_cap, const int32_t* drafts,
                           int max_ngram, int max_new, int min_len, int eos_id, int stop_on_eos, const emu_sample_params* params,
                           const float* uniforms, int uni_rows, emu_stream_t s);

/* ---- LLaMA decoder engine ------------------------------------------------------------------------------
 * transformers LlamaModel / LlamaForCausalLM as used by EmuModel.generate / generate_image
 * (emu.py:133-138, 213-229).  Weights are passed as raw pointers to PACKED tensors (see emu_amd/llama.py):
 *   wqkv  [3*Hl*D, hidden]   rows = q heads | k heads | v heads of this TP shard
 *   wo    [hidden, Hl*D]
 *   wgu   [2*Fl, hidden]     gate/up interleaved: row 2j = gate_j, row 2j+1 = up_j
 *   wdown [hidden, Fl]
 * KV cache: [layers, B, Hl, S_max, D] for K and V. */
typedef struct {
    int hidden, heads_local, head_dim, ffn_local, layers, vocab, max_pos;
    float rms_eps;
} emu_llama_cfg;
int emu_llama_create(emu_ctx* ctx, const emu_llama_cfg* cfg, emu_llama** out);
void emu_llama_destroy(emu_llama* m);
int emu_llama_set_layer(emu_llama* m, int layer, const void* wqkv, const void* wo, const void* wgu,
                        const void* wdown, const void* ln1, const void* ln2);
/* Optional fp8 decode stream (not in the reference, which runs bf16 end to end -- Emu2/emu/chat.py:199-213; this is
 * the weight-only quantised serving mode of BASELINE.json configs[5]).  W8: OCP e4m3fn bytes in the SAME packed row
 * layout as the bf16 weight; scale: fp32 [rows], W ~= fp8 * scale[row].  emu_llama_use_fp8(m, 1): decode rows (B*T <= 2)
 * stream them, prefill keeps the bf16 weights; (m, 2): prefill rows (B*T > 16) run W8A8 GEMMs as well -- activations
 * quantised per row ahead of every GEMM, emu_linear_fp8_bf16 -- when hidden, heads_local*head_dim and ffn_local are
 * multiples of 128 (BASELINE.json configs[4], "fp8 MFMA weights"); (m, 0): bf16.  Fails if the fp8 tensors were not registered.
 * emu_llama_use_fp8(m, 3) is mode 1 and (m, 4) is mode 2 plus: every forward / logits call of 3 <= B*T <= 16 rows (a 5-beam step, a
 * batch of prompts, contrastive search) streams the fp8 set through emu_linear_fp8w_thin_bf16's kernel -- qkv, o_proj, gate/up, down
 * and the head where it has an fp8 copy (whole or emu_llama_set_head_shard rows); the RMSNorm launches of the bf16 few-row path stay,
 * attention is untouched.  Modes 3 and 4 fail (-22, with a message) unless hidden, heads_local*head_dim and ffn_local are multiples
 * of 256 (every TP = 1 / 2 sharding of the 33B shapes; the TP = 4 / 8 shards are refused).  Modes 0..2 are what they were.
 * emu_llama_use_fp8(m, 5) is mode 3 and (m, 6) is mode 4 plus: every forward / logits call of 17 <= B*T <= 64 rows (beams x batch,
 * contrastive search on a batch) streams the fp8 set through emu_linear_fp8w_gemm_bf16's kernel, the same projections and head; the
 * RMSNorm launches stay in front of the projections and a prompt of 17..64 rows runs the unfused RoPE / KV append and V^T launches
 * (no RoPE epilogue, no K-slice sum + RMSNorm fusion at those row counts).  Above 64 rows mode 5 is mode 3 (bf16) and mode 6 is
 * mode 4 (W8A8 GEMMs).  Same width and every-layer requirements as modes 3 and 4.  Modes 0..4 are what they were.
 * emu_llama_use_fp8_all(m, 1), a switch beside modes 5 / 6: every call of 65 rows and more (a prompt, a scoring prefill, beams x
 * batch) stays on the fp8 set too -- under mode 5 qkv, o_proj, gate/up, down and the head run emu_linear_fp8w_tile_bf16's kernel
 * (RMSNorm, RoPE / KV append and V^T stay launches; no RoPE epilogue, no K-slice sum + RMSNorm fusion, no two-lane prefill); under
 * mode 6 the layer projections keep the W8A8 GEMMs and the head, which has none, runs that kernel.  It needs mode 5 or 6 (so their
 * width and every-layer requirements: TP = 1 / 2 shards of the 33B shapes, TP = 4 / 8 refused) and the head's fp8 copy, and is
 * refused while fp4 is on (-22, with a message).  emu_llama_use_fp8 with a mode below 5 clears it.  With it on emu_llama_release_bf16
 * is valid (see there): afterwards only emu_llama_use_fp8(m, 5 | 6) is accepted, the switch cannot be cleared, and
 * emu_llama_use_fp8(m, < 5), emu_llama_use_fp4(m, any), emu_llama_set_decode_fused(m, != 0, ..) and the bf16 pack setters answer
 * -22 with a message that names the release.  Out of scope: TP = 4 / 8 widths (a partial last K stage), a fused RoPE / RMSNorm
 * epilogue in the new form, loading a checkpoint straight to fp8.  Accuracy on a trained checkpoint is unmeasured. */
int emu_llama_set_layer_fp8(emu_llama* m, int layer, const void* wqkv8, const float* sqkv, const void* wo8,
                            const float* so, const void* wgu8, const float* sgu, const void* wdown8,
                            const float* sdown);
int emu_llama_set_head_fp8(emu_llama* m, const void* lm_head8, const float* lm_scale);
int emu_llama_use_fp8(emu_llama* m, int enable);
int emu_llama_use_fp8_all(emu_llama* m, int on);
/* Optional MXFP4 decode stream (not in the reference; 0.53125 byte per weight, 0.53 of the fp8 stream's bytes).  W4 / scales: the
 * two tensors of emu_quantize_mxfp4_rows over the SAME packed (and, under tensor parallelism, sharded) bf16 matrix -- or prepared
 * offline by any quantiser that writes the format (emu_amd/mxfp4.py), the scale rows of every matrix at the stride that
 * emu_linear_fp4w_mfma_bf16 asks of its K (K / 32 where K % 256 == 0, else 8 * ceil(K / 256)).  emu_llama_set_head_fp4 covers the rows the bf16 lm_head
 * pointer holds (emu_llama_set_head_shard is honoured).  emu_llama_use_fp4(m, 1): steps of B*T <= 2 rows stream the 4-bit set
 * through the per-layer launches; prefill and steps of more rows keep the bf16 weights, so both sets stay resident.  It fails
 * (-22) unless every layer and the head are registered, if hidden, heads_local*head_dim or ffn_local is not a multiple of 32, and
 * while the fp8 stream is on; emu_llama_use_fp8 fails while the fp4 stream is on (the two streams are exclusive).  The fused-layer
 * modes, the persistent engine and the merged o_proj do not run in this mode.  Accuracy on a trained checkpoint is unmeasured.
 * emu_llama_use_fp4(m, 2) is mode 1 plus: every forward / logits call of 3 <= B*T <= 16 rows (a 5-beam step, a batch of prompts,
 * contrastive search) streams the 4-bit set through emu_linear_fp4w_thin_bf16's kernel -- qkv, o_proj, gate/up, down and the head
 * (whole or emu_llama_set_head_shard rows); the RMSNorm launches of the bf16 few-row path stay, attention is untouched.  It also
 * fails (-22) if hidden, heads_local*head_dim or ffn_local is below 256 (a multiple of 32 at least 256 will do: the TP = 4 / 8
 * shards of the 33B shapes, K = 896 / 2240 / 4480, run with a partial last K stage).
 * Steps of 17 rows and more, and prefill, keep the bf16 weights in modes 1 and 2.
 * emu_llama_use_fp4(m, 3) is mode 2 plus: every forward / logits call of B*T >= 17 rows (prefill, beams x batch) runs qkv, o_proj,
 * gate/up, down and the head (whole or sharded) through emu_linear_fp4w_gemm_bf16's kernel, so no row count reads a bf16 matrix.
 * The RMSNorm launches stay in front of the projections; RoPE / KV append, V^T and flash attention are the unfused launches (no
 * RoPE epilogue, no K-slice sum + RMSNorm fusion, no two-lane prefill while the mode is on).  Same width requirement as mode 2.
 * emu_llama_release_bf16(m): valid only in mode 3, or in fp8 mode 5 / 6 with emu_llama_use_fp8_all on (else -22).  Forgets every layer's four bf16 matrix pointers and the bf16 lm_head
 * pointer, so the caller may free them (33B: 65 GB leave, 17 GB of 4-bit tensors stay); the norm gains, the embedding and the RoPE
 * tables stay.  From then on emu_llama_use_fp4(m, 0 | 1 | 2), emu_llama_use_fp8(m, != 0) and emu_llama_set_decode_fused(m, != 0, ..)
 * answer -22 with a message that names the release; there is no way back. */
int emu_llama_set_layer_fp4(emu_llama* m, int layer, const void* wqkv4, const void* sqkv, const void* wo4, const void* so,
                            const void* wgu4, const void* sgu, const void* wdown4, const void* sdown);
int emu_llama_set_head_fp4(emu_llama* m, const void* lm_head4, const void* lm_scales);
int emu_llama_use_fp4(emu_llama* m, int enable);
int emu_llama_release_bf16(emu_llama* m);
/* The one rule by which emu_llama_forward and emu_llama_logits pick the kernel of a projection -- host arithmetic on integers, no HIP
 * call, no model -- and its CPU test hook (tests/test_projection_rule.py).  The engine asks it with exactly these facts.
 * The kernels: 0 bf16 (the weight stream up to 8 / 16 rows, GEMMs above); 1 the fp8 stream (1..2 rows); 2 W8A8 GEMMs (17 rows and
 * more); 3 the MXFP4 stream (1..2 rows); 4 the MXFP4 matrix-core stream (3..16 rows); 5 the MXFP4 GEMM (17 rows and more); 6 the
 * 13-bit packed bf16 stream (1 row); 7 the fp8 matrix-core stream (3..16 rows); 8 the packed matrix-core stream (4..16 rows); 9 the
 * fp8 W8A16 GEMM (17..64 rows); 10 its form for 65 rows and more (64 weight rows x 128 activation rows; emu_linear_fp8w_tile_bf16).
 * Under the weight-stream profiler a launch over [N, K] is priced at 2NK bytes (0 where it streams), NK (1, 7, 9, 10), N(K/2 + K/32)
 * (3, 4, 5), the bytes its packed set stores (6, 8), nothing (2 and the bf16 GEMMs).  10, like 5, has no bf16 GEMM behind it: norms,
 * RoPE / KV append and V^T stay launches under it and it never runs the two-lane prefill.
 * emu_weight_mode: what the setters took -- fp8 0..6 (emu_llama_use_fp8), fp4 0..3 (emu_llama_use_fp4), never both non-zero; pack,
 * pack_wide (emu_llama_use_bf16_pack, _wide); bf16_released (emu_llama_release_bf16); fp8_all 0 / 1 (emu_llama_use_fp8_all: a switch
 * beside fp8 modes 5 / 6, as pack_wide is beside pack; with it off every answer is what it was).
 * The call-level rule (emu_llama_weight_kernel is this alone): mode, rows = B*T of the call and the shard's hidden, heads_local *
 * head_dim and ffn_local give the kernel the call is planned around.  1..2 rows: 3 if fp4, 1 if fp8, else 0.  3..16 rows: 4 in fp4
 * modes 2, 3; 7 in fp8 modes 3..6 when the three widths are multiples of 256; else 0.  17 rows and more: 5 in fp4 mode 3; 9 in fp8
 * modes 5, 6 up to 64 rows, same widths; 10 in fp8 mode 5 under fp8_all at 65 rows and more, same widths; 2 in fp8 modes 2, 4, 6
 * when the widths are multiples of 128 (mode 6 keeps the faster W8A8 prefill for the layer projections under fp8_all); else 0.
 * The matrix-level rule: that answer and the facts of ONE matrix at one call site give the kernel that launches, and norm_in_stream
 * (out) = the RMSNorm rides in the weight stream.  [N, K], epi: the projection.  has_fp8: the matrix has an fp8 copy.  pack_rows,
 * set_n, set_k: the rows per group (0: none) and shape of its registered packed set.  fused_mode, tail_mode, warm_mask: what inhibits
 * the packed one-row stream -- emu_llama_set_decode_fused as set; a layer projection passes the decode tail its call runs and the
 * L2-warm boundaries its call and this launch carry, the head emu_llama_set_decode_tail / _l2_warm as set.  tune: the emu_gemm_tune
 * mask.  head = 0, a layer projection: norm = its call fuses the norm in front (1..2 rows on kernels 1, 3; one row on 0; never in a
 * chunk step on 0), and norm_in_stream = norm; 2 runs as 0 when !has_fp8.  head = 1 (norm is not read, the head always has one in
 * front; ws_fits: the caller's workspace holds the normalised rows): 2 runs as 10 under fp8_all when has_fp8, rows >= 65 and
 * K % 256 == 0, else as 0, and so do 1, 7, 9, 10 when !has_fp8, 7 when !ws_fits && !(bf16_released && fp8_all),
 * 4 when !ws_fits && !bf16_released; norm_in_stream = kernels 1, 3, and 0 at one row or, when !ws_fits, up to 8 rows.  Then, either
 * site, 0 becomes 6 when pack is on, rows == 1, no inhibitor is set and the set is of this [N, K] with emu_bf16_pack_rows(N, K,
 * norm_in_stream, epi, tune) == pack_rows; and 0 becomes 8 when pack and pack_wide are on, 4 <= rows <= 16, !norm_in_stream, the set
 * is of this [N, K] and emu_gemv_pack_thin_plan has a plan for the shape.  Every other kernel passes through.
 * Returns the kernel, or -22: q null, a mode out of range or both non-zero, fp8_all outside 0 / 1 or set with fp8 below 5 (so with
 * any fp4 mode), rows / a width / N / K < 1, pack_rows or warm_mask < 0.  emu_llama_weight_kernel answers with fp8_all off. */
typedef struct emu_weight_mode { int fp8, fp4, pack, pack_wide, bf16_released, fp8_all; } emu_weight_mode;
typedef struct emu_projection {
    emu_weight_mode mode;
    int rows, hidden, heads_dim_local, ffn_local;               /* the call */
    int N, K, norm, epi, has_fp8, pack_rows, set_n, set_k;      /* the matrix */
    int fused_mode, tail_mode, warm_mask, tune, head, ws_fits;  /* the site */
    int norm_in_stream;                                         /* out */
} emu_projection;
int emu_llama_projection_kernel(emu_projection* q);
int emu_llama_weight_kernel(int fp8_mode, int fp4_mode, int rows, int hidden, int heads_dim_local, int ffn_local);
/* The 13-bit lossless packing of a bf16 weight matrix for the one-row decode streams; emu_amd/bf16pack.py is the definition of the
 * format and emu_amd/csrc/bf16_pack.h states the layout once for the packer and the kernels.  A weight keeps its low byte and its
 * sign and stores the top 7 bits of its exponent field as a 4-bit offset from a per-matrix base hb (a window of 32 binades below the
 * matrix's largest finite exponent); a row group with a weight outside the window is flagged and read from the bf16 matrix.
 * Lossless: the streams decode in registers and feed the bf16 kernels' arithmetic, the results are the same bits.
 * emu_bf16_pack_rows: the rows per group (2 or 4) of the set a one-row stream over [N, K] with / without the fused RMSNorm and epilogue
 * epi would read under the emu_gemm_tune mask `tune`, or 0 when the planner sends the shape to a form without a packed twin.
 * emu_bf16_pack: packs bf16 [N, ldw] (K % 32 == 0, rows 2 or 4) on the device: lo ceil(N/rows)*rows*K bytes, nib half, sign an
 * eighth of that, flags ceil(ceil(N/rows)/32) 32-bit words; *hb_out = hb.  The call waits for its own result.
 * emu_linear_bf16pack (tests): C[1, N] = epi(norm(A) W^T [+ res]) over such a set in the given form (1 head: rows 4, norm_w set, K <=
 * 8192, epi NONE / SWIGLU; 2 preload: rows 2, K <= 8192; 3 single round trip: rows 2, K <= 18432; both without norm, epi NONE /
 * RESID); W = the bf16 matrix [N, K], read for flagged row groups.  Bit-identical to emu_linear_bf16 on W. */
typedef struct emu_bf16_pack_set { const void *lo, *nib, *sign, *flags; int hb, rows; } emu_bf16_pack_set;
int emu_bf16_pack_rows(int N, int K, int norm, int epi, int tune);
int emu_bf16_pack(const void* w_bf16, int ldw, int N, int K, int rows, void* lo, void* nib, void* sign, void* flags, int* hb_out,
                  emu_stream_t s);
int emu_linear_bf16pack(const void* A, const void* W, const emu_bf16_pack_set* set, const void* res, const void* norm_w, void* C, int N,
                        int K, int form, float eps, int epi, emu_stream_t s);
/* The 12-bit format of the same streams (emu_amd/csrc/bf16_pack.h, emu_amd/bf16pack.py: pack12): the sign moves into the nibble
 * beside a 3-bit exponent code (a window of 8 codes from the base hb that covers the most weights), the sign plane goes, and the few
 * weights a row group has outside the window travel in its patch record (8 slots of 32 bits at patch + 32 g bytes); a row group with
 * more than 8 of them is flagged.  Lossless like the 13-bit format; a matrix holds a set of one format or the other.
 * emu_bf16_pack12: packs bf16 [N, ldw] (K % 32 == 0, K < 2^21, rows 2 or 4) on the device: lo and nib as emu_bf16_pack, patch
 * 32 * ceil(N/rows) bytes, flags as there; *hb_out = hb, *flagged_out = the number of flagged row groups.  Waits for its own results.
 * emu_linear_bf16pack12 (tests): emu_linear_bf16pack over a 12-bit set; bit-identical to emu_linear_bf16 on W.
 * emu_llama_set_layer_bf16_pack12 / emu_llama_set_head_bf16_pack12: the 12-bit counterparts of the two setters below (a matrix's set
 * of either format replaces the one it had).  The one-row streams read a 12-bit set; the 4..16-row twin reads one only under
 * emu_llama_use_bf16_pack_wide(m, 2) and otherwise leaves such a matrix on the bf16 kernel. */
typedef struct emu_bf16_pack12_set { const void *lo, *nib, *patch, *flags; int hb, rows; } emu_bf16_pack12_set;
int emu_bf16_pack12(const void* w_bf16, int ldw, int N, int K, int rows, void* lo, void* nib, void* patch, void* flags, int* hb_out,
                    int* flagged_out, emu_stream_t s);
int emu_linear_bf16pack12(const void* A, const void* W, const emu_bf16_pack12_set* set, const void* res, const void* norm_w, void* C,
                          int N, int K, int form, float eps, int epi, emu_stream_t s);
int emu_llama_set_layer_bf16_pack12(emu_llama* m, int layer, const emu_bf16_pack12_set* sets4);
int emu_llama_set_head_bf16_pack12(emu_llama* m, const emu_bf16_pack12_set* set, int rows_n);
/* The packed sets of a layer (sets4: qkv, o_proj, gate/up, down; rows == 0: that matrix has none and stays on bf16) and of the head
 * (rows_n: the rows the lm_head pointer holds); refused after emu_llama_release_bf16.  emu_llama_use_bf16_pack(m, 1): projections of
 * ONE activation row on the bf16 kernels stream their set where emu_llama_projection_kernel says so; everything else reads what it read. */
int emu_llama_set_layer_bf16_pack(emu_llama* m, int layer, const emu_bf16_pack_set* sets4);
int emu_llama_set_head_bf16_pack(emu_llama* m, const emu_bf16_pack_set* set, int rows_n);
int emu_llama_use_bf16_pack(emu_llama* m, int on);
/* CPU test hook (tests/test_bf16_pack_rule.py): the matrix-level rule of emu_llama_projection_kernel for `kernel` (0..7, else -22) at
 * a layer projection with an fp8 copy and a set of pack_rows rows per group for its own [N, K], the wide switch off: 6 or `kernel`. */
int emu_llama_pack_kernel(int kernel, int rows, int pack_rows, int pack_on, int fused_mode, int tail_mode, int warm_mask, int N, int K,
                          int norm, int epi, int tune);
/* The same sets under steps of 4..16 activation rows: the matrix-core twin of the bf16 few-row stream (gemv_pack_thin.hip), whose
 * outputs are that stream's bit for bit at 13/16 of its bytes.
 * emu_linear_bf16pack_thin (tests): C[M, N] = epi(A W^T [+ res]) for 4 <= M <= 16 rows of K contiguous elements over the set of the
 * bf16 matrix W [N, K] (read for flagged row groups); epi NONE / RESID (res [M, N]) / SWIGLU (C [M, N / 2]).  -22, nothing
 * written, where emu_gemv_pack_thin_plan refuses or a pointer is missing or a plane is off a 16-byte boundary.
 * emu_linear_bf16pack12_thin (tests): the same over a 12-bit set (the kernel's 12-bit twin: no sign piece in a stage, the row groups'
 * patch records applied to the decoded fragments); the same bits.  Also -22: a set without its patch pointer, records off a 16-byte
 * boundary, hb outside 0..120, K / 8 >= 2^18.
 * emu_llama_use_bf16_pack_wide(m, on): OFF (0) by default; with emu_llama_use_bf16_pack on, projections and the head at 4..16 rows that
 * are on the bf16 kernels stream their set where emu_llama_projection_kernel says so.  on = 1: matrices with a 13-bit set only -- one
 * that holds a 12-bit set is not offered to the rule at more than one row (pack_rows 0) and stays on the bf16 kernel there.  on = 2:
 * 12-bit sets are offered too, so one resident set serves a matrix's one-row and 4..16-row steps (13-bit sets go to the 13-bit twin
 * as under 1).  Any other non-zero value counts as 1.  Refused after emu_llama_release_bf16.
 * emu_llama_pack_thin_kernel (CPU test hook, tests/test_pack_thin_plan.py): the matrix-level rule of emu_llama_projection_kernel for
 * `kernel` (0..8, else -22) at a layer projection with an fp8 copy, a set of pack_rows rows per group for [set_n, set_k], the two
 * switches as given and the one-row stream inhibited: 8 or `kernel`. */
int emu_linear_bf16pack_thin(const void* A, const void* W, const emu_bf16_pack_set* set, const void* res, void* C, int M, int N, int K,
                             int epi, emu_stream_t s);
int emu_linear_bf16pack12_thin(const void* A, const void* W, const emu_bf16_pack12_set* set, const void* res, void* C, int M, int N, int K,
                               int epi, emu_stream_t s);
int emu_llama_use_bf16_pack_wide(emu_llama* m, int on);
int emu_llama_pack_thin_kernel(int kernel, int rows, int pack_rows, int set_n, int set_k, int pack_on, int wide_on, int N, int K, int norm,
                               int epi, int tune);
/* Vocabulary-sharded lm_head under tensor parallelism (the reference's lm_head is lm.lm_head of LlamaForCausalLM reached
 * from Emu2/emu/emu.py:213-229): the lm_head pointer of emu_llama_set_head holds rows [row0, row0 + rows) of the vocabulary only;
 * emu_llama_logits fills this rank's columns of the caller's [M, vocab] rows, zeroes the others and all-reduces the rows, so every
 * rank ends with the full, bit-identical logits.  rows < 0 = whole matrix (the default). */
int emu_llama_set_head_shard(emu_llama* m, int row0, int rows);
int emu_llama_set_head(emu_llama* m, const void* final_norm, const void* lm_head, const void* embed,
                       const void* rope_cos, const void* rope_sin);
/* kcache == vcache == NULL detaches the caches (the caller freed them): emu_llama_forward answers -22 until new ones are set. */
int emu_llama_set_kv(emu_llama* m, void* kcache, void* vcache, int batch, int s_max);
/* Beam search (the reference's default decoding mode: lm.generate(num_beams=5), Emu2/emu/emu.py:163-172,213-229; transformers
 * replicates the prompt's cache per beam with expand_inputs / _reorder_cache).  Here cache rows come in groups of `beams`
 * consecutive rows of one prompt whose first `shared_slots` slots (the prompt) are stored ONCE, in the group's first row:
 * single-token steps read them from there (the beams' workgroups for one 128-key split run on one XCD, whose L2 then
 * serves all but the first), and only slots >= shared_slots are per-row.  beams <= 1 switches it off
 * (emu_llama_set_kv does too).  -22 for beams > 8, a batch the group size does not divide, or slots beyond the capacity. */
int emu_llama_set_kv_share(emu_llama* m, int beams, int shared_slots);
/* Candidate ranking on a shared prompt (Emu1/models/prediction_mixin.py:36-131: one prompt, N candidate answers): the prompt's keys
 * and values stay where its prefill left them, kprefix / vprefix [layer, 1, Hl, prefix_s_max, D] (read only), of which slots
 * [kstart, prefix_len) are attended; the engine's current cache (emu_llama_set_kv) holds only the rows' OWN slots.  While set,
 * emu_llama_forward with T > 1 writes the rows' K / V at slot[] as always and runs emu_flash_attn_prefix_bf16's kernel over the prefix
 * plus own slots [0, ctx); a layer's prefix V is transposed once (one row), not once per batch row.  kstart[] must hold the same value
 * for every row (element 0 is used).  The fused RoPE / V^T prefill epilogues are off.  -22 with a message, before any launch: T == 1,
 * the chunk step, the token / lookup steps, emu_llama_set_kv_share, the fused decode modes, the two-lane tensor-parallel prefill;
 * head_dim != 128.  prefix_len = 0 or NULL pointers switch it off (emu_llama_set_kv does too).  emu_llama_workspace_bytes accounts
 * for the prefix V^T. */
int emu_llama_set_kv_prefix(emu_llama* m, const void* kprefix, const void* vprefix, int prefix_s_max, int prefix_len);
/* Parity hook: emu_llama_forward runs decoder layers [l0, l1) only (l1 < 0: through the last; default 0, -1 = all), each on the
 * KV-cache plane of its own index.  The full-size tests feed ONE layer the fp32 oracle's input of that layer (a common input per
 * layer instead of 60 layers of accumulated bf16 rounding); production code never calls it. */
int emu_llama_set_layer_range(emu_llama* m, int l0, int l1);

/* Prefill fusion (off by default), a PER-CALL promise: a caller that sets it promises that its NEXT emu_llama_forward call with
 * T > 1 rows passes slot[i] = i (the rows of the one batch element are the whole context, in order -- what EmuModel's prefill
 * does); that call consumes the promise, so any other caller of emu_llama_forward (rows in another slot order) gets the
 * unfused sequence, which honours slot[] everywhere, unless it renews the promise itself.  Then, for
 * B = 1, T == ctx, head_dim 128 and heads_local * 128 a multiple of 256, the qkv projection applies RoPE to q and k, appends
 * k / v to the cache and writes V^T for the attention kernel from its own epilogue (same arithmetic and rounding points as the
 * three launches it replaces: bit-identical hidden states and caches); every other call runs the unfused sequence. */
int emu_llama_set_prefill_fusion(emu_llama* m, int enable);

/* Tensor-parallel prefill with the all-reduces overlapped (the reference has no tensor parallelism: its multi-GPU scheme
 * is layer placement, Emu2/emu/mixin.py:44-81, Emu2/emu/chat.py:250-283).  min_rows > 0: a B = 1, T == ctx forward under the
 * slot-order promise (emu_llama_set_prefill_fusion) with at least min_rows rows (clamped up to 512) on a context with tp_size > 1
 * (or a 1-rank communicator / comm block) cuts the prompt's rows once, at a multiple of 256, into two halves that run as two
 * CONCURRENT LANES: causal attention makes the first half independent of the second, and the second needs only the first's keys /
 * values of the same layer, so each half walks all layers as its own chain (norm, qkv, attention, o_proj, all-reduce, norm, gate/up,
 * down, all-reduce) on its own stream -- the first on the caller's, the second on a stream owned by the context -- with one event
 * per layer (the first half's K / V rows are in the cache) the only edge between them.  While one lane's partial sums are on the
 * wire, the other lane's GEMMs have the CUs.  The caller's stream has joined the second one when the call returns (the whole
 * forward is capturable into one hipGraph).  All-reduces run inside their lane's stream where RCCL takes them; without a
 * communicator (rank processes sharing a device) every peer-to-peer all-reduce additionally waits for the one issued before it.
 * Same kernels and rounding points as the serial schedule; results agree to bf16 rounding, not bit for bit (a half-size launch may
 * take another tile configuration than the whole prompt's).  Cost on ONE GPU with a no-op all-reduce (what the cut itself costs):
 * +17 % (TP = 8 shard) ... +21 % (TP = 2) per prefill under graph replay; what it hides -- 2 x layers all-reduces of [S, hidden] --
 * needs a multi-GPU node to be measured.  min_rows = 0 keeps every all-reduce on the caller's stream between the GEMMs.  The first
 * call with min_rows > 0 creates the stream and events (never inside a forward); the workspace grows by the second lane's V^T and
 * K-slice scratch (emu_llama_workspace_bytes follows the setting). */
int emu_llama_set_tp_overlap(emu_llama* m, int min_rows);
/* forwards that took the two-half schedule since the engine was created (tests, tools) */
long emu_llama_tp_overlap_count(const emu_llama* m);

/* Decode attention in ONE launch (OFF by default): the last split workgroup of a head to arrive merges the head's splits itself
 * (agent-scope stores / loads of the split states and a relaxed arrival counter: no fence, no spinning) instead of a second,
 * combine launch; same arithmetic, bit-identical outputs.  Measured 0.4 % slower than the two launches on MI355X (three
 * dependent fabric round trips in the tail cost what the launch does), so it stays an option for A/B timing. */
int emu_llama_set_decode_tail(emu_llama* m, int enable);

/* L2 warming in the default one-row decode step (per-layer launches, bf16 weights, no tensor parallelism, own KV rows): the last
 * workgroups of a launch -- extra workgroups in the combine launch -- request the head of what the NEXT launch reads, each line from
 * a workgroup of the reader's XCD class, never waited for; results are bit-identical whatever the mask.  Bits 0-4, one boundary each:
 * 0 combine -> o_proj, 1 o_proj -> gate/up, 2 gate/up -> down, 3 down -> the next layer's qkv (lm_head behind the last layer),
 * 4 qkv -> this layer's K / V cache rows.  Bit 5: the first 4 KiB of every row of more workgroups instead of whole blocks of the
 * first ones; bits 8-15: the budget per boundary in MiB (0 = EMU_L2_WARM_DEFAULT_MIB).  Every other mode of the engine (beams, fp8,
 * fp4, tensor parallelism, fused layers, the persistent engine) runs without.  The default is what measured faster
 * (profiles/l2_warm.md); emu_gemm_tune bit 30 switches all of it off.  emu_llama_l2_warm_count: launches that carried a plan (tests). */
#define EMU_L2_WARM_DEFAULT 0
#define EMU_L2_WARM_DEFAULT_MIB 16
int emu_llama_set_l2_warm(emu_llama* m, int mask);
long emu_llama_l2_warm_count(const emu_llama* m);

/* Whole decoder layers of a one-row decode step in ONE launch (csrc/decode_layer.hip): with enable != 0, emu_llama_forward calls
 * with B == 1, T == 1, bf16 weights, head_dim 128 and no shared-prefix KV rows run layers_per_launch layers (0 = all layers of the
 * call) per launch instead of six launches (+ two all-reduces) per layer.  The workgroups of the launches it replaces become roles
 * of one grid that wait on arrival counters with their weight slice already requested; results are bit-identical to the launches
 * (same rows per workgroup and summation order).  Under tensor parallelism, enable == 1 cuts every layer at its two all-reduces
 * ([q, attention, o_proj] | emu_allreduce_bf16 | [gate/up, down] | emu_allreduce_bf16: four launches instead of eight), and
 * enable == 2 runs the all-reduces INSIDE the launch over the P2P comm blocks (emu_tp_p2p_enable must be on, else as 1): the
 * workgroup that completes o_proj / down_proj runs the peer exchange while the consumers' weight slices are already in flight.
 * enable == 3 (tensor parallelism with the P2P path on; otherwise as 1): the two RMSNorm-fronted weight streams stay stand-alone
 * launches, the attention (its split merge done by the head's last split) and the two row-sharded projections run as single-role
 * launches whose LAST workgroup to arrive runs the all-reduce in its tail -- 5 launches per layer instead of 8, and nothing waits
 * inside a launch except that one workgroup for its peers, so this mode is safe for rank processes sharing a device.
 * Mode 2 needs every rank on its own GPU (a launch that waits for a peer holds its CUs), and every fused mode needs the DEVICE TO
 * ITSELF (modes 1 and 2; also mode 1's cut layers wait inside their launches): processes that share a GPU can starve each other's producer workgroups of CU slots (observed with eight rank processes on
 * one device: a time-out, then garbage and a non-zero give-up count).  Every in-kernel wait is bounded in wall-clock time (2 s, or
 * the peer-to-peer time-out where longer).
 * enable == 4: the persistent weight-streaming engine (emu_amd/csrc/decode_engine.hip; see emu_gemv_chain_bf16): per layer the
 * attention launches, then ONE launch  o_proj -> all-reduce -> RMSNorm + gate/up (SwiGLU) -> down -> all-reduce -> RMSNorm + the next
 * layer's qkv projection, whose loader waves stream the layer's weights through an LDS ring ahead of the four hand-offs and whose
 * all-reduces run over the ranks' comm arrays (tags numbered by a per-CU device counter).  Tensor-parallel shards whose rows are at
 * most 13 KiB (hidden, heads_local * 128, ffn_local <= 6656: TP >= 4 at the LLaMA-33B shape) with the fence-free P2P path on; anything
 * else keeps the launches.  Same bits as the launches; needs every rank on its own GPU and the device to itself.
 * The first fused forward after a weight change uploads a pointer table and must therefore run outside stream capture (-16).
 * Replaces: the per-layer module calls of the LlamaDecoderLayer loop (Emu2/emu/emu.py:133-138, :213-229) and the device hops of
 * Emu2/emu/mixin.py:44-81. */
int emu_llama_set_decode_fused(emu_llama* m, int enable, int layers_per_launch);
/* giveups: in-kernel waits that ran into their time limit since creation (non-zero: outputs are garbage, treat as an error);
 * forwards: emu_llama_forward calls that took the fused path.  Either pointer may be NULL.  Synchronises the device. */
int emu_llama_decode_fused_stats(emu_llama* m, unsigned int* giveups, long* forwards);
/* Tools hook (tools/decode_trace.py): device buffer of 4 x u64 per workgroup of the LAST fused launch of a forward -- {role | layer << 8,
 * entry, input ready (0: no wait), exit} in 100 MHz ticks; written only by a library built with -DEMU_TRACE; NULL = off. */
int emu_llama_set_decode_trace(emu_llama* m, void* buf);
size_t emu_llama_workspace_bytes(const emu_llama* m, int B, int T);
/* all decoder layers over B*T rows (T > 1: prefill with MFMA GEMMs + flash attention; T == 1: decode with
 * weight-streaming GEMVs).  hidden [B*T, hidden] is the residual stream, updated in place (NOT final-normed).
 * pos/slot: device int32 [B*T] (RoPE position / cache slot per row); kstart: device int32 [B] or NULL;
 * ctx_dev: device int32 [1] = number of valid cache slots AFTER this call (decode only, may be NULL);
 * ctx: the same value on the host (exact for prefill; upper bound used when ctx_dev is given). */
int emu_llama_forward(emu_llama* m, void* hidden, int B, int T, const int32_t* pos, const int32_t* slot,
                      const int32_t* kstart, const int32_t* ctx_dev, int ctx, void* workspace, size_t ws_bytes,
                      emu_stream_t s);
/* final RMSNorm (+ lm_head): rows [M, hidden] -> normed [M, hidden] / logits [M, ld] */
int emu_llama_final_norm(emu_llama* m, const void* hidden, void* out, int rows, emu_stream_t s);
int emu_llama_logits(emu_llama* m, const void* hidden, int ldh, int M, void* logits, int ld, void* workspace,
                     size_t ws_bytes, emu_stream_t s);
/* one greedy decode step entirely on the device (graph-capturable): embed(cur_ids) -> layers -> logits ->
 * argmax -> out_ids[step_dev[0], :] = cur_ids = next; pos/slot/ctx/step advance by one.
 * state: device int32 arrays cur_ids[B], pos[B], slot[B], ctx[1], step[1]; out_ids [max_new, B]. */
int emu_llama_greedy_step(emu_llama* m, int B, int32_t* cur_ids, int32_t* pos, int32_t* slot,
                          const int32_t* kstart, int32_t* ctx_dev, int32_t* step_dev, int32_t* out_ids,
                          int ctx_upper, void* hidden, void* logits, int ld_logits, void* workspace,
                          size_t ws_bytes, emu_stream_t s);

/* emu_llama_greedy_step with emu_sample_bf16 in the place of the arg-max (emu.py:213-229 with do_sample / repetition_penalty; the
 * demo's chat.py:86-148): embed(cur_ids) -> layers -> logits -> select -> out_ids[step_dev[0], :] = cur_ids = next; pos / slot / ctx /
 * step advance by one.  out_ids [max_new, B] is also the history the penalty reads; uniforms fp32 [max_new, B] (may be NULL without
 * do_sample); unfinished int32 [B].  Graph-capturable: one captured step replays for every token. */
int emu_llama_sample_step(emu_llama* m, int B, int32_t* cur_ids, int32_t* pos, int32_t* slot, const int32_t* kstart,
                          int32_t* ctx_dev, int32_t* step_dev, int32_t* out_ids, int max_new, int ctx_upper, void* hidden,
                          void* logits, int ld_logits, void* workspace, size_t ws_bytes, const float* uniforms,
                          int32_t* unfinished, const emu_sample_params* params, emu_stream_t s);
/* emu_llama_sample_step with emu_sample_trie_bf16 as its selection (constrained greedy / constrained sampling with one beam, the
 * one-beam form of Emu1/mm_eval/models/emu.py:96-109): node int32 [B] is the rows' trie state, advanced on the device.  Capturable. */
int emu_llama_sample_step_trie(emu_llama* m, int B, int32_t* cur_ids, int32_t* pos, int32_t* slot, const int32_t* kstart,
                               int32_t* ctx_dev, int32_t* step_dev, int32_t* out_ids, int max_new, int ctx_upper, void* hidden,
                               void* logits, int ld_logits, void* workspace, size_t ws_bytes, const float* uniforms,
                               int32_t* unfinished, const emu_sample_params* params, const emu_token_trie* trie, int32_t* node,
                               emu_stream_t s);
/* emu_llama_sample_step with emu_sample_ngram_bf16 as its selection (lm.generate(num_beams=1, no_repeat_ngram_size=n),
 * Emu1/models/modeling_emu.py:115,177): the history the ban reads is out_ids, the ids of steps 0 .. step - 1, as for the penalty.
 * ngram is a scalar of the launch: a captured step holds the value it was captured with.  -22: ngram < 0, the parent's refusals. */
int emu_llama_sample_step_ngram(emu_llama* m, int B, int32_t* cur_ids, int32_t* pos, int32_t* slot, const int32_t* kstart,
                                int32_t* ctx_dev, int32_t* step_dev, int32_t* out_ids, int max_new, int ctx_upper, void* hidden,
                                void* logits, int ld_logits, void* workspace, size_t ws_bytes, const float* uniforms,
                                int32_t* unfinished, const emu_sample_params* params, int ngram, emu_stream_t s);
/* emu_llama_greedy_step with the next token FORCED instead of chosen: one teacher-forced step of scoring a given continuation
 * (Emu1/models/prediction_mixin.py:36-131 ranks candidates by the LM loss of Emu1/models/modeling_llama.py:110-116; here the rows run
 * through the decode kernels, so the active weight stream -- bf16, e4m3, MXFP4 -- is the one that is scored).  With step = *step_dev:
 * embed(cur_ids) -> layers -> logits -> emu_token_logprob_bf16 against targets[step, :] (targets int32 [T, B]; lp / lse / top1
 * [T, B], each may be NULL, written at [step, :]) -> cur_ids = targets[step, :] with an ignored target replaced by id 0 (that row is
 * padding from there on) -> pos / slot / ctx / step advance by one.  Once step >= T the scoring, the forcing and the advance do
 * nothing, so a replay past the end changes no state.  Graph-capturable: one captured step replays for every token. */
int emu_llama_score_step(emu_llama* m, int B, int32_t* cur_ids, int32_t* pos, int32_t* slot, const int32_t* kstart,
                         int32_t* ctx_dev, int32_t* step_dev, const int32_t* targets, int T, int ctx_upper, void* hidden,
                         void* logits, int ld_logits, void* workspace, size_t ws_bytes, float* lp, float* lse, int32_t* top1,
                         emu_stream_t s);
/* The layer body for a chunk of T rows per sequence on top of the cache (2 <= T <= 8, B * T <= 16): hidden [B*T, hidden] in place;
 * pos0 / slot0 device int32 [B] (row i: + i); the projections take whatever kernel the engine plans for B * T rows (bf16, fp8-wide,
 * MXFP4-wide), the attention is emu_decode_chunk_bf16's launch.  ctx_upper sizes the launches (>= max slot0 + T); ctx_dev is not read.
 * workspace: emu_llama_chunk_workspace_bytes.  Refused with -22 and a message: shared-prefix KV rows, the fused decode modes 1-4,
 * B * T > 16, tensor parallelism.  emu_llama_forward is not involved. */
size_t emu_llama_chunk_workspace_bytes(const emu_llama* m, int B, int T);
int emu_llama_forward_chunk(emu_llama* m, void* hidden, int B, int T, const int32_t* pos0, const int32_t* slot0, const int32_t* kstart,
                            const int32_t* ctx_dev, int ctx_upper, void* workspace, size_t ws_bytes, emu_stream_t s);
/* One step of prompt-lookup speculative greedy decoding (lm.generate(prompt_lookup_num_tokens=k), reached through the **kwargs of
 * Emu2/emu/emu.py:175,228), one sequence: embed(cur [T = 1 + k]) -> emu_llama_forward_chunk -> final norm + logits on the T rows
 * (logits [T, ld_logits], hidden [T, hidden]) -> emu_lookup_select_bf16.  Every emitted id is the arg-max of the model's own logits.
 * Graph-capturable: every index is read from the device, one captured step replays for every iteration. */
int emu_llama_lookup_step(emu_llama* m, int T, int32_t* cur, int32_t* amax, int32_t* st, int32_t* pos0, int32_t* slot0,
                          const int32_t* kstart, int32_t* ctx_dev, int32_t* out_ids, int32_t* hist, int hist_cap, const int32_t* drafts,
                          int max_ngram, int max_new, int min_len, int eos_id, int stop_on_eos, int ctx_upper, void* hidden,
                          void* logits, int ld_logits, void* workspace, size_t ws_bytes, emu_stream_t s);
/* emu_llama_lookup_step with emu_lookup_sample_bf16 as its selection: one step of prompt-lookup speculative decoding under sampling
 * or a repetition penalty (lm.generate(prompt_lookup_num_tokens=k, do_sample=True, temperature, top_p, ...), the chat demo's mode,
 * Emu2/emu/chat.py:86-148).  uniforms: fp32 [uni_rows], indexed by output position.  Graph-capturable like its parent.  -22, nothing
 * launched: params NULL, the vocabulary above EMU_SAMPLE_MAX_VOCAB, do_sample without uniforms, the parent's refusals. */
int emu_llama_lookup_sample_step(emu_llama* m, int T, int32_t* cur, int32_t* amax, int32_t* st, int32_t* pos0, int32_t* slot0,
                                 const int32_t* kstart, int32_t* ctx_dev, int32_t* out_ids, int32_t* hist, int hist_cap,
                                 const int32_t* drafts, int max_ngram, int max_new, int min_len, int eos_id, int stop_on_eos,
                                 int ctx_upper, void* hidden, void* logits, int ld_logits, void* workspace, size_t ws_bytes,
                                 const emu_sample_params* params, const float* uniforms, int uni_rows, emu_stream_t s);
/* One step of transformers' beam search (lm.generate(num_beams=N), Emu2/emu/emu.py:163-172,213-229: the library's BeamSearchScorer
 * logic in its vectorised form), deterministic mode, in two launches: log-softmax of the N beams' logit rows of every prompt, the 2N
 * best continuations over beams x vocabulary of (log p + running score) with EOS masked while cur < min_len, then the bookkeeping --
 * the N best non-finished candidates keep running; candidates among the first N that hit EOS or the length limit L compete with the
 * kept results at score / len ** length_penalty; the early-stopping heuristic (early_stopping=False) clears heuristic_open[b] when
 * no continuation can beat the worst kept result any more.  hf431 selects the scorer conventions: 0 = transformers 5.x (the library
 * installed beside this repo, which the golden fixtures pin: every ending hypothesis is scored over cur + 1 tokens, the heuristic
 * looks at the best running beam); 1 = transformers 4.31, the release the reference pins (Emu2/requirements.txt:2;
 * BeamHypotheses.add divides an EOS hypothesis by the cur tokens ahead of the EOS, is_done looks at the best of all 2N candidates,
 * finalize adds the running beams at the length limit unless the prompt is done) -- restated from that release, not runnable here.
 * cur: tokens generated so far; cur_dev (device int32, may be NULL) overrides it so that a captured hipGraph replays the step for
 * every token (steps with cur >= L do nothing).
 * logits row of (prompt b, beam j) = logits + b * ld_prompt + j * ld_beam elements (step 0: ld_beam = 0).  State, updated in
 * place (device): running_seq / sequences int32 [B, nb, L], running_scores / beam_scores f32 [B, nb] (initial: running (0, -1e9, ...),
 * kept -1e9), finished u8 [B, nb], seq_len int32 [B, nb], heuristic_open u8 [B] (initial 1).  Out: next_tok int32 [B * nb] (the tokens
 * to feed), beam_flat int64 [B * nb] (cache row b * nb + beam each of them continues).  nb <= 8, L <= 256, cur < L.
 * workspace: emu_beam_step_workspace_bytes(B, nb, V) of device scratch (per-chunk partial results of the first of the two launches). */
size_t emu_beam_step_workspace_bytes(int B, int nb, int V);
int emu_beam_step_bf16(const void* logits, long ld_prompt, long ld_beam, int V, int B, int nb, int L, int cur, const int32_t* cur_dev,
                       int min_len, int eos_id, float length_penalty, int hf431, int32_t* running_seq, int32_t* sequences,
                       float* running_scores, float* beam_scores, unsigned char* finished, int32_t* seq_len,
                       unsigned char* heuristic_open, int32_t* next_tok, long* beam_flat, void* workspace, size_t ws_bytes,
                       emu_stream_t s);
/* emu_beam_step_bf16 under a constraint (lm.generate(num_beams=5, prefix_allowed_tokens_fn=...), Emu1/mm_eval/models/emu.py:96-109):
 * the mask acts on the per-beam LOG-PROBABILITIES -- the log-sum-exp is taken over the whole, unmasked row, exactly as for the
 * min-length suppress -- so fewer than 2N candidates may be finite; ties, those among -inf included, go to the lower flat index
 * beam * V + id.  node: device int32 [B * nb], in/out (all 0 = the root at step 0): beam j of prompt b is masked by node[b * nb + j],
 * and after the bookkeeping the new beam j takes child(node[beam it continues], next_tok[j]): the state follows beam_flat.  With
 * every id an edge of every beam's node the outputs are emu_beam_step_bf16's bit for bit.  A step with cur >= L changes nothing.
 * -22, nothing launched: emu_beam_step_bf16's bounds, trie or node NULL, a table NULL, nodes < 1, edges < 0. */
int emu_beam_step_trie_bf16(const void* logits, long ld_prompt, long ld_beam, int V, int B, int nb, int L, int cur, const int32_t* cur_dev,
                            int min_len, int eos_id, float length_penalty, int hf431, int32_t* running_seq, int32_t* sequences,
                            float* running_scores, float* beam_scores, unsigned char* finished, int32_t* seq_len,
                            unsigned char* heuristic_open, int32_t* next_tok, long* beam_flat, void* workspace, size_t ws_bytes,
                            const emu_token_trie* trie, int32_t* node, emu_stream_t s);
/* emu_beam_step_bf16 with the no-repeat n-gram ban (lm.generate(num_beams=N, no_repeat_ngram_size=n),
 * Emu1/models/modeling_emu.py:115,177; the rule is emu_sample_ngram_bf16's, the history of beam j of prompt b being
 * running_seq[b, j, :cur], which follows the beams).  Like the min-length suppress and the constraint the ban acts on the per-beam
 * LOG-PROBABILITIES: the log-sum-exp is taken over the whole row, a banned id is -inf, and ties, those among -inf included, go to
 * the lower flat index.  The caller keeps V >= L + 1 + 2 * nb so that every beam keeps 2N finite continuations.  ngram = 0:
 * emu_beam_step_bf16's outputs bit for bit.  A step with cur >= L changes nothing.
 * -22, nothing launched: ngram < 0, emu_beam_step_bf16's bounds. */
int emu_beam_step_ngram_bf16(const void* logits, long ld_prompt, long ld_beam, int V, int B, int nb, int L, int cur, const int32_t* cur_dev,
                             int min_len, int eos_id, float length_penalty, int hf431, int32_t* running_seq, int32_t* sequences,
                             float* running_scores, float* beam_scores, unsigned char* finished, int32_t* seq_len,
                             unsigned char* heuristic_open, int32_t* next_tok, long* beam_flat, void* workspace, size_t ws_bytes,
                             int ngram, emu_stream_t s);

/* One step of the library's beam-search multinomial sampling (lm.generate(num_beams=N, do_sample=True, temperature, top_k, top_p,
 * repetition_penalty): the call of the demo backend, demo/backend/pytorch_model/backend.py:179-186) and of penalised beam search
 * (do_sample = 0 with a repetition penalty), in two launches; the specification is emu_amd/sampling.py (beam_reference_*).  Per beam
 * row: lp = x - logsumexp(x); repetition penalty once per distinct id of running_seq[b, j, :cur] (lp < 0 ? lp * pen : lp / pen);
 * lp[eos_id] = -inf while cur < min_len; then do_sample = 0: acc = lp + running score; do_sample = 1: temperature, top-k, top-p
 * (emu_sample_bf16's rules, min_keep forced to at least 2) on lp with the running score added afterwards (warp_accumulated = 0, the
 * order of transformers 5.x) or on lp + running score (warp_accumulated = 1, beam_sample of transformers 4.31).  Per prompt, over the
 * flattened [nb * V] scores: do_sample = 0: the 2N best, ties to the lower flat index; do_sample = 1: 2N draws without replacement
 * from softmax(acc), draw k taking the lowest flat index not yet drawn whose inclusive cumulative mass over the not-yet-drawn
 * entries exceeds u_k * (the mass that remains) (rounding left it at or beyond the total: the highest remaining entry of positive
 * mass; no mass left: the lowest not-yet-drawn flat index of finite score), sorted by score (stable) when warp_accumulated.  Then
 * emu_beam_step_bf16's bookkeeping, with its arguments and state (params->suppress_id, eos_id and pad_id are not read: eos_id and
 * min_len are the step's own).  uniforms: fp32 [uni_rows, B, 2 * nb] in [0, 1), the step reads row min(cur, uni_rows - 1); needed
 * when do_sample.  draws_out (may be NULL): int32 [B, 2 * nb] flat indices in draw order, before the sort; acc_out (may be NULL):
 * fp32 [B * nb] rows ld_acc apart receive acc, -inf for removed ids.  workspace: emu_beam_sample_workspace_bytes(B, nb, V).
 * No allocation, no synchronisation: capturable.  The same inputs give the same outputs bit for bit.
 * -22, nothing launched or written: V > EMU_SAMPLE_MAX_VOCAB, V < 2 * nb, nb > 8, L > 256, a missing pointer, a workspace too small. */
size_t emu_beam_sample_workspace_bytes(int B, int nb, int V);
int emu_beam_sample_step_bf16(const void* logits, long ld_prompt, long ld_beam, int V, int B, int nb, int L, int cur, const int32_t* cur_dev,
                              int min_len, int eos_id, float length_penalty, int hf431, int32_t* running_seq, int32_t* sequences,
                              float* running_scores, float* beam_scores, unsigned char* finished, int32_t* seq_len,
                              unsigned char* heuristic_open, int32_t* next_tok, long* beam_flat, void* workspace, size_t ws_bytes,
                              const emu_sample_params* params, int warp_accumulated, const float* uniforms, int uni_rows,
                              int32_t* draws_out, float* acc_out, long ld_acc, emu_stream_t s);
/* emu_beam_sample_step_bf16 with the no-repeat n-gram ban (Emu1/models/modeling_emu.py:115,177; the rule is
 * emu_sample_ngram_bf16's over running_seq[b, j, :cur]): lp[banned] = -inf after the repetition penalty and ahead of the EOS
 * suppress, so the warpers and the draws run over what is left.  ngram = 0: emu_beam_sample_step_bf16's outputs bit for bit.
 * -22, nothing launched or written: ngram < 0, emu_beam_sample_step_bf16's bounds. */
int emu_beam_sample_step_ngram_bf16(const void* logits, long ld_prompt, long ld_beam, int V, int B, int nb, int L, int cur,
                                    const int32_t* cur_dev, int min_len, int eos_id, float length_penalty, int hf431, int32_t* running_seq,
                                    int32_t* sequences, float* running_scores, float* beam_scores, unsigned char* finished,
                                    int32_t* seq_len, unsigned char* heuristic_open, int32_t* next_tok, long* beam_flat, void* workspace,
                                    size_t ws_bytes, const emu_sample_params* params, int warp_accumulated, const float* uniforms,
                                    int uni_rows, int32_t* draws_out, float* acc_out, long ld_acc, int ngram, emu_stream_t s);

/* Loop state of EmuModel.generate_image (emu.py:92-153, KV-cached form: step j feeds project_up(project_down(h_{j-1}))) on the
 * device, so that {project_up, decoder step, final norm, project_down, this} is captured once and replayed n_query - 1 times:
 * out_all[step_dev[0]] = prev = src ([B, cols] bf16: the step's visual embedding), pos[b]++, slot[b]++, step_dev[0]++. */
int emu_regress_advance_bf16(const void* src, void* out_all, void* prev, int32_t* pos, int32_t* slot, int32_t* step_dev, int B,
                             int cols, emu_stream_t s);

/* The host work of a beam step moved to the device, so that {advance, re-order, embed, decoder step, logits, emu_beam_step_bf16} can
 * be captured once and replayed for every token (the reference's default decoding mode must not run at the speed of the host):
 * emu_beam_advance phase 0: slot[i] = slot0 + cur - 1, pos[i] = pos0[i] + cur - 1 for the step that feeds token cur - 1 (cur read
 *   from cur_dev; rows = prompts x beams); phase 1: cur_dev += 1.  Nothing happens once cur >= L.
 * emu_llama_beam_reorder_kv: transformers' _reorder_cache for the generated slots [slot0, slot0 + cur - 1) of the engine's current
 *   cache (rows in groups of `beams`; the shared prompt slots never move): row r takes the slots of row beam_flat[r], in place. */
int emu_beam_advance(int32_t* cur_dev, int32_t* pos, int32_t* slot, const int32_t* pos0, int slot0, int rows, int L, int phase,
                     emu_stream_t s);
int emu_llama_beam_reorder_kv(emu_llama* m, const long* beam_flat, const int32_t* cur_dev, int beams, int slot0, int L,
                              emu_stream_t s);

/* Contrastive search (lm.generate(penalty_alpha = a, top_k = k), Emu2/emu/emu.py:167,223) with its token loop on the device; the
 * specification is emu_amd/sampling.py (contrastive_reference_candidates / contrastive_reference_select).  One step is {advance phase
 * 0, pick, embedding gather of cand_ids, emu_llama_forward on the B * k candidate rows, emu_llama_final_norm, emu_llama_logits, score,
 * keep, advance phase 1}; every launch reads the step from step_dev (device int32[1]) and does nothing once step >= L, so one captured
 * hipGraph replays for every token and replays beyond the end are harmless.  No allocation, no synchronisation: capturable.  The same
 * inputs give the same outputs bit for bit (every sum has a fixed order, no floating-point atomics).
 *
 * emu_contrastive_pick_bf16: per prompt b, from the bf16 logit row b * k + sel[b] (rows ld elements apart; sel NULL = 0):
 *   s = float32(logit); repetition penalty once per distinct id of hist[t * hist_ld + b], t < step (s < 0 ? s * pen : s / pen, ids
 *   outside [0, V) ignored; hist may be NULL); s[eos_id] = -inf while step < min_len (eos_id < 0 = off); p = softmax(s) (blocked
 *   fixed-order fp32 sums); cand_ids int32 [B * k] / cand_p fp32 [B * k] receive the k largest in descending order, ties to the
 *   lower id.
 * emu_contrastive_score (two launches): ctx_n fp32 [B, Lc, H] holds the context rows ALREADY divided by their norms; the valid rows
 *   of prompt b are [kstart[b], S + step) (kstart NULL = 0; rows outside are never read).  cand: bf16 [B * k, H], the candidates'
 *   final-normed hidden rows.  pen[b, j] = max over the valid rows of dot(ctx_n row, cand row) / |cand row| (the dot products in
 *   fp32, the norm from an fp64 sum; identical candidates get identical penalties); score = (1 - alpha) * cand_p - alpha * pen; the
 *   first maximum wins.  Then, for a prompt whose unfinished flag (int32 [B]) is set: out_ids[step * B + b] = the kept id, the flag
 *   is cleared when that id is eos_id, sel[b] = the kept index, ctx_n[b, S + step] = the kept row / its norm, pen_out (fp32 [B * k],
 *   may be NULL) = pen.  A finished prompt gets out_ids[step * B + b] = pad_id and nothing else of it is written.  Phase 1 gives
 *   every EMU_CONTRASTIVE_CHUNK_ROWS context rows a workgroup (chunks beyond S + step exit at once) and leaves per-chunk maxima in
 *   the workspace: emu_contrastive_workspace_bytes(B, k, Lc).
 * emu_llama_contrastive_keep_kv: cache slot slot0 + step of row b * k + sel[b] goes to its k - 1 siblings, in every layer, K and V, of
 *   the engine's current cache (rows in groups of k; nothing else moves).
 * emu_contrastive_advance phase 0: slot[i] = slot0 + step, pos[i] = pos0[i] + step (rows = B * k); phase 1: step_dev += 1.
 * -22, nothing launched or written: k < 1 or k > EMU_CONTRASTIVE_MAX_K, V > EMU_SAMPLE_MAX_VOCAB, V < k, H not a multiple of 4 or
 * above EMU_CONTRASTIVE_MAX_HIDDEN, Lc < S + L, slot0 + L beyond the cache, rows not a multiple of k, a missing pointer (those not
 * marked optional above), a workspace too small. */
#define EMU_CONTRASTIVE_MAX_K 8
#define EMU_CONTRASTIVE_CHUNK_ROWS 8
#define EMU_CONTRASTIVE_MAX_HIDDEN 8192 /* k x H bf16 candidate rows in the CU's LDS */
int emu_contrastive_pick_bf16(const void* logits, int ld, int V, int B, int k, int L, const int32_t* sel, const int32_t* hist, int hist_ld,
                              const int32_t* step_dev, float repetition_penalty, int eos_id, int min_len, int32_t* cand_ids,
                              float* cand_p, emu_stream_t s);
size_t emu_contrastive_workspace_bytes(int B, int k, int Lc);
int emu_contrastive_score(float* ctx_n, const void* cand, const int32_t* cand_ids, const float* cand_p, const int32_t* kstart,
                          const int32_t* step_dev, int B, int k, int H, int S, int L, int Lc, float alpha, float one_minus_alpha,
                          int eos_id, int pad_id, int32_t* out_ids, int32_t* unfinished, int32_t* sel, float* pen_out, void* workspace,
                          size_t ws_bytes, emu_stream_t s);
int emu_llama_contrastive_keep_kv(emu_llama* m, const int32_t* sel, const int32_t* step_dev, int k, int slot0, int L, emu_stream_t s);
int emu_contrastive_advance(int32_t* step_dev, int32_t* pos, int32_t* slot, const int32_t* pos0, int slot0, int rows, int L, int phase,
                            emu_stream_t s);

/* ---- EVA-CLIP ViT engine -------------------------------------------------------------------------------
 * EVAVisionTransformer.forward_features (eva_vit.py:402-431), post-norm blocks (:296-300), naive attention
 * (:182-252) with heads zero-padded from head_width to 128 at pack time (see emu_amd/vit.py):
 *   wqkv [3*Hh*128, C] (+ bqkv [3*Hh*128] = q_bias | 0 | v_bias), wproj [C, Hh*128], fc1 [F, C], fc2 [C, F]. */
typedef struct {
    int image_size, patch_size, width, layers, heads, head_width, mlp_hidden, kpad;
    float ln_eps;
    int prenorm;   /* 0: Emu2 post-norm blocks (eva_vit.py:298-300); 1: Emu1 EVA-CLIP-g pre-norm blocks
                      (Emu1/models/eva_vit_model.py:409-416: x += attn(LN1(x)); x += mlp(LN2(x))) */
} emu_vit_cfg;
int emu_vit_create(emu_ctx* ctx, const emu_vit_cfg* cfg, emu_vit** out);
void emu_vit_destroy(emu_vit* m);
int emu_vit_set_stem(emu_vit* m, const void* wpatch, const void* bpatch, const void* cls, const void* pos);
int emu_vit_set_block(emu_vit* m, int layer, const void* wqkv, const void* bqkv, const void* wproj,
                      const void* bproj, const void* ln1w, const void* ln1b, const void* fc1w, const void* fc1b,
                      const void* fc2w, const void* fc2b, const void* ln2w, const void* ln2b);
/* Optional W8A8 mode of the encoder blocks (not a reference feature -- the reference runs bf16 end to end; BASELINE.json
 * configs[4] names an fp8 MFMA path): e4m3 copies of the four matrices of a block (emu_quantize_fp8_rows of the PACKED bf16
 * matrices registered with emu_vit_set_block: bytes [N, K] + one fp32 scale per output row).  With emu_vit_use_fp8(m, 1) every
 * GEMM of a block quantises its activation rows (per-row e4m3) and runs on emu_linear_fp8_bf16's kernels; LayerNorm, attention
 * and the stem stay bf16.  width and mlp_hidden must be multiples of 128.  Registering changes emu_vit_workspace_bytes. */
int emu_vit_set_block_fp8(emu_vit* m, int layer, const void* wqkv8, const float* sqkv, const void* wproj8, const float* sproj,
                          const void* fc1w8, const float* sfc1, const void* fc2w8, const float* sfc2);
int emu_vit_use_fp8(emu_vit* m, int enable);
/* Launch fusions of the encoder blocks (all on by default; 0 = the launch sequence of rounds 1-3, for A/B timing and parity):
 * bit 0: with one image the V heads leave the qkv projection key-contiguous (no transpose launch); bit 1: the K-slice sum of a
 * post-norm block's fc2 applies bias, LayerNorm and the residual add row-wise in the same launch (no reduce + layernorm launches).
 * Bit-identical tokens either way. */
int emu_vit_set_fusion(emu_vit* m, int mask);
size_t emu_vit_workspace_bytes(const emu_vit* m, int B);
/* image NCHW (fp32 or bf16) -> tokens [B, 1+g*g, C] bf16 (raw block output incl. cls, eva_vit.py:433-445) */
int emu_vit_forward(emu_vit* m, const void* image, int image_is_f32, int B, void* out_tokens, void* workspace,
                    size_t ws_bytes, emu_stream_t s);

/* Parity hook: blocks [l0, l1) of the encoder in place on tokens [B, 1+g*g, C] bf16 (what emu_vit_forward runs after the stem
 * for l0 = 0, l1 = layers); the full-size tests compare every block on a common input.  Same workspace as emu_vit_forward. */
int emu_vit_blocks(emu_vit* m, void* tokens, int B, int l0, int l1, void* workspace, size_t ws_bytes, emu_stream_t s);

/* Token-parallel encode of ONE image across tensor-parallel ranks (emu_amd/vit.py: VitEngine.init_token_parallel): rank r computes
 * token rows [r0, r1) of the stem and of every block (emu_amd/tp.py::token_rows: 8-row groups, CLS on rank 0, balanced; a trailing
 * rank may own none).  Every rank holds the whole encoder; after each block's qkv projection the ranks exchange their K rows and
 * V^T key columns over IPC-mapped exchange regions (csrc/p2p.hip, the one-shot all-reduce's protocol and give-up counter,
 * emu_tp_p2p_giveups), attention runs over all N keys, and the final tokens are gathered once: every rank returns the same bytes.
 * emu_vit_set_token_parallel: this rank and the world size (1 <= world <= 8); emulate != 0 skips every exchange (timing tools:
 * only this rank's rows are right).  world >= 2: emu_vit_tp_create exports this rank's region (64-byte IPC handle), then
 * emu_vit_tp_open maps every rank's (world x 64 bytes in rank order; timeout_ms bounds every wait, 0 = 10 s; fenced as
 * emu_tp_p2p_set_fenced).  emu_vit_forward_tp is collective over the ranks and takes emu_vit_forward's workspace for B = 1;
 * out_tokens [1+g*g, C].  The fp8 blocks have no token-parallel form: -22.  emu_vit_tp_rows: the rows the last call computed. */
int emu_vit_set_token_parallel(emu_vit* m, int rank, int world, int emulate);
int emu_vit_tp_create(emu_vit* m, void* handle64_out);
int emu_vit_tp_open(emu_vit* m, const void* handles, int timeout_ms, int fenced);
int emu_vit_forward_tp(emu_vit* m, const void* image, int image_is_f32, void* out_tokens, void* workspace, size_t ws_bytes,
                       emu_stream_t s);
int emu_vit_tp_rows(const emu_vit* m, int* r0, int* r1);

/* ---- SDXL-style UNet denoise engine ---------------------------------------------------------------------
 * One call = one iteration of EmuVisualGeneration's denoising loop (Emu2/emu/diffusion.py:130-149):
 * cat([latents]*2) -> scheduler.scale_model_input -> UNet2DConditionModel (conf/diffusion_config/unet/config.json)
 * -> chunk(cond, uncond) -> guidance -> EulerDiscreteScheduler.step (conf/.../scheduler_config.json).
 * Weights are registered by PACKED name (see emu_amd/unet.py: conv weights [Cout, 3,3,Cin], fused attn1 qkv / attn2 kv,
 * interleaved GEGLU rows, all time_emb_proj concatenated into temb_proj_all).  Parity of this path is UNPINNED
 * (diffusers is not available to run; see oracle/unet_ref.py). */
/* GroupNorm(groups, eps)(+SiLU) over an NHWC activation [B, HW, C] (diffusers ResnetBlock2D / Transformer2DModel norms) */
size_t emu_groupnorm_ws_bytes(int B, int HW, int C);
int emu_groupnorm_nhwc_bf16(const void* x, const void* gamma, const void* beta, void* y, void* ws, int B, int HW, int C,
                            int groups, float eps, int silu, emu_stream_t s);
/* 3x3 convolution, padding 1, as an implicit GEMM over NHWC input [B,Hin,Win,Cin] (Cin % 64 == 0), weights
 * [Cout, 3, 3, Cin].  mode 1: stride 1; 2: stride 2 (Downsample2D); 3: nearest x2 upsample fused (Upsample2D).
 * y = bf16(res + bf16(bf16(conv + bias) + bias2[b]))  (bias2: per-batch rows, e.g. the time embedding projection) */
int emu_conv3x3_nhwc_bf16(const void* x, const void* w, const void* bias, const void* bias2, int ld_bias2, const void* res,
                          void* y, int B, int Hin, int Win, int Cin, int Cout, int mode, emu_stream_t s);

typedef struct emu_unet emu_unet;
typedef struct {
    int in_ch, out_ch;
    int ch[3];
    int layers_per_block;
    int depth[3], heads[3], attn[3];
    int cross_dim, groups;
    float gn_eps;
    int temb_dim, kpad_in;
} emu_unet_cfg;
int emu_unet_create(emu_ctx* ctx, const emu_unet_cfg* cfg, emu_unet** out);
void emu_unet_destroy(emu_unet* u);
int emu_unet_set_weight(emu_unet* u, const char* name, const void* ptr);
int emu_unet_finalize(emu_unet* u);                       /* -2 + emu_last_error: first missing tensor        */
/* Launch fusions of the transformer blocks (default: every one whose packed tensors are registered).  Bit 0: LayerNorm folded
 * into the consumer GEMM (needs "<block>attn1.qkv.wln/.c/.d", "attn2.q.wln/.c/.d", "ff.geglu.wln/.c/.d": W * gamma, its fp32
 * row sums, W @ beta + bias); bit 1: V^T written by the qkv projection's epilogue (no transpose launch); bit 2: the cross-attention
 * over the (<= 64) prompt tokens runs inside the attn2.to_q projection's epilogue (no q tensor, no attention launch).  0 = the
 * unfused launch sequence (A/B timing, parity of fused vs unfused).  Returns the mask in effect. */
int emu_unet_set_fusion(emu_unet* u, int mask);
/* Optional W8A8 mode of the transformer blocks (not a reference feature; BASELINE.json configs[4] names an fp8 MFMA path).
 * Register every block's six packed matrices (attn1.qkv.w, attn1.out.w, attn2.q.w, attn2.out.w, ff.geglu.w, ff.out.w) a second
 * time with emu_unet_set_weight as "<name>.fp8" (the e4m3 bytes of emu_quantize_fp8_rows) and "<name>.fp8s" (fp32 row
 * scales), then emu_unet_use_fp8(u, 1): the blocks' GEMMs run on emu_linear_fp8_bf16's kernels, the three LayerNorms of a
 * block emit the consumer's fp8 rows themselves, the attention outputs and the GEGLU product are quantised per row by a launch
 * of their own; convs, GroupNorm, proj_in / proj_out, attention and the scheduler stay bf16.  Of emu_unet_set_fusion's bits the
 * V^T stores (1) and the cross-attention epilogue (2) stay in effect -- they work on finished sums -- the LayerNorm fold (0) has
 * no fp8 form.  Changes emu_unet_workspace_bytes; returns -2 when a copy is missing. */
int emu_unet_use_fp8(emu_unet* u, int enable);
/* CPU test hook (tests/test_unet_block_plan.py): the one rule by which a transformer's blocks pick their GEMM format and their
 * fusions -- host arithmetic on integers, no HIP call, no engine.  fp8 0 / 1 as emu_unet_use_fp8 takes it, fusion 0..7 the mask in
 * effect (emu_unet_set_fusion), M = rows of the token stream (batch elements x HW: 2 x HW for the CFG pair, HW for one row of it),
 * C = the transformer's channels, HW = tokens per batch element, n_ctx = prompt tokens, depth = its blocks.  Returns a bit set:
 *   1  fp8: the six GEMMs of a block run W8A8 (fp8 on, M > 8, C a multiple of 128 and <= 2048)
 *   2  ln_fold: the LayerNorms are folded into their consumer GEMMs (not fp8, fusion bit 0, M > 8, C a multiple of 128)
 *   4  vt_epilogue: the qkv projection stores V^T (fusion bit 1, M > 8, HW a multiple of 64)
 *   8  cross_epilogue: cross-attention inside the to_q projection (fusion bit 2, M > 8, HW a multiple of 64, n_ctx <= 64)
 *  16  prefetch: every GEMM of the chain requests its successor's weights (not fp8, M > 8, depth > 0)
 * M <= 8 is the few-row stream, which fuses nothing: 0.  -22: an argument outside its range, or M no multiple of HW. */
int emu_unet_block_plan(int fp8, int fusion, int M, int C, int HW, int n_ctx, int depth);
int emu_unet_temb_total(const emu_unet* u);               /* rows of temb_proj_all (sum of resnet out channels) */
size_t emu_unet_workspace_bytes(const emu_unet* u, int H, int W);
size_t emu_unet_context_bytes(const emu_unet* u, int n_ctx);
/* once per prompt: cross-attention K / V^T of every block from ctx_tokens [2, n_ctx, cross] (cond FIRST,
 * diffusion.py:202,210) and the text_time embedding from add_in [2, add_dim] = cat(mean(prompt), Timesteps(time_ids)) */
int emu_unet_set_context(emu_unet* u, const void* ctx_tokens, int n_ctx, const void* add_in, int add_dim, void* cache,
                         size_t cache_bytes, void* workspace, size_t ws_bytes, emu_stream_t s);
/* one denoise step in place on latents NCHW [1, 4, H, W] bf16.  temb_table [steps, ch0] bf16 = Timesteps(t_i);
 * sigmas [steps+1] fp32; step_dev: device int32 step index, incremented by the call (graph replay advances it). */
int emu_unet_step(emu_unet* u, void* latents, int H, int W, const void* temb_table, const void* sigmas, int32_t* step_dev,
                  float guidance, void* workspace, size_t ws_bytes, emu_stream_t s);
/* bare UNet forward (parity tests): eps_out NHWC [2*H*W, 4] for cat([latents]*2) / sqrt(sigmas[step]^2 + 1) */
int emu_unet_forward(emu_unet* u, const void* latents, int H, int W, const void* temb_table, const void* sigmas,
                     const int32_t* step_dev, void* eps_out, void* workspace, size_t ws_bytes, emu_stream_t s);
/* Classifier-free guidance split over a rank pair (Emu2/emu/diffusion.py:131-145 runs cat([latents] * 2) through the
 * UNet and chunk(2)s the prediction): half = 0 / 1 makes emu_unet_forward compute ONLY the cond / uncond row of the pair (batch 1;
 * eps_out is then [H*W, 4]) against the context emu_unet_set_context cached for both rows; -1 (default) restores the pair.  The
 * ranks exchange their halves (131 KB per step at 128 x 128 latents) and each applies emu_unet_cfg_euler_step -- guidance + Euler
 * update of emu_unet_step on eps_pair [2*H*W, 4] (cond first), advancing step_dev.  emu_unet_step refuses while a half is set. */
int emu_unet_set_cfg_half(emu_unet* u, int half);
int emu_unet_cfg_euler_step(emu_unet* u, const void* eps_pair, void* latents, int H, int W, const void* sigmas, int32_t* step_dev,
                            float guidance, emu_stream_t s);


#ifdef __cplusplus
}
#endif
#endif /* EMU_HIP_H */
