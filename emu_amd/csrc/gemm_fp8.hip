// fp8 (OCP e4m3fn, one fp32 scale per weight row) weights for steps of 17..64 rows (beams x batch, contrastive search on a batch) and,
// in a third form, for 65 rows and more (prompts, scoring prefills: LLaMA on the fp8 set alone): a weight-only GEMM on the bf16 matrix
// cores, W8A16
//     out[m, n] = epilogue( bf16( wscale[n] * sum_k x[m, k] * e4m3(W8[n, k]) + bias[n] ) )
//
// gemv_fp8_thin.hip streams the fp8 set for up to 16 rows: one 16-row activation tile, every converted weight fragment used by ONE
// MFMA, the k of a stage split over the four waves.  At these row counts a step is still a weight stream, so this is the tile of
// gemm_fp4.hip fed the way that kernel is fed:
//   * structure (gemm_fp4.hip; the two forms of 17..64 rows): four waves side by side along N, 64 weight rows per workgroup (grid =
//     ceil(N / 64)); a wave owns 16 weight rows x the whole activation tile (B_ x 16 rows) and walks the whole stage itself -- no k split, no reduction through
//     LDS.  K is walked in stages of 256 delivered by LDS-DMA through a ring of NSTG stages, counted vmcnt + one raw s_barrier per
//     stage; weight rows take the non-temporal path (a use-once stream), activation rows the cached one; M and N are clamped on load
//     and masked on store;
//   * operands (gemv_fp8_thin.hip, fp8_tile.h): 256 weight bytes and 512 activation bytes per row and stage, the swizzle carried by the
//     DMA source address, the LDS image lane-linear, chunk c of staged row r in slot c ^ (r & 15) -- every ds_read_b128 of 16 rows x
//     one chunk is conflict-free.  In round ku = 0..3 lane (i, g) reads ONE 16-byte chunk of its wave's weight row i, chunk 4 ku + g;
//     the chunk's two halves each become an A fragment through cvt8_e4m3 (4 x v_cvt_scalef32_pk_bf16_fp8, lossless) and each A
//     fragment feeds B_ v_mfma_f32_16x16x32_bf16 against chunk 2 (4 ku + g) + h of activation rows 16 bi + i: the 32 conversions of a
//     stage sit behind 8 * B_ matrix instructions;
//   * rounding points: those of fp8_thin_kernel -- fp32 accumulation, the row scale in fp32 ahead of the bias, then store_c4
//     (fp4_tile.h: bias, round to bf16, then the residual or SiLU(gate) * up on interleaved rows).  No fused RMSNorm.
//   form       A_ B_ WN WM   BN x BM    stage          ring   LDS       rows
//   narrow      1  2  4  1   64 x 32    16 + 16 KiB    4      128 KiB   17..32   (emu_gemm_tune bit 20: ring 2, 64 KiB, two workgroups per CU)
//   one tile    1  4  4  1   64 x 64    16 + 32 KiB    3      144 KiB   33..64
//   tile        2  4  2  2   64 x 128   16 + 64 KiB    2      160 KiB   65 and up
// The third form has the geometry of gemm_fp4.hip's prefill form: the four waves as WN x WM = 2 x 2, a wave owns A_ = 2 x 16 weight rows
// x B_ = 4 x 16 activation rows, so each converted A fragment still feeds four MFMAs; the grid is two-dimensional, grid.x over the row
// tiles and grid.y over the column tiles, so that the workgroups in flight share weight rows in L2, and the weight bytes -- re-read once
// per row tile -- take the cached LDS-DMA path (glds16).  Its ring of two whole 256-k stages is exactly the CU's 160 KiB (163840 bytes
// static: hipcc and the launch take it; the half-stage ring of three was not needed).  It keeps the k walk of the 64 x 64 form -- stages
// ascending, ku = 0..3, h = 0..1, lane (i, g) on chunk 4 ku + g, the same MFMA -- so every output element sums the same 32-k products in
// the same order: a row's result is the 64-row form's bit for bit and does not depend on how many rows share the call.
// The result is what the bf16 GEMM computes on the dequantised weights (the conversion is exact, the scale a separate fp32 factor), up to
// fp32 summation order.  Algorithmic bytes per call = N * K; the activation tile adds BM * 512 / (64 * 256) of that as L2 -> LDS traffic.
// Resources (hipcc -O3, gfx950, kernel-resource-usage remark; the largest of the three epilogues), no scratch in any instantiation:
//     narrow, ring 4:   116 VGPRs + 12 AGPRs, 131072 bytes LDS, no scratch        (one workgroup per CU)
//     narrow, ring 2:   116 VGPRs + 12 AGPRs,  65536 bytes LDS, no scratch        (two workgroups per CU)
//     one tile, ring 3:  79 VGPRs + 20 AGPRs, 147456 bytes LDS, no scratch        (one workgroup per CU)
//     tile, ring 2:      96 VGPRs + 32 AGPRs, 163840 bytes LDS, no scratch        (one workgroup per CU; the same for all three epilogues)
// Which form, which grid, which arguments are acceptable: gemv.hip::gemm_fp8w_plan (17..64 rows) and gemm_fp8t_plan (65 and up), pure host
// arithmetic (C ABI: emu_gemm_fp8w_plan, emu_gemm_fp8t_plan); launch_gemm_fp8w / launch_gemm_fp8t below are only the switch from their
// answers to template arguments, and callers come through gemv.hip::launch_gemm_fp8w_stream / launch_gemm_fp8t_stream (shape, plan,
// pointer checks, launch).
#include "common.h"
#include "kernels.h"
#include "fp8_tile.h"

using namespace emu_gemm;

namespace {

// STREAM: the two forms of 17..64 rows (grid.x over the column tiles, one row tile, use-once weight bytes); otherwise the 65-rows-and-up
// form (grid.x over the row tiles, grid.y over the column tiles, weight bytes re-read once per row tile: the cached DMA path)
template <int EPI, int A_, int B_, int WN, int WM, int NSTG, bool STREAM>
__global__ __launch_bounds__(256) void fp8_gemm_kernel(const GemvArgs a) {
    static_assert(WN * WM == 4, "four waves");
    constexpr int BN = 16 * A_ * WN, BM = 16 * B_ * WM;
    static_assert(BN == 64, "64 weight rows per workgroup in every form");
    constexpr int WI = BN / 4, XI = BM / 2, JN = (WI + XI) / 4;            // 1 KiB DMA instructions per stage: weights, activations; per wave
    static_assert(WI % 4 == 0 && XI % 4 == 0, "every wave issues the same instructions: WI / 4 of weights, then activations");
    static_assert((NSTG - 2) * JN <= 63, "vmcnt field is 6 bits");
    constexpr int WB = BN * F8_WROW, ST = WB + BM * F8_XROW;               // stage = weight rows | activation rows
    static_assert(NSTG * ST <= 160 * 1024, "a CU's LDS");
    __shared__ __attribute__((aligned(16))) char smem[NSTG * ST];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int wn = WM == 1 ? wave : wave % WN, wm = WM == 1 ? 0 : wave / WN;
    const int m0 = (STREAM ? 0 : blockIdx.x) * BM, n0 = (STREAM ? blockIdx.x : blockIdx.y) * BN;

    // DMA sources: instruction q = j * 4 + wave.  q < WI fills weight rows 4q .. 4q + 3 of the tile (lane / 16 selects, slot lane % 16;
    // rows clamped at N - 1), q >= WI activation rows 2 (q - WI), + 1 (lane / 32 selects, slot lane % 32; rows clamped at M - 1); slot p
    // of row r receives global chunk p ^ (r & 15)
    const char* src[JN];
#pragma unroll
    for (int j = 0; j < JN; ++j) {
        const int q = j * 4 + wave;
        if (j < WI / 4) {
            const int r = 4 * q + (lane >> 4), c = (lane & 15) ^ (r & 15), n = n0 + r;
            src[j] = reinterpret_cast<const char*>(a.W) + (size_t)(n < a.N ? n : a.N - 1) * a.ldw + c * 16;
        } else {
            const int r = 2 * (q - WI) + (lane >> 5), c = (lane & 31) ^ (r & 15), m = m0 + r;
            src[j] = reinterpret_cast<const char*>(a.x + (size_t)(m < a.M ? m : a.M - 1) * a.ldx) + c * 16;
        }
    }
    const int nk = a.K / F8_KC;
    auto issue = [&](int kt, int stage) {
        kt = kt < nk ? kt : nk - 1;                    // past-the-end stages re-load the last one (uniform vmcnt counts)
        char* base = smem + stage * ST;
#pragma unroll
        for (int j = 0; j < JN; ++j) {
            const int q = j * 4 + wave;
            if (j < WI / 4) {
                if constexpr (STREAM) glds16_nt(src[j] + (size_t)kt * F8_WROW, base + q * 1024);   // weight rows: a use-once stream
                else glds16(src[j] + (size_t)kt * F8_WROW, base + q * 1024);                       // ... or re-read once per row tile
            } else
                glds16(src[j] + (size_t)kt * F8_XROW, base + q * 1024);
        }
    };
    f32x4_t acc[A_][B_];
#pragma unroll
    for (int ai = 0; ai < A_; ++ai)
#pragma unroll
        for (int bi = 0; bi < B_; ++bi) acc[ai][bi] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const int woff = (wn * A_ * 16 + i) * F8_WROW;     // this lane's weight row of sub-tile 0 (A operand row i of the wave's A_ x 16)
    const int xoff = WB + (wm * B_ * 16 + i) * F8_XROW;   // ... and its activation row of sub-tile 0 (B operand column i)
#pragma unroll
    for (int t = 0; t < NSTG - 1; ++t) issue(t, t);
    for (int kt = 0; kt < nk; ++kt) {
        wait_vmcnt<(NSTG - 2) * JN>();                 // this wave's share of stage kt has landed
        __builtin_amdgcn_s_barrier();                  // ... and everyone's; everyone is done reading stage kt - 1
        issue(kt + NSTG - 1, (kt + NSTG - 1) % NSTG);
        const char* sb = smem + (kt % NSTG) * ST;
#pragma unroll
        for (int ku = 0; ku < 4; ++ku) {
            const int c = 4 * ku + g;                  // this lane's 16-byte weight chunk of the stage: k = 16 c .. 16 c + 15
            u32x4 wv[A_];
#pragma unroll
            for (int ai = 0; ai < A_; ++ai) wv[ai] = *reinterpret_cast<const u32x4*>(sb + woff + ai * 16 * F8_WROW + ((c ^ i) << 4));
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                bf16x8_t bf[B_];
#pragma unroll
                for (int bi = 0; bi < B_; ++bi)
                    bf[bi] = *reinterpret_cast<const bf16x8_t*>(sb + xoff + bi * 16 * F8_XROW + (((2 * c + h) ^ i) << 4));
#pragma unroll
                for (int ai = 0; ai < A_; ++ai) {
                    const bf16x8_t af = cvt8_e4m3(wv[ai][2 * h], wv[ai][2 * h + 1]);
#pragma unroll
                    for (int bi = 0; bi < B_; ++bi) acc[ai][bi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf[bi], acc[ai][bi], 0, 0, 0);
                }
            }
        }
    }
    wait_vmcnt<0>();                                   // the tail DMA lands before the workgroup's LDS is handed on
    // lane holds C[weight row 4g + r][activation row i] of every (ai, bi) sub-tile, r = 0..3
#pragma unroll
    for (int ai = 0; ai < A_; ++ai) {
        const int nb = n0 + (wn * A_ + ai) * 16 + 4 * g;   // first of this lane's 4 output columns
        float sc[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[r] = a.wscale[nb + r < a.N ? nb + r : a.N - 1];
#pragma unroll
        for (int bi = 0; bi < B_; ++bi) {
            const int m = m0 + (wm * B_ + bi) * 16 + i;
            if (m >= a.M) continue;
            f32x4_t v = acc[ai][bi];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] *= sc[r];     // the row scale, in fp32, ahead of the bias
            store_c4<EPI>(a, m, nb, v);
        }
    }
}

template <int A_, int B_, int WN, int WM, int NSTG, bool STREAM>
int launch_fp8_gemm(const GemvArgs& a, dim3 grid, int block, hipStream_t s) {
#define EMU_F8G_CASE(E) case E: hipLaunchKernelGGL((fp8_gemm_kernel<E, A_, B_, WN, WM, NSTG, STREAM>), grid, dim3(block), 0, s, a); break;
    EMU_EPI3(EMU_F8G_CASE)
#undef EMU_F8G_CASE
}

}  // namespace

// the built (activation rows of the tile, ring depth) combinations; gemv.hip::gemm_fp8w_plan picks among them
int launch_gemm_fp8w(const GemvArgs& a, const GemmFp8wPlan& p, hipStream_t s) {
    if (p.status) return -22;
    switch (p.bm * 10 + p.stages) {
        case 324: return launch_fp8_gemm<1, 2, 4, 1, 4, true>(a, dim3(p.grid), p.block, s);
        case 322: return launch_fp8_gemm<1, 2, 4, 1, 2, true>(a, dim3(p.grid), p.block, s);
        case 643: return launch_fp8_gemm<1, 4, 4, 1, 3, true>(a, dim3(p.grid), p.block, s);
        default: return -22;
    }
}
// the 65-rows-and-up form; gemv.hip::gemm_fp8t_plan is its plan
int launch_gemm_fp8t(const GemvArgs& a, const GemmFp8tPlan& p, hipStream_t s) {
    if (p.status || p.form != 3 || p.bm != 128 || p.stages != 2) return -22;
    return launch_fp8_gemm<2, 4, 2, 2, 2, false>(a, dim3(p.grid_x, p.grid_y), p.block, s);
}
