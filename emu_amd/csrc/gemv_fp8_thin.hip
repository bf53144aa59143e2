// fp8 (OCP e4m3fn, one fp32 scale per weight row) weight stream for few-row steps (3..16 rows: beam search, small batches,
// contrastive search) on the matrix cores:
//     out[m, n] = epilogue( bf16( wscale[n] * sum_k x[m, k] * e4m3(W8[n, k]) + bias[n] ) )
//
// gemv_fp8_kernel (gemv.hip) converts and multiplies on the VALU and is built for one or two rows; gemv_thin.hip streams bf16 weights
// for these row counts through LDS-DMA stages into v_mfma_f32_16x16x32_bf16 with no VALU in the loop.  This is that structure fed
// from bytes (W8 [N, ldw] as emu_quantize_fp8_rows writes it), weight-only: the activations stay bf16 (W8A16, as the 1-2-row stream):
//   * a workgroup (4 waves) owns RN = 16 / 32 weight rows and walks K in stages of 256: 256 bytes per weight row -- half a bf16
//     row, so a 1 KiB LDS-DMA instruction carries four weight rows or two activation rows (512 bytes each) -- NSTG stages deep
//     (as deep as lets three workgroups share a CU's LDS: 48 KiB), counted vmcnt + one raw s_barrier per stage.  Weight rows take
//     the non-temporal path (a use-once stream), activation rows the cached one;
//   * the DMA source address carries the swizzle, the LDS image is lane-linear: 16-byte chunk c of staged row r sits in slot
//     c ^ (r & 15), for the 16-slot weight rows and the 32-slot activation rows alike, which makes every 16-lane group of the
//     ds_read_b128 below conflict-free (a group holds all 16 values of i at two values of g that differ in bit 0);
//   * the k order inside an MFMA is free as long as A and B agree: lane (i, g) of wave w reads ONE 16-byte chunk of weight row i --
//     chunk 4w + g of the stage, 16 codes, k = 16 (4w + g) .. + 15 -- and spends its two halves on two MFMAs: dwords 2h, 2h + 1
//     become the A fragment through 4 x v_cvt_scalef32_pk_bf16_fp8 under scale 2^0, and the B lane reads the matching 8 k of
//     activation row i: chunk 2 (4w + g) + h.  So wave w multiplies k [64w, 64w + 64) of every stage for all RN / 16 row groups and
//     the four partial 16 x 16 products meet in LDS at the end;
//   * the epilogue multiplies the row scale in fp32, then store_c4 (fp4_tile.h): bias, round to bf16, then the residual or
//     SiLU(gate) * up -- the rounding points of thin_stream_kernel.  No fused RMSNorm: callers normalise first.
// Conversion: every e4m3 value (2^-9 .. 448) is exact in bf16, so the conversion is lossless whichever way it is done.  gfx950's
// scaled pack conversion is used because it goes from two bytes to two bf16 in ONE instruction (8 per 16 weights); the other route,
// v_cvt_pk_f32_fp8 + v_cvt_pk_bf16_f32, takes two (16 per 16 weights) for the same bits.  tests/test_gpu_fp8_wide.py pins all 254
// finite codes at every byte position of a stage.
// Rounding points against the 1-2-row kernel (gemv_fp8_kernel): that one sums on the VALU in another order and folds the fused
// norm's rinv into the scale, so the two may differ in the last bit of the bf16 result.  Accepted: a generation runs on one of them
// per row count.
// Algorithmic bytes per call = N * K.  Activations add MR * 512 / (RN * 256) of that as L2 -> LDS traffic, nothing in HBM.
// Resources (hipcc -O3, gfx950, kernel-resource-usage remark; the largest of the three epilogues), no scratch in any instantiation:
//     RN 32, MR  8, 4 stages:  40 VGPRs + 8 AGPRs, 49152 bytes LDS        RN 32, MR 16, 3 stages:  40 VGPRs + 8 AGPRs, 49152 bytes LDS
//     RN 16, MR  8, 6 stages:  32 VGPRs + 4 AGPRs, 49152 bytes LDS        RN 16, MR 16, 4 stages:  36 VGPRs + 4 AGPRs, 49152 bytes LDS
// (the LDS ring, not the registers, sets the occupancy: three workgroups per CU)
// Which instantiation, which grid, which arguments are acceptable: gemv.hip::gemv_thin_plan (weight kind fp8, family GEMV_FAM_FP8_THIN),
// the one host planner of the three few-row matrix-core streams; launch_gemv_fp8_thin below is only the switch from its answer to
// template arguments, and callers come through gemv.hip::launch_gemv_thin_stream.
#include "common.h"
#include "kernels.h"
#include "fp8_tile.h"                                   // F8_* stage constants and cvt8_e4m3, shared with gemm_fp8.hip

using namespace emu_gemm;

namespace {

template <int EPI, int RN, int MR, int NSTG>
__global__ __launch_bounds__(256) void fp8_thin_kernel(const GemvArgs a) {
    constexpr int WI = RN / 4, XI = MR / 2, LPT = (WI + XI) / 4, RG = RN / 16;    // 1 KiB DMA instructions per stage: weights, activations
    constexpr int WB = RN * F8_WROW, ST = WB + MR * F8_XROW;                      // stage = weight rows | activation rows
    static_assert((WI + XI) % 4 == 0, "every wave issues the same number of DMA instructions per stage");
    static_assert((NSTG - 2) * LPT <= 63, "vmcnt field is 6 bits");
    constexpr int RED = 4 * RG * 64 * 16;
    __shared__ __attribute__((aligned(16))) char smem[NSTG * ST > RED ? NSTG * ST : RED];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * RN;

    // DMA sources: instruction q = j * 4 + wave.  q < WI fills weight rows 4q .. 4q + 3 (lane / 16 selects, slot lane % 16; rows clamped
    // at N - 1), q >= WI activation rows 2 (q - WI), + 1 (lane / 32 selects, slot lane % 32; rows clamped at M - 1); slot p of row r
    // receives global chunk p ^ (r & 15)
    const char* src[LPT];
    int adv[LPT];                                      // bytes per stage of the instruction's rows
#pragma unroll
    for (int j = 0; j < LPT; ++j) {
        const int q = j * 4 + wave;
        if (q < WI) {
            const int r = 4 * q + (lane >> 4), c = (lane & 15) ^ (r & 15), n = n0 + r;
            src[j] = reinterpret_cast<const char*>(a.W) + (size_t)(n < a.N ? n : a.N - 1) * a.ldw + c * 16;
            adv[j] = F8_WROW;
        } else {
            const int r = 2 * (q - WI) + (lane >> 5), c = (lane & 31) ^ (r & 15);
            src[j] = reinterpret_cast<const char*>(a.x + (size_t)(r < a.M ? r : a.M - 1) * a.ldx) + c * 16;
            adv[j] = F8_XROW;
        }
    }
    const int nk = a.K / F8_KC;
    auto issue = [&](int kt, int stage) {
        kt = kt < nk ? kt : nk - 1;                    // past-the-end stages re-load the last one (uniform vmcnt counts)
        char* base = smem + stage * ST + wave * 1024;
#pragma unroll
        for (int j = 0; j < LPT; ++j) {
            if (j * 4 + wave < WI) glds16_nt(src[j] + kt * adv[j], base + j * 4096);      // weight rows: stream
            else glds16(src[j] + kt * adv[j], base + j * 4096);
        }
    };
    f32x4_t acc[RG];
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) acc[rg] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const int rb = i < a.M ? i : a.M - 1;              // this lane's activation row (B operand column i)
    const int c = 4 * wave + g;                        // this lane's 16-byte weight chunk of the stage
    const int xoff = WB + rb * F8_XROW, xs = rb & 15;
#pragma unroll
    for (int t = 0; t < NSTG - 1; ++t) issue(t, t);
    for (int kt = 0; kt < nk; ++kt) {
        wait_vmcnt<(NSTG - 2) * LPT>();                // this wave's share of stage kt has landed
        __builtin_amdgcn_s_barrier();                  // ... and everyone's; everyone is done reading stage kt - 1
        issue(kt + NSTG - 1, (kt + NSTG - 1) % NSTG);
        const char* sb = smem + (kt % NSTG) * ST;
        const bf16x8_t b0 = *reinterpret_cast<const bf16x8_t*>(sb + xoff + (((2 * c) ^ xs) << 4));
        const bf16x8_t b1 = *reinterpret_cast<const bf16x8_t*>(sb + xoff + (((2 * c + 1) ^ xs) << 4));
        u32x4 wv[RG];
#pragma unroll
        for (int rg = 0; rg < RG; ++rg) wv[rg] = *reinterpret_cast<const u32x4*>(sb + (rg * 16 + i) * F8_WROW + ((c ^ i) << 4));
#pragma unroll
        for (int rg = 0; rg < RG; ++rg) {
            acc[rg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cvt8_e4m3(wv[rg][0], wv[rg][1]), b0, acc[rg], 0, 0, 0);
            acc[rg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cvt8_e4m3(wv[rg][2], wv[rg][3]), b1, acc[rg], 0, 0, 0);
        }
    }
    wait_vmcnt<0>();                                   // drain the tail DMA before the ring is reused
    __syncthreads();
    f32x4_t (*part)[RG][64] = reinterpret_cast<f32x4_t (*)[RG][64]>(smem);
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) part[wave][rg][lane] = acc[rg];
    __syncthreads();
    // wave w finishes row group w: lane holds C[weight row 4g + r][activation row i], r = 0..3
    if (wave >= RG) return;
    f32x4_t v = part[0][wave][lane];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const f32x4_t t = part[w][wave][lane];
        v[0] += t[0]; v[1] += t[1]; v[2] += t[2]; v[3] += t[3];
    }
    const int m = i;
    if (m >= a.M) return;
    const int nb = n0 + 16 * wave + 4 * g;             // first of this lane's 4 output columns
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] *= a.wscale[nb + r < a.N ? nb + r : a.N - 1];       // the row scale, in fp32, ahead of the bias
    store_c4<EPI>(a, m, nb, v);
}

template <int RN, int MR, int NSTG>
int launch_fp8_thin(const GemvArgs& a, const GemvPlan& p, hipStream_t s) {
#define EMU_F8T_CASE(E) case E: hipLaunchKernelGGL((fp8_thin_kernel<E, RN, MR, NSTG>), dim3(p.grid), dim3(p.block), 0, s, a); break;
    EMU_EPI3(EMU_F8T_CASE)
#undef EMU_F8T_CASE
}

}  // namespace

// the built (weight rows, activation rows, ring depth) combinations; gemv.hip::gemv_thin_plan picks among them
int launch_gemv_fp8_thin(const GemvArgs& a, const GemvPlan& p, hipStream_t s) {
    switch ((p.rows * 100 + p.mb) * 10 + p.stages) {   // digits: rows, mb (two), stages
        case 32084: return launch_fp8_thin<32, 8, 4>(a, p, s);
        case 32163: return launch_fp8_thin<32, 16, 3>(a, p, s);
        case 16086: return launch_fp8_thin<16, 8, 6>(a, p, s);
        case 16164: return launch_fp8_thin<16, 16, 4>(a, p, s);
        default: return -22;
    }
}
