// MXFP4 weight stream for few-row steps (3..16 rows: beam search, small batches, contrastive search) on the matrix cores:
//     out[m, n] = epilogue( sum_k x[m, k] * fp4(W4[n, k]) * 2^(S[n, k / 32] - 127) )
//
// gemv_fp4.hip decodes and multiplies on the VALU and cannot hold more than two rows of accumulators; gemv_thin.hip already streams
// bf16 weights for these row counts through LDS-DMA stages into v_mfma_f32_16x16x32_bf16 with no VALU in the loop.  This is that
// structure fed from 4-bit bytes (format: emu_amd/mxfp4.py -- elements [N, K/2], element 2j in the low nibble; E8M0 scales [N, K/32]):
//   * a workgroup (4 waves) owns RN = 16 / 32 weight rows and walks K in stages of 256, the last one partial when K % 256 != 0
//     (K % 32 == 0: the TAIL instantiations) (128 element bytes + 8 scale bytes per
//     weight row, 512 bytes per activation row), NSTG stages deep, counted vmcnt + one raw s_barrier per stage;
//   * element bytes and activations arrive by 16-byte LDS-DMA (one instruction = 8 weight rows or 2 activation rows); the DMA source
//     address carries the swizzle, the LDS image is lane-linear.  The stage geometry, both swizzles (source side and read side)
//     and the conversion are fp4_tile.h's, shared with gemm_fp4.hip;
//   * the k order inside an MFMA is free as long as A and B agree: lane (i, g) of a wave takes ONE whole MX block -- row i, block
//     4 * ku + g of the stage, one 16-byte LDS read, one scale byte -- and spends its four dwords on four MFMAs; dword q becomes the
//     A fragment through 4 x v_cvt_scalef32_pk_bf16_fp4 (one byte -> two bf16, the block scale applied in the conversion; every
//     dequantised value is exact in bf16), and the B lane reads the matching 8 k of activation row i: 16-byte chunk 4 * block + q;
//   * a unit of work is (16-row group, k half of the stage): RN / 8 units on 4 waves.  Wave u streams the scale bytes of ITS unit
//     itself: 16 rows x 4 contiguous bytes by one 4-byte DMA into a region of its own (lanes 16..63 repeat lanes 0..15);
//   * the two k-half partials of a row group meet in LDS at the end; the epilogue is store_c4 (fp4_tile.h: bias, round to bf16,
//     then residual or SiLU(gate) * up -- thin_stream_kernel's rounding points), the one the 4-bit GEMM uses.  No fused RMSNorm:
//     callers normalise first.
// Algorithmic bytes per call = N * (K/2 + K/32).  Activations add MR * 512 / (RN * 136) of that as L2 -> LDS traffic.
// Which tile, which grid, which arguments are acceptable: gemv.hip::gemv_thin_plan (weight kind MXFP4, family GEMV_FAM_FP4_THIN), the
// one host planner of the three few-row matrix-core streams; launch_gemv_fp4_thin below is only the switch from its answer (and
// K % 256: TAIL) to template arguments, and callers come through gemv.hip::launch_gemv_thin_stream.
//
// Conversion semantics on the device (pinned by tests/test_gpu_fp4_wide.py::test_decode_exhaustive_mfma): low nibble -> element 0;
// the scale operand contributes 2^(its exponent field - 127).  With scale bytes 1 and 2 some products lie below 2^-126 (bf16
// denormals): neither the conversion nor the MFMA flushes them on MI355X (test_decode_denormal_products: all exact).
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "fp4_tile.h"

using namespace emu_gemm;

namespace {

// TAIL: K % 256 != 0 (K % 32 == 0, K >= 256): one more stage with kb = (K % 256) / 32 valid MX blocks, peeled off the k loop, so
// the instantiations for whole stages keep theirs.  fp4_tile.h has the two halves of it: lanes whose block / chunk lies at or past
// K fetch the stage before (w_src_past / x_src_past; scale rows are padded to whole stages, fp4_scale_stride), and the read side
// multiplies nothing for a dead block (tail_mask_w / tail_mask_x).  A unit whose k half is dead altogether (ku = 1, kb <= 4) sits
// the stage out; it still issues and waits like everyone.
template <int EPI, int RN, int MR, int NSTG, bool TAIL>
__global__ __launch_bounds__(256) void fp4_thin_kernel(const GemvArgs a) {
    constexpr int WI = RN / 8, XI = MR / 2, TOT = WI + XI, JMAX = (TOT + 3) / 4;   // 1 KiB DMA instructions per stage: weights, activations
    constexpr int WB = RN * WROW, XB = MR * XROW, ST = WB + XB + 4 * 256;  // stage = weight rows | activation rows | 4 scale regions
    constexpr int RG = RN / 16, UNITS = 2 * RG;
    static_assert(UNITS <= 4, "one unit per wave");
    // DMA instructions per stage of a wave: instructions q = wave, wave + 4, .. < TOT, plus its scale instruction
    constexpr int L_HI = JMAX + 1, L_LO = TOT / 4 + 1;
    static_assert((NSTG - 2) * L_HI <= 63, "vmcnt field is 6 bits");
    constexpr int RED = UNITS * 64 * 16;
    __shared__ __attribute__((aligned(16))) char smem[NSTG * ST > RED ? NSTG * ST : RED];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * RN;
    const int unit = wave % UNITS, rg = unit >> 1, ku = unit & 1;         // waves >= UNITS stage only (their unit is a repeat)

    // DMA sources (fp4_tile.h): instruction q < WI fills weight rows 8q .. 8q + 7, q >= WI activation rows 2(q - WI), + 1
    const int nk = TAIL ? a.K / KC + 1 : a.K / KC;
    const int kb = TAIL ? (a.K % KC) / 32 : SROW;      // valid MX blocks of the last stage
    const char* src[JMAX];
    uint32_t past = 0;                                 // TAIL: bit j = in the last stage, the source of instruction j lies at or past K
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
        const int q = j * 4 + wave;
        if (q < WI) {
            src[j] = w_src(a, n0, q, lane);
            if constexpr (TAIL) past |= (w_src_past(q, lane, kb) ? 1u : 0u) << j;
        } else {
            const int r = x_dma_row(q - WI, lane), rr = r < MR ? r : MR - 1;   // (q >= TOT: never issued)
            src[j] = x_src(a, 0, rr, lane);
            if constexpr (TAIL) past |= (x_src_past(rr, lane, kb) ? 1u : 0u) << j;
        }
    }
    const char* ssrc;
    {
        const int n = n0 + rg * 16 + i;
        ssrc = reinterpret_cast<const char*>(a.w4scale) + (size_t)(n < a.N ? n : a.N - 1) * a.lds + ku * 4;
    }
    auto issue = [&](int kt, int stage) {
        kt = kt < nk ? kt : nk - 1;                    // past-the-end stages re-load the last one (uniform vmcnt counts)
        const bool last = TAIL && kt == nk - 1;        // (nk >= 2 then: the stage before exists)
        char* base = smem + stage * ST;
#pragma unroll
        for (int j = 0; j < JMAX; ++j) {
            const int q = j * 4 + wave;
            if (j * 4 + 3 < TOT || q < TOT) {
                int kj = kt;
                if constexpr (TAIL) kj -= last && ((past >> j) & 1u) ? 1 : 0;
                if (q < WI) glds16_nt(src[j] + kj * WROW, base + q * 1024);            // weight rows: stream
                else glds16(src[j] + kj * XROW, base + q * 1024);
            }
        }
        glds4<true>(ssrc + kt * SROW, base + WB + XB + wave * 256);
    };
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    const int rb = i < a.M ? i : a.M - 1;              // this lane's activation row (B operand column i)
    const int blk = ku * 4 + g;                        // this lane's MX block of the stage
    const int wr = rg * 16 + i;                        // this lane's weight row (A operand row i)
    const int woff = w_off(wr, blk);
    const int soff = WB + XB + wave * 256 + i * 4;
#pragma unroll
    for (int t = 0; t < NSTG - 1; ++t) issue(t, t);
    // one stage of the k loop; LAST: the partial stage of a TAIL kernel
    auto round = [&](int kt, auto last_stage) {
        constexpr bool LAST = decltype(last_stage)::value;
        // this wave's share of stage kt has landed
        if (TOT % 4 == 0 || wave < TOT % 4) wait_vmcnt<(NSTG - 2) * L_HI>();
        else wait_vmcnt<(NSTG - 2) * L_LO>();
        __builtin_amdgcn_s_barrier();                  // ... and everyone's; everyone is done reading stage kt - 1
        issue(kt + NSTG - 1, (kt + NSTG - 1) % NSTG);
        if (wave < UNITS && (!LAST || 4 * ku < kb)) {
            const char* sb = smem + (kt % NSTG) * ST;
            u32x4 wv = *reinterpret_cast<const u32x4*>(sb + woff);
            const uint32_t sd = *reinterpret_cast<const uint32_t*>(sb + soff);
            float sc = scale_operand((sd >> (8 * g)) & 0xffu);
            if constexpr (LAST) tail_mask_w(blk < kb, wv, sc);
            bf16x8_t bf[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                bf[q] = *reinterpret_cast<const bf16x8_t*>(sb + WB + x_off(rb, 4 * blk + q));
                if constexpr (LAST) bf[q] = tail_mask_x(blk < kb, bf[q]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cvt8(wv[q], sc), bf[q], acc, 0, 0, 0);
        }
    };
    const int nfull = TAIL ? nk - 1 : nk;
    for (int kt = 0; kt < nfull; ++kt) round(kt, std::false_type{});
    if constexpr (TAIL) round(nfull, std::true_type{});
    wait_vmcnt<0>();                                   // drain the tail DMA before the ring is reused
    __syncthreads();
    f32x4_t (*part)[64] = reinterpret_cast<f32x4_t (*)[64]>(smem);
    if (wave < UNITS) part[unit][lane] = acc;
    __syncthreads();
    // wave w finishes row group w: lane holds C[weight row 4g + r][activation row i], r = 0..3
    if (wave >= RG) return;
    const int m = i;
    f32x4_t v = part[2 * wave][lane];
    {
        const f32x4_t t = part[2 * wave + 1][lane];
        v[0] += t[0]; v[1] += t[1]; v[2] += t[2]; v[3] += t[3];
    }
    if (m >= a.M) return;
    const int nb = n0 + 16 * wave + 4 * g;             // first of this lane's 4 output columns
    store_c4<EPI>(a, m, nb, v);
}

template <int RN, int MR, int NSTG, bool TAIL>
int launch_fp4_thin(const GemvArgs& a, const GemvPlan& p, hipStream_t s) {
#define EMU_F4T_CASE(E) case E: hipLaunchKernelGGL((fp4_thin_kernel<E, RN, MR, NSTG, TAIL>), dim3(p.grid), dim3(p.block), 0, s, a); break;
    EMU_EPI3(EMU_F4T_CASE)
#undef EMU_F4T_CASE
}

}  // namespace

// the built (weight rows, activation rows, ring depth) combinations, each with and without the partial last stage (TAIL: K % 256 != 0);
// gemv.hip::gemv_thin_plan picks among them
int launch_gemv_fp4_thin(const GemvArgs& a, const GemvPlan& p, hipStream_t s) {
#define EMU_F4T_TILE(RN, MR, NSTG) return a.K % KC ? launch_fp4_thin<RN, MR, NSTG, true>(a, p, s) : launch_fp4_thin<RN, MR, NSTG, false>(a, p, s);
    switch ((p.rows * 100 + p.mb) * 10 + p.stages) {   // digits: rows, mb (two), stages
        case 32085: EMU_F4T_TILE(32, 8, 5)
        case 16086: EMU_F4T_TILE(16, 8, 6)
        case 32164: EMU_F4T_TILE(32, 16, 4)
        case 16164: EMU_F4T_TILE(16, 16, 4)
        default: return -22;
    }
#undef EMU_F4T_TILE
}
