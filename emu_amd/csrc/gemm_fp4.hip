// MXFP4 weights for 17 rows and more (beams x batch, contrastive search, prefill): a GEMM on the bf16 matrix cores, W4A16
//     out[m, n] = epilogue( sum_k x[m, k] * fp4(W4[n, k]) * 2^(S[n, k / 32] - 127) )
//
// gemv_fp4_thin.hip streams the 4-bit set for up to 16 rows: one 16-row activation tile, every converted weight fragment used by ONE
// MFMA.  This is the same arithmetic with a two-dimensional tile (format: emu_amd/mxfp4.py -- elements [N, K/2], element 2j in the
// low nibble; E8M0 scales [N, K/32]); what the two kernels share is defined once, in fp4_tile.h:
//   * K is walked in stages of 256, the last one partial when K % 256 != 0 (K % 32 == 0: the TAIL instantiations) (128 element bytes + 8 scale bytes per weight row, 512 bytes per activation row), NSTG stages
//     deep, counted vmcnt + one raw s_barrier per stage; element bytes, scale bytes and activation rows arrive by LDS-DMA, the DMA
//     source address carries the swizzle and the LDS image is lane-linear (fp4_tile.h: stage constants, w_src / x_src on the
//     source side, w_off / x_off on the read side): every ds_read_b128 of 16 rows x one block is conflict-free in every lane group;
//   * lane (i, g) of a wave owns ONE whole MX block per round -- row i, block 4 * ku + g of the stage, one 16-byte LDS read, one
//     scale byte -- and its four dwords become four A fragments through 4 x v_cvt_scalef32_pk_bf16_fp4 each (block scale applied
//     in the conversion; every dequantised value is exact in bf16: cvt8);
//   * the epilogue and its rounding points: store_c4 (bias, round to bf16, then residual or SiLU(gate) * up on
//     interleaved rows).
// What differs is the tile: a workgroup (4 waves, WN x WM) owns BN = 16 * A_ * WN weight rows x BM = 16 * B_ * WM activation rows;
// a wave owns A_ x 16 weight rows x B_ x 16 activation rows and walks the whole stage itself (no k split, no reduction through
// LDS).  A converted fragment feeds B_ MFMAs, so the 16 conversions of a block sit behind 4 * B_ matrix instructions.
//   form        A_ B_ WN WM   BN x BM    stage             ring   LDS        rows
//   narrow       1  2  4  1   64 x 32    8 + 16 + 0.5 KiB    3    73.5 KiB   17..32   (two workgroups per CU)
//   one tile     1  4  4  1   64 x 64    8 + 32 + 0.5 KiB    3    121.5 KiB  33..64
//   prefill      2  4  2  2   64 x 128   8 + 64 + 0.5 KiB    2    145 KiB    65 and up (grid.x walks the row tiles, so the
//                                                                             workgroups in flight share weight rows in L2)
// The first two are bound by the weight stream (use-once bytes: nt loads); the third re-reads the 4-bit bytes once per row tile
// from L2 / the Infinity Cache.  Ragged M and N: rows and columns are clamped on load and masked on store.
// No fused RMSNorm, no RoPE epilogue, no K-slicing.  The result is what the bf16 GEMM computes on the dequantised weights, up to
// fp32 summation order.
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "fp4_tile.h"

using namespace emu_gemm;

namespace {

// TAIL: K % 256 != 0 (K % 32 == 0, K >= 256): one more stage with kb = (K % 256) / 32 valid MX blocks, peeled off the k loop as in
// gemv_fp4_thin.hip, with the same two halves from fp4_tile.h (source clamp, read mask); a dead k half (ku = 1, kb <= 4) is skipped.
template <int EPI, int A_, int B_, int WN, int WM, int NSTG, bool STREAM, bool TAIL>
__global__ __launch_bounds__(256) void fp4_gemm_kernel(const GemvArgs a) {
    static_assert(WN * WM == 4, "four waves");
    constexpr int BN = 16 * A_ * WN, BM = 16 * B_ * WM;
    static_assert(BN == 64, "two 32-row scale instructions per stage");
    constexpr int WI = BN / 8, XI = BM / 2, TOT = WI + XI;                 // 1 KiB DMA instructions per stage: weights, activations
    static_assert(WI % 4 == 0 && TOT % 4 == 0, "every wave issues the same instructions: WI / 4 of weights, then activations");
    constexpr int JN = TOT / 4, L = JN + 1;                                // + the wave's scale instruction
    static_assert((NSTG - 2) * L <= 63, "vmcnt field is 6 bits");
    constexpr int WB = BN * WROW, XB = BM * XROW, ST = WB + XB + BN * SROW;   // stage = weight rows | activation rows | scale rows
    __shared__ __attribute__((aligned(16))) char smem[NSTG * ST];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int wn = wave % WN, wm = wave / WN;
    const int m0 = (STREAM ? 0 : blockIdx.x) * BM, n0 = (STREAM ? blockIdx.x : blockIdx.y) * BN;

    // DMA sources (fp4_tile.h): instruction q < WI fills weight rows 8q .. 8q + 7 of the tile, q >= WI activation rows 2(q - WI), + 1
    const int nk = TAIL ? a.K / KC + 1 : a.K / KC;
    const int kb = TAIL ? (a.K % KC) / 32 : SROW;      // valid MX blocks of the last stage
    const char* src[JN];
    static_assert(JN <= 32, "one bit per instruction");
    uint32_t past = 0;                                 // TAIL: bit j = in the last stage, the source of instruction j lies at or past K
#pragma unroll
    for (int j = 0; j < JN; ++j) {
        const int q = j * 4 + wave;
        src[j] = j < WI / 4 ? w_src(a, n0, q, lane) : x_src(a, m0, x_dma_row(q - WI, lane), lane);
        if constexpr (TAIL)
            past |= ((j < WI / 4 ? w_src_past(q, lane, kb) : x_src_past(x_dma_row(q - WI, lane), lane, kb)) ? 1u : 0u) << j;
    }
    // scale rows: one 4-byte instruction = 32 rows x 8 bytes; waves w and w + 2 fill the same half with the same bytes
    const char* ssrc;
    {
        const int n = n0 + (wave & 1) * 32 + (lane >> 1);
        ssrc = reinterpret_cast<const char*>(a.w4scale) + (size_t)(n < a.N ? n : a.N - 1) * a.lds + (lane & 1) * 4;
    }
    auto issue = [&](int kt, int stage) {
        kt = kt < nk ? kt : nk - 1;                    // past-the-end stages re-load the last one (uniform vmcnt counts)
        const bool last = TAIL && kt == nk - 1;        // (nk >= 2 then: the stage before exists)
        char* base = smem + stage * ST;
#pragma unroll
        for (int j = 0; j < JN; ++j) {
            const int q = j * 4 + wave;
            int kj = kt;
            if constexpr (TAIL) kj -= last && ((past >> j) & 1u) ? 1 : 0;
            if (j < WI / 4) {
                if constexpr (STREAM) glds16_nt(src[j] + kj * WROW, base + q * 1024);
                else glds16(src[j] + kj * WROW, base + q * 1024);
            } else
                glds16(src[j] + kj * XROW, base + q * 1024);
        }
        glds4<false>(ssrc + kt * SROW, base + WB + XB + (wave & 1) * 256);
    };
    f32x4_t acc[A_][B_];
#pragma unroll
    for (int ai = 0; ai < A_; ++ai)
#pragma unroll
        for (int bi = 0; bi < B_; ++bi) acc[ai][bi] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NSTG - 1; ++t) issue(t, t);
    // one stage of the k loop; LAST: the partial stage of a TAIL kernel
    auto round = [&](int kt, auto last_stage) {
        constexpr bool LAST = decltype(last_stage)::value;
        wait_vmcnt<(NSTG - 2) * L>();                  // this wave's share of stage kt has landed
        __builtin_amdgcn_s_barrier();                  // ... and everyone's; everyone is done reading stage kt - 1
        issue(kt + NSTG - 1, (kt + NSTG - 1) % NSTG);
        const char* sb = smem + (kt % NSTG) * ST;
#pragma unroll
        for (int ku = 0; ku < 2; ++ku) {
            if (LAST && 4 * ku >= kb) break;
            const int blk = ku * 4 + g;                // this lane's MX block of the stage
            u32x4 wv[A_];
            float sc[A_];
#pragma unroll
            for (int ai = 0; ai < A_; ++ai) {
                const int wr = (wn * A_ + ai) * 16 + i;
                wv[ai] = *reinterpret_cast<const u32x4*>(sb + w_off(wr, blk));
                sc[ai] = scale_operand(*reinterpret_cast<const uint8_t*>(sb + WB + XB + wr * SROW + blk));
                if constexpr (LAST) tail_mask_w(blk < kb, wv[ai], sc[ai]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                bf16x8_t bf[B_];
#pragma unroll
                for (int bi = 0; bi < B_; ++bi) {
                    bf[bi] = *reinterpret_cast<const bf16x8_t*>(sb + WB + x_off((wm * B_ + bi) * 16 + i, 4 * blk + q));
                    if constexpr (LAST) bf[bi] = tail_mask_x(blk < kb, bf[bi]);
                }
#pragma unroll
                for (int ai = 0; ai < A_; ++ai) {
                    const bf16x8_t af = cvt8(wv[ai][q], sc[ai]);
#pragma unroll
                    for (int bi = 0; bi < B_; ++bi) acc[ai][bi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf[bi], acc[ai][bi], 0, 0, 0);
                }
            }
        }
    };
    const int nfull = TAIL ? nk - 1 : nk;
    for (int kt = 0; kt < nfull; ++kt) round(kt, std::false_type{});
    if constexpr (TAIL) round(nfull, std::true_type{});
    wait_vmcnt<0>();                                   // the tail DMA lands before the workgroup's LDS is handed on
    // lane holds C[weight row 4g + r][activation row i] of every (ai, bi) sub-tile, r = 0..3
#pragma unroll
    for (int bi = 0; bi < B_; ++bi) {
        const int m = m0 + (wm * B_ + bi) * 16 + i;
        if (m >= a.M) continue;
#pragma unroll
        for (int ai = 0; ai < A_; ++ai)
            store_c4<EPI>(a, m, n0 + (wn * A_ + ai) * 16 + 4 * g, acc[ai][bi]);   // nb = first of this lane's 4 output columns
    }
}

template <int A_, int B_, int WN, int WM, int NSTG, bool STREAM, bool TAIL>
int launch_fp4_gemm(const GemvArgs& a, hipStream_t s) {
    constexpr int BN = 16 * A_ * WN, BM = 16 * B_ * WM;
    const int nt = (a.N + BN - 1) / BN, mt = (a.M + BM - 1) / BM;
    if (!STREAM && nt > 65535) return -22;
    const dim3 grid = STREAM ? dim3(nt) : dim3(mt, nt), block(256);
#define EMU_F4G_CASE(E) case E: hipLaunchKernelGGL((fp4_gemm_kernel<E, A_, B_, WN, WM, NSTG, STREAM, TAIL>), grid, block, 0, s, a); break;
    switch (a.epi) {
        EMU_F4G_CASE(EPI_NONE)
        EMU_F4G_CASE(EPI_RESID)
        EMU_F4G_CASE(EPI_SWIGLU)
        default: return -22;
    }
#undef EMU_F4G_CASE
    EMU_CHECK_LAUNCH();
    return 0;
}

}  // namespace

// The same tiles whether or not K ends in a partial stage (a K of whole stages runs the kernels without it).
template <bool TAIL>
static int dispatch_fp4_gemm(const GemvArgs& a, hipStream_t s) {
    if (a.M <= 32) return launch_fp4_gemm<1, 2, 4, 1, 3, true, TAIL>(a, s);
    if (a.M <= 64) return launch_fp4_gemm<1, 4, 4, 1, 3, true, TAIL>(a, s);
    return launch_fp4_gemm<2, 4, 2, 2, 2, false, TAIL>(a, s);
}
int launch_gemm_fp4(const GemvArgs& a, hipStream_t s) {
    if (!fp4_mfma_ok(a)) return -22;
    return a.K % KC ? dispatch_fp4_gemm<true>(a, s) : dispatch_fp4_gemm<false>(a, s);
}
