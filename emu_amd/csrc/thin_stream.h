// The body of the bf16 few-row weight stream, thin_stream_kernel (gemv_thin.hip), as functions for its 13-bit packed twin
// (gemv_pack_thin.hip), whose flagged workgroups stream the bf16 rows and whose unflagged ones must end in the same bits.  The text
// is gemv_thin.hip's, statement for statement; that kernel keeps its own copy for now because building it from these functions changes
// its register allocation and schedule (same instructions, other order), which wants an A/B of its own before it replaces a kernel
// on the default path.  tests/test_gpu_bf16_pack_wide.py holds the two against each other on the bits.
//   thin_stream_loop    the LDS-DMA ring over K and the MFMAs of one workgroup (RN weight rows from n0, MR activation rows)
//   thin_stream_finish  the four waves' partial products summed through LDS, then the epilogue (bias, rounding points, RESID / SWIGLU ..)
// What the sum depends on is KCH alone (which k-steps a wave multiplies, in which order); RN, MR and the ring depth do not enter it.
#pragma once
#include "common.h"
#include "kernels.h"
#include "gemm_tile.h"

namespace emu_thin {

using namespace emu_gemm;

// LDS bytes of the ring / of the reduction that follows it in the same memory
template <int RN, int MR, int NSTG, int KCH>
constexpr int thin_ring_bytes() { return NSTG * (RN + MR) * KCH * 16; }
template <int RN>
constexpr int thin_red_bytes() { return 4 * (RN / 16) * 64 * 16; }

// KCH = 16-byte slots per row and stage: 32 (256 k, one DMA instruction = two rows) or 64 (512 k, one instruction = one row).
// On return every DMA of the ring has landed and every wave is past its last read of it.
template <int RN, int MR, int NSTG, int KCH>
__device__ __forceinline__ void thin_stream_loop(const GemvArgs& a, char* smem, const int n0, f32x4_t (&acc)[RN / 16]) {
    constexpr int KC = KCH * 8, ROWB = KCH * 16, RPI = 64 / KCH;          // k per stage, bytes per LDS row, rows per instruction
    constexpr int ROWS = RN + MR, ST = ROWS * ROWB, LPT = ROWS / (4 * RPI), RG = RN / 16, KSW = KCH / 16;   // k-steps per wave
    static_assert(ROWS % (4 * RPI) == 0, "every wave issues the same number of DMA instructions per stage");
    static_assert((NSTG - 2) * LPT <= 63, "vmcnt field is 6 bits");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;

    // DMA sources: instruction q = j * 4 + wave fills LDS rows q * RPI .. (lane / KCH selects), slot p = lane % KCH receives
    // global chunk p ^ (row & 15).  Rows [0, RN): weights (clamped at N - 1); [RN, ROWS): activations (clamped at M - 1).
    const bf16_t* src[LPT];
#pragma unroll
    for (int j = 0; j < LPT; ++j) {
        const int r = RPI * (j * 4 + wave) + lane / KCH;
        const int c = (lane % KCH) ^ (r & 15);
        const bf16_t* row;
        if (r < RN) { const int n = n0 + r; row = a.W + (size_t)(n < a.N ? n : a.N - 1) * a.ldw; }
        else { const int m = r - RN; row = a.x + (size_t)(m < a.M ? m : a.M - 1) * a.ldx; }
        src[j] = row + c * 8;
    }
    const int nk = a.K / KC;
    auto issue = [&](int kt, int stage) {
        kt = kt < nk ? kt : nk - 1;                    // past-the-end stages re-load the last one (uniform vmcnt counts)
        char* base = smem + stage * ST + wave * 1024;
#pragma unroll
        for (int j = 0; j < LPT; ++j) {
            if (RPI * (j * 4 + 3) + RPI - 1 < RN) glds16_nt(src[j] + kt * KC, base + j * 4096);      // weight rows only: stream
            else glds16(src[j] + kt * KC, base + j * 4096);
        }
    };
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) acc[rg] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const int rb = RN + (i < a.M ? i : a.M - 1);       // this lane's activation row (B operand column i)
#pragma unroll
    for (int t = 0; t < NSTG - 1; ++t) issue(t, t);
    for (int kt = 0; kt < nk; ++kt) {
        wait_vmcnt<(NSTG - 2) * LPT>();                // this wave's share of stage kt has landed
        __builtin_amdgcn_s_barrier();                  // ... and everyone's; everyone is done reading stage kt - 1
        issue(kt + NSTG - 1, (kt + NSTG - 1) % NSTG);
        const char* sb = smem + (kt % NSTG) * ST;
        bf16x8_t bf[KSW], af[KSW][RG];
#pragma unroll
        for (int s = 0; s < KSW; ++s) {
            const int c = (KSW * wave + s) * 4 + g;    // 16-byte chunk of this lane's 8 k values
            bf[s] = *reinterpret_cast<const bf16x8_t*>(sb + rb * ROWB + ((c ^ (rb & 15)) << 4));
#pragma unroll
            for (int rg = 0; rg < RG; ++rg)
                af[s][rg] = *reinterpret_cast<const bf16x8_t*>(sb + (rg * 16 + i) * ROWB + ((c ^ i) << 4));
        }
#pragma unroll
        for (int s = 0; s < KSW; ++s)
#pragma unroll
            for (int rg = 0; rg < RG; ++rg)
                acc[rg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[s][rg], bf[s], acc[rg], 0, 0, 0);
    }
    wait_vmcnt<0>();                                   // drain the tail DMA before the ring is reused
    __syncthreads();
}

// smem: thin_red_bytes<RN>() at least, free of readers (thin_stream_loop ends that way)
template <int EPI, int RN>
__device__ __forceinline__ void thin_stream_finish(const GemvArgs& a, char* smem, const int n0, const f32x4_t (&acc)[RN / 16]) {
    constexpr int RG = RN / 16;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;
    f32x4_t (*part)[RG][64] = reinterpret_cast<f32x4_t (*)[RG][64]>(smem);
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) part[wave][rg][lane] = acc[rg];
    __syncthreads();
    // wave w finishes row groups w, w + 4, ...: lane holds C[weight row 4g + r][activation row i], r = 0..3
    const int m = i;
    for (int rg = wave; rg < RG; rg += 4) {
        f32x4_t v = part[0][rg][lane];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const f32x4_t t = part[w][rg][lane];
            v[0] += t[0]; v[1] += t[1]; v[2] += t[2]; v[3] += t[3];
        }
        if (m >= a.M) continue;
        const int nb = n0 + 16 * rg + 4 * g;           // first of this lane's 4 output columns
        if constexpr (EPI == EPI_SWIGLU) {
#pragma unroll
            for (int r = 0; r < 4; r += 2) {
                const int n = nb + r;
                if (n + 1 < a.N) {
                    float gt = v[r], up = v[r + 1];
                    if (a.bias) { gt += bf2f(a.bias[n]); up += bf2f(a.bias[n + 1]); }
                    gt = bfround(gt); up = bfround(up);
                    a.out[(size_t)m * a.ldo + (n >> 1)] = f2bf(bfround(silu(gt)) * up);
                }
            }
        } else {
            float o[4];
            const bool full = nb + 3 < a.N;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = nb + r;
                float t = v[r];
                if (n < a.N) {
                    if (a.bias) t += bf2f(a.bias[n]);
                    t = bfround(t);
                    if constexpr (EPI == EPI_SILU) t = bfround(silu(t));
                    if constexpr (EPI == EPI_GELU) t = bfround(gelu_erf(t));
                    if constexpr (EPI == EPI_RESID) t = t + bf2f(a.res[(size_t)m * a.ldres + n]);
                }
                o[r] = t;
            }
            bf16_t* dst = a.out + (size_t)m * a.ldo + nb;
            if (full && ((reinterpret_cast<size_t>(dst) & 7) == 0)) {
                uint2 pk;
                pk.x = packbf(o[0], o[1]); pk.y = packbf(o[2], o[3]);
                *reinterpret_cast<uint2*>(dst) = pk;
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (nb + r < a.N) dst[r] = f2bf(o[r]);
            }
        }
    }
}

}  // namespace emu_thin
