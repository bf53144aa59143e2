// Decode-shape (M <= 16 rows) weight streams:  out[m, n] = epilogue( sum_k xeff[m, k] * W[n, k] )
//
// HBM-bound: every weight byte is read exactly once per call (PMC: traffic / algorithmic = 1.0013) with non-temporal
// loads; the activations (a few KB) come from L1/L2.  launch_gemv() is three steps: the shape of the argument block (gemv_shape_of:
// integers and flags), gemv_plan() -- the one place that decides the kernel family, its form, rows per workgroup, waves, trips, grid
// -- and launch_planned(), which maps the plan's values to template arguments.  The planner is pure host arithmetic (no HIP call,
// no global; the emu_gemm_tune mask is an argument), exported as emu_gemv_plan and held against recorded launches by
// tests/test_gemv_plan.py; emu_gemv_geometry / emu_gemv_partition are views of the same plan.  gemv_thin_plan() is the part of it
// that plans the three matrix-core few-row streams (bf16, fp8, MXFP4), exported as emu_gemv_thin_plan (tests/test_thin_plan.py);
// gemv_plan asks it for bf16 from 4 rows on, launch_gemv_thin_stream() launches whatever it answers.  The families:
//   block (gemv_kernel)      1..8 rows.  One 256-thread workgroup owns R (16/8/4/2) consecutive weight rows and splits K across its
//                    4 waves (thread t owns 16-byte vectors t, t+256, ...), N/R workgroups >> 256 CUs.  Inner product on
//                    v_dot2c_f32_bf16 (weights consumed unpacked), wave reductions on DPP.  Optional fused prologue: LLaMA
//                    RMSNorm of x (fp32 variance, the reference's bf16 rounding points: xeff = bf16(g * bf16(x * rinv))).
//                    Fused epilogues: bias, residual add, SwiGLU over interleaved (gate, up) row pairs, SiLU, GELU.
//                    One row runs in one of three forms (GemvForm): head, preload, rolling loop.
//   single round trip (gemv_rt_kernel)   M = 1, all loads of a workgroup issued up front: down_proj, small shards; bf16 or fp8.
//   wave (gemv_wave_kernel)  M = 1, K <= 2560: one wave per 4 whole rows, no LDS / barrier (TP-shard o_proj / down_proj).
//   register-fed MFMA (gemv_mfma_kernel)   9..16 rows on v_mfma_f32_16x16x32_bf16 where the thin stream does not apply.
//   thin stream (gemv_thin.hip)            4..16 rows, K in whole 256-wide stages: LDS-DMA stages + MFMA.
//   fp8 block (gemv_fp8_kernel)            optional e4m3 weight stream (per-row scale), 1..2 rows, 8- or 16-byte weight loads.
//   MXFP4 rows (gemv_fp4.hip)              optional MXFP4 weight stream (4-bit elements, one E8M0 scale per 32), M <= 2.
//   fp8 thin (gemv_fp8_thin.hip), MXFP4 thin (gemv_fp4_thin.hip)   the thin stream fed from e4m3 / 4-bit bytes, 1..16 rows; reached
//                    through launch_gemv_thin_stream only (the engine's 3..16-row steps), never through gemv_plan.
//
// Replaces (reference call sites): LlamaDecoderLayer linears + RMSNorm reached from Emu2/emu/emu.py:133-138
// and :213-229 at S=1 (greedy: 1 row; beam search: num_beams rows), project_up/project_down emu.py:131,147.
// Algorithmic bytes per call = 2*N*K (fp8: N*K).
#include "common.h"
#include <type_traits>
#include "kernels.h"

namespace {

// PRE > 0: all (<= PRE) 16-byte weight chunks of this thread are requested BEFORE the RMSNorm prologue, so the HBM
// stream is already in flight while the block computes mean(x^2); requires K/8 <= 256*PRE.  PRE == 0: generic loop.
template <int R, int MB, bool NORM, int EPI, int PRE>
__global__ __launch_bounds__(256) void gemv_kernel(const GemvArgs a) {
    __shared__ float red[4][R * MB];
    __shared__ float fin[R * MB];
    __shared__ float scratch[4];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int KV = a.K >> 3;                       // 16-byte vectors per row
    const int n0 = blockIdx.x * R;

    const bf16_t* wrow[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int n = n0 + r;
        n = n < a.N ? n : a.N - 1;                 // tail rows: clamp loads, mask stores
        wrow[r] = a.W + (size_t)n * a.ldw;
    }
    // PRE path (MB == 1): x first (L2 hits, returned first because loads complete in order), then the whole weight
    // slice of this thread, so HBM is streaming while the RMSNorm statistics are reduced.
    u32x4 pre[PRE > 0 ? PRE : 1][R];
    u32x4 xr[PRE > 0 ? PRE : 1];
    if constexpr (PRE > 0) {
        static_assert(PRE == 0 || MB == 1, "preload form is for the single-row decode case");
#pragma unroll
        for (int c = 0; c < PRE; ++c) {
            const int vi = tid + 256 * c;
            const u32x4 z = {0u, 0u, 0u, 0u};
            xr[c] = vi < KV ? ld16(a.x + vi * 8) : z;
        }
#pragma unroll
        for (int c = 0; c < PRE; ++c) {
            const int vi = tid + 256 * c;
            const int vc = vi < KV ? vi : KV - 1;  // clamped: x is zero there, so the product vanishes
#pragma unroll
            for (int r = 0; r < R; ++r) pre[c][r] = ld_stream(reinterpret_cast<const u32x4*>(wrow[r] + vc * 8));
        }
    }

    float rinv[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) rinv[m] = 1.f;
    // PRE < 0 ("head" form, MB == 1, fused norm, K <= 8192): the activation vector and the gain (<= 4 chunks per thread
    // each, L2 hits, returned first because loads complete in order) and the first trip of the weight stream are requested
    // before the RMSNorm statistics are reduced, and the reduction goes through a raw s_barrier (a __syncthreads drains
    // vmcnt, i.e. waits for the weights): HBM streams during the prologue instead of after it.  The normalised activations
    // are packed once into registers, so the remaining trips issue nothing but weight loads.
    u32x4 hx[4], hg[4];
    u32x4 hw[R];
    if constexpr (PRE < 0) {
        static_assert(PRE >= 0 || (MB == 1 && NORM), "head form: single row with the fused norm");
        __shared__ float ssp[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int vi = tid + 256 * c;
            const int vc = vi < KV ? vi : KV - 1;
            hx[c] = vi < KV ? ld16(a.x + vi * 8) : u32x4{0u, 0u, 0u, 0u};
            hg[c] = ld16(a.norm_w + vc * 8);
        }
#pragma unroll
        for (int r = 0; r < R; ++r)                                    // short rows (K < 2048): clamped, against a zero operand
            hw[r] = ld_stream(reinterpret_cast<const u32x4*>(wrow[r] + (tid < KV ? tid : KV - 1) * 8));
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float f[8];
            unpack8(hx[c], f);
#pragma unroll
            for (int j = 0; j < 8; ++j) ss += f[j] * f[j];
        }
        ss = wave_sum(ss);
        if (lane == 0) *reinterpret_cast<volatile float*>(&ssp[wave]) = ss;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const volatile float* sp = ssp;
        rinv[0] = rsqrtf((sp[0] + sp[1] + sp[2] + sp[3]) / (float)a.K + a.eps);
#pragma unroll
        for (int c = 0; c < 4; ++c) {                                  // hx <- bf16(g * bf16(x * rinv)), the dot2 operand
            float xf[8], g[8];
            unpack8(hx[c], xf);
            unpack8(hg[c], g);
#pragma unroll
            for (int j = 0; j < 8; ++j) xf[j] = g[j] * bfround(xf[j] * rinv[0]);
            hx[c] = pack8(xf);
        }
    } else
    if constexpr (NORM) {
        float ss[MB];
#pragma unroll
        for (int m = 0; m < MB; ++m) ss[m] = 0.f;
        if constexpr (PRE > 0) {
#pragma unroll
            for (int c = 0; c < PRE; ++c) {
                float f[8];
                unpack8(xr[c], f);
#pragma unroll
                for (int j = 0; j < 8; ++j) ss[0] += f[j] * f[j];
            }
        } else
        for (int vi = tid; vi < KV; vi += 256) {
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                if (m < a.M) {
                    float f[8];
                    unpack8(ld16(a.x + (size_t)m * a.ldx + vi * 8), f);
#pragma unroll
                    for (int j = 0; j < 8; ++j) ss[m] += f[j] * f[j];
                }
            }
        }
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            const float t = block_sum<4>(ss[m], scratch);
            rinv[m] = rsqrtf(t / (float)a.K + a.eps);
        }
    }

    float acc[R][MB];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int m = 0; m < MB; ++m) acc[r][m] = 0.f;

    // The inner product runs on v_dot2c_f32_bf16: weights are consumed as they arrive (no unpack) against the activation
    // vector re-packed to bf16 pairs once per 16-byte column group -- exact, because the reference rounds the normalised
    // activations to bf16 anyway.  4 VALU ops per 8 weights instead of 16 (unpack + fma).
    auto consume = [&](int vi, const u32x4 (&wv)[R], const u32x4* xpre) {
        float g[8];
        if constexpr (NORM) unpack8(ld16(a.norm_w + vi * 8), g);
        u32x4 xp[MB];
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            if (m < a.M) {
                xp[m] = xpre ? *xpre : ld16(a.x + (size_t)m * a.ldx + vi * 8);
                if constexpr (NORM) {
                    float xf[8];
                    unpack8(xp[m], xf);
#pragma unroll
                    for (int j = 0; j < 8; ++j) xf[j] = g[j] * bfround(xf[j] * rinv[m]);
                    xp[m] = pack8(xf);                               // the pack is the reference's second rounding
                }
            } else {
                xp[m] = u32x4{0u, 0u, 0u, 0u};
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                float t = acc[r][m];
                t = bf16_dot2(wv[r].x, xp[m].x, t);
                t = bf16_dot2(wv[r].y, xp[m].y, t);
                t = bf16_dot2(wv[r].z, xp[m].z, t);
                t = bf16_dot2(wv[r].w, xp[m].w, t);
                acc[r][m] = t;
            }
        }
    };

    uint32_t warm = 0;                                                 // destination of the successor touches (l2_warm.h): live to the end
    if constexpr (PRE < 0) {
        auto dots = [&](const u32x4 (&wv)[R], const u32x4& xp) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float t = acc[r][0];
                t = bf16_dot2(wv[r].x, xp.x, t);
                t = bf16_dot2(wv[r].y, xp.y, t);
                t = bf16_dot2(wv[r].z, xp.z, t);
                t = bf16_dot2(wv[r].w, xp.w, t);
                acc[r][0] = t;
            }
        };
        // trip 0 from the head registers; trips 1..3 stream behind it through two register sets (two trips in flight)
        u32x4 w1[R];
        auto fetch = [&](u32x4 (&wv)[R], int c) {
            const int vi = tid + 256 * c;
            if (vi < KV) {
#pragma unroll
                for (int r = 0; r < R; ++r) wv[r] = ld_stream(reinterpret_cast<const u32x4*>(wrow[r] + vi * 8));
            }
        };
        fetch(w1, 1);
        dots(hw, hx[0]);
        __builtin_amdgcn_sched_barrier(0);                             // a third register set would cost a wave of occupancy
        fetch(hw, 2);
        if (tid + 256 < KV) dots(w1, hx[1]);
        __builtin_amdgcn_sched_barrier(0);
        fetch(w1, 3);
        warm = warm_touch(a.warm, blockIdx.x, tid);                    // behind this workgroup's last weight load
        if (tid + 512 < KV) dots(hw, hx[2]);
        if (tid + 768 < KV) dots(w1, hx[3]);
    } else if constexpr (PRE > 0) {
        warm = warm_touch(a.warm, blockIdx.x, tid);                    // every weight load was issued in the prologue
#pragma unroll
        for (int c = 0; c < PRE; ++c) {
            const int vi = tid + 256 * c;
            if (vi < KV) consume(vi, pre[c], &xr[c]);
        }
    } else {
#pragma unroll 2
        for (int vi = tid; vi < KV; vi += 256) {
            u32x4 wv[R];
#pragma unroll
            for (int r = 0; r < R; ++r) wv[r] = ld_stream(reinterpret_cast<const u32x4*>(wrow[r] + vi * 8));
            consume(vi, wv, nullptr);
        }
    }

#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            const float v = wave_sum(acc[r][m]);
            if (lane == 0) red[wave][r * MB + m] = v;
        }
    __syncthreads();
    if (tid < R * MB) fin[tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    __syncthreads();

    if constexpr (EPI == EPI_SWIGLU) {
        // rows (2j, 2j+1) = (gate_j, up_j); out[m, n0/2 + j] = bf16(bf16(silu(gate)) * up)
        if (tid < (R / 2) * MB) {
            const int j = tid / MB, m = tid % MB;
            const int n = n0 + 2 * j;
            if (m < a.M && n + 1 < a.N) {
                const float gt = bfround(fin[(2 * j) * MB + m] + (a.bias ? bf2f(a.bias[n]) : 0.f));
                const float up = bfround(fin[(2 * j + 1) * MB + m] + (a.bias ? bf2f(a.bias[n + 1]) : 0.f));
                const float act = bfround(silu(gt));
                a.out[(size_t)m * a.ldo + (n >> 1)] = f2bf(act * up);
            }
        }
    } else {
        if (tid < R * MB) {
            const int r = tid / MB, m = tid % MB;
            const int n = n0 + r;
            if (m < a.M && n < a.N) {
                float v = fin[tid];
                if (a.bias) v += bf2f(a.bias[n]);
                v = bfround(v);
                if constexpr (EPI == EPI_SILU) v = bfround(silu(v));
                if constexpr (EPI == EPI_GELU) v = bfround(gelu_erf(v));
                if constexpr (EPI == EPI_RESID) v = v + bf2f(a.res[(size_t)m * a.ldres + n]);
                a.out[(size_t)m * a.ldo + n] = f2bf(v);
            }
        }
    }
    if constexpr (PRE != 0) asm volatile("" :: "v"(warm));
}

// Single-round-trip GEMV (decode, M = 1): every load of the block -- x, gain, and the block's WHOLE weight slice
// (R rows x KIT 256-lane trips, fully unrolled into registers) -- is issued before anything waits, so a block pays one
// HBM latency instead of one per loop trip plus one for the RMSNorm prologue.  The prologue's cross-wave reduction uses
// a raw s_barrier (a __syncthreads would drain vmcnt and serialise the weight loads behind it).  FP8: 8-byte loads of
// e4m3 weights with a per-row fp32 scale.  KIT = ceil(K / 8 / 256) rounded up to a built value.
template <int R, int KIT, bool NORM, int EPI, bool FP8>
__global__ __launch_bounds__(256) void gemv_rt_kernel(const GemvArgs a) {
    using WT = typename std::conditional<FP8, u32x2, u32x4>::type;
    __shared__ float red[4][R];
    __shared__ float fin[R];
    __shared__ float ssp[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int KV = a.K >> 3;
    const int n0 = blockIdx.x * R;
    constexpr int WB = FP8 ? 1 : 2;                                   // bytes per weight
    const unsigned char* W8 = reinterpret_cast<const unsigned char*>(a.W);

    u32x4 xv[KIT], gv[KIT];
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
        const int vi = tid + 256 * it;
        xv[it] = u32x4{0u, 0u, 0u, 0u};
        gv[it] = u32x4{0u, 0u, 0u, 0u};
        if (vi < KV) {
            xv[it] = ld16(a.x + vi * 8);
            if constexpr (NORM) gv[it] = ld16(a.norm_w + vi * 8);
        }
    }
    WT wv[KIT][R];
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
        const int vi = tid + 256 * it;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            int n = n0 + r;
            n = n < a.N ? n : a.N - 1;
            wv[it][r] = WT{};
            if (vi < KV)
                wv[it][r] = __builtin_nontemporal_load(
                    reinterpret_cast<const WT*>(W8 + ((size_t)n * a.ldw + (size_t)vi * 8) * WB));
        }
    }

    uint32_t warm = 0;                                               // successor touches (l2_warm.h), behind the last weight load
    if constexpr (!FP8) warm = warm_touch(a.warm, blockIdx.x, tid);

    float rinv = 1.f;
    if constexpr (NORM) {
        float ss = 0.f;
#pragma unroll
        for (int it = 0; it < KIT; ++it) {
            float f[8];
            unpack8(xv[it], f);
#pragma unroll
            for (int j = 0; j < 8; ++j) ss += f[j] * f[j];
        }
        ss = wave_sum(ss);
        if (lane == 0) *reinterpret_cast<volatile float*>(&ssp[wave]) = ss;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const volatile float* sp = ssp;
        rinv = rsqrtf((sp[0] + sp[1] + sp[2] + sp[3]) / (float)a.K + a.eps);
    }

    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
        float xf[8];
        u32x4 xp = xv[it];                                           // bf16 pairs for the dot2 path
        if constexpr (NORM || FP8) unpack8(xv[it], xf);
        if constexpr (NORM) {
            float g[8];
            unpack8(gv[it], g);
#pragma unroll
            for (int j = 0; j < 8; ++j) xf[j] = g[j] * bfround(xf[j] * rinv);
            xp = pack8(xf);                                          // the reference's second rounding
            if constexpr (FP8) unpack8(xp, xf);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if constexpr (FP8) {
                f32x2_t a2 = {0.f, 0.f};
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8(wv[it][r][q], false);
                    const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8(wv[it][r][q], true);
                    a2 = __builtin_elementwise_fma(lo, f32x2_t{xf[4 * q], xf[4 * q + 1]}, a2);       // v_pk_fma_f32
                    a2 = __builtin_elementwise_fma(hi, f32x2_t{xf[4 * q + 2], xf[4 * q + 3]}, a2);
                }
                acc[r] += a2[0] + a2[1];
            } else {
                float t = acc[r];
                t = bf16_dot2(wv[it][r].x, xp.x, t);
                t = bf16_dot2(wv[it][r].y, xp.y, t);
                t = bf16_dot2(wv[it][r].z, xp.z, t);
                t = bf16_dot2(wv[it][r].w, xp.w, t);
                acc[r] = t;
            }
        }
    }

#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float v = wave_sum(acc[r]);
        if (lane == 0) red[wave][r] = v;
    }
    __syncthreads();
    if (tid < R) {
        float t = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
        if constexpr (FP8) { const int n = n0 + tid; t *= a.wscale[n < a.N ? n : a.N - 1]; }
        fin[tid] = t;
    }
    __syncthreads();
    if constexpr (EPI == EPI_SWIGLU) {
        if (tid < R / 2) {
            const int n = n0 + 2 * tid;
            if (n + 1 < a.N) {
                const float gt = bfround(fin[2 * tid] + (a.bias ? bf2f(a.bias[n]) : 0.f));
                const float up = bfround(fin[2 * tid + 1] + (a.bias ? bf2f(a.bias[n + 1]) : 0.f));
                a.out[n >> 1] = f2bf(bfround(silu(gt)) * up);
            }
        }
    } else {
        if (tid < R) {
            const int n = n0 + tid;
            if (n < a.N) {
                float v = fin[tid];
                if (a.bias) v += bf2f(a.bias[n]);
                v = bfround(v);
                if constexpr (EPI == EPI_SILU) v = bfround(silu(v));
                if constexpr (EPI == EPI_GELU) v = bfround(gelu_erf(v));
                if constexpr (EPI == EPI_RESID) v = v + bf2f(a.res[n]);
                a.out[n] = f2bf(v);
            }
        }
    }
    if constexpr (!FP8) asm volatile("" :: "v"(warm));
}

// Short rows (K <= 2560: the o_proj / down_proj of a tensor-parallel shard, K = 896 / 2240 at TP = 8): splitting such
// a row over 256 threads leaves most lanes idle and pays two barriers for a cross-wave sum.  Here every wave owns RW whole
// rows -- all loads up front, v_dot2c, one DPP wave reduction, lane 0 stores -- no LDS, no barrier: the launch is pure
// latency, so the shortest dependency chain wins.
template <int RW, int KITW, int EPI>
__global__ __launch_bounds__(256) void gemv_wave_kernel(const GemvArgs a) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int KV = a.K >> 3;
    const int n0 = (blockIdx.x * 4 + wave) * RW;
    u32x4 xv[KITW], wv[KITW][RW];
#pragma unroll
    for (int it = 0; it < KITW; ++it) {
        const int vi = lane + 64 * it;
        const int vc = vi < KV ? vi : KV - 1;                         // clamped; the activation is zeroed instead
        xv[it] = vi < KV ? ld16(a.x + vi * 8) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            int n = n0 + r;
            n = n < a.N ? n : a.N - 1;
            wv[it][r] = ld_stream(reinterpret_cast<const u32x4*>(a.W + (size_t)n * a.ldw + vc * 8));
        }
    }
    float acc[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) acc[r] = 0.f;
#pragma unroll
    for (int it = 0; it < KITW; ++it)
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            float t = acc[r];
            t = bf16_dot2(wv[it][r].x, xv[it].x, t);
            t = bf16_dot2(wv[it][r].y, xv[it].y, t);
            t = bf16_dot2(wv[it][r].z, xv[it].z, t);
            t = bf16_dot2(wv[it][r].w, xv[it].w, t);
            acc[r] = t;
        }
#pragma unroll
    for (int r = 0; r < RW; ++r) acc[r] = wave_sum(acc[r]);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            const int n = n0 + r;
            if (n < a.N) {
                float v = acc[r];
                if (a.bias) v += bf2f(a.bias[n]);
                v = bfround(v);
                if constexpr (EPI == EPI_RESID) v = v + bf2f(a.res[n]);
                a.out[n] = f2bf(v);
            }
        }
    }
}

// Skinny-M weight stream on the matrix cores (2 <= M <= 16 rows: beam search, CFG pairs).  The FMA kernel above costs
// M FMAs + an unpack per weight and goes VALU-bound past M = 2 (M = 5: 0.9 TB/s); here one v_mfma_f32_16x16x32_bf16
// consumes a 16-row x 32-k weight fragment exactly as it arrives from HBM (A operand: lane -> row l & 15, 8 consecutive k
// at 8 * (l >> 4)) against the activations as the B operand (col = activation row, same k), so the VALU does nothing in
// the loop.  A block owns 16 weight rows; its 4 waves interleave over 32-k blocks (together 256 contiguous bytes per
// row per step) and reduce through LDS.  Activations are re-read from L2 per fragment (no LDS staging, any K % 32 == 0).
template <int EPI, int RG>
__global__ __launch_bounds__(256) void gemv_mfma_kernel(const GemvArgs a) {
    typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
    __shared__ f32x4_t part[4][RG][64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * (16 * RG);
    const int mrow = i < a.M ? i : a.M - 1;                            // columns >= M duplicate the last row (discarded)
    const bf16_t* wp[RG];
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) {
        const int n = n0 + 16 * rg + i;
        wp[rg] = a.W + (size_t)(n < a.N ? n : a.N - 1) * a.ldw + g * 8;
    }
    const bf16_t* xp = a.x + (size_t)mrow * a.ldx + g * 8;
    const int KB = a.K >> 5;
    f32x4_t acc[RG];
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) acc[rg] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    constexpr int U = RG >= 4 ? 4 : 8;                                 // fragments in flight per row group
    int kb = wave;
    for (; kb + 4 * (U - 1) < KB; kb += 4 * U) {
        u32x4 wv[RG][U], xv[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            xv[j] = ld16(xp + (kb + 4 * j) * 32);                      // one activation fragment serves RG weight fragments
#pragma unroll
            for (int rg = 0; rg < RG; ++rg) wv[rg][j] = ld_stream(reinterpret_cast<const u32x4*>(wp[rg] + (kb + 4 * j) * 32));
        }
#pragma unroll
        for (int j = 0; j < U; ++j)
#pragma unroll
            for (int rg = 0; rg < RG; ++rg)
                acc[rg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wv[rg][j]),
                                                                  __builtin_bit_cast(bf16x8_t, xv[j]), acc[rg], 0, 0, 0);
    }
    for (; kb < KB; kb += 4) {
        const u32x4 xv = ld16(xp + kb * 32);
#pragma unroll
        for (int rg = 0; rg < RG; ++rg) {
            const u32x4 wv = ld_stream(reinterpret_cast<const u32x4*>(wp[rg] + kb * 32));
            acc[rg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wv),
                                                              __builtin_bit_cast(bf16x8_t, xv), acc[rg], 0, 0, 0);
        }
    }
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
        const int nb = n0 + 16 * rg + 4 * g;                           // first of this lane's 4 output columns
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


// fp8 (OCP e4m3fn) weight stream: half the HBM bytes per token.  One VB-byte load = VB weights of one row (16: long rows; 8: rows of
// K <= 8192, where 16-byte groups would leave 3.25 trips per lane at K = 6656 to half the lanes); the per-row fp32 scale is applied
// once to the fp32 dot product.  Same fused RMSNorm / epilogues as the bf16 kernel.
template <int R, int MB, bool NORM, int EPI, int NW, int VB>
__global__ __launch_bounds__(NW * 64) void gemv_fp8_kernel(const GemvArgs a) {
    static_assert(VB == 8 || VB == 16, "one weight load is 8 or 16 bytes");
    using WT = typename std::conditional<VB == 16, u32x4, u32x2>::type;
    __shared__ float red[NW][R * MB];
    __shared__ float red_ss[NW][MB];
    __shared__ float fin[R * MB];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int KV = a.K >> (VB == 16 ? 4 : 3);      // VB-element groups per row
    const int n0 = blockIdx.x * R;
    const uint8_t* W8 = reinterpret_cast<const uint8_t*>(a.W);
    const uint8_t* wrow[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int n = n0 + r;
        n = n < a.N ? n : a.N - 1;
        wrow[r] = W8 + (size_t)n * a.ldw;
    }
    // fused RMSNorm without a prologue: y = rinv * sum_k w[k] * (g[k] * x[k]), rinv = rsqrt(mean(x^2) + eps).  The sum of
    // squares rides along the one pass over x (every column belongs to exactly one lane of the workgroup), so the weight
    // stream starts at once instead of behind a load -> reduce -> barrier round trip; the reference's two bf16 rounding
    // points inside the norm are not reproduced (2^-9 relative, far below the e4m3 weight error of this optional stream).
    float ss[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) ss[m] = 0.f;
    float acc[R][MB];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int m = 0; m < MB; ++m) acc[r][m] = 0.f;

#pragma unroll 2
    for (int vi = tid; vi < KV; vi += NW * 64) {
        WT wv[R];
#pragma unroll
        for (int r = 0; r < R; ++r) wv[r] = __builtin_nontemporal_load(reinterpret_cast<const WT*>(wrow[r] + vi * VB));
        float xf[MB][VB];
        float g[VB];
        if constexpr (NORM) {
            unpack8(ld16(a.norm_w + vi * VB), g);
            if constexpr (VB == 16) unpack8(ld16(a.norm_w + vi * VB + 8), g + 8);
        }
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            if (m < a.M) {
                unpack8(ld16(a.x + (size_t)m * a.ldx + vi * VB), xf[m]);
                if constexpr (VB == 16) unpack8(ld16(a.x + (size_t)m * a.ldx + vi * VB + 8), xf[m] + 8);
                if constexpr (NORM) {
#pragma unroll
                    for (int j = 0; j < VB; ++j) { ss[m] = fmaf(xf[m][j], xf[m][j], ss[m]); xf[m][j] *= g[j]; }
                }
            } else {
#pragma unroll
                for (int j = 0; j < VB; ++j) xf[m][j] = 0.f;
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            f32x2_t wf[VB / 2];                                       // v_cvt_pk_f32_fp8 pairs feed v_pk_fma_f32
#pragma unroll
            for (int q = 0; q < VB / 4; ++q) {
                wf[2 * q] = __builtin_amdgcn_cvt_pk_f32_fp8(wv[r][q], false);
                wf[2 * q + 1] = __builtin_amdgcn_cvt_pk_f32_fp8(wv[r][q], true);
            }
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                f32x2_t a2 = {0.f, 0.f};
#pragma unroll
                for (int j = 0; j < VB / 2; ++j)
                    a2 = __builtin_elementwise_fma(wf[j], f32x2_t{xf[m][2 * j], xf[m][2 * j + 1]}, a2);
                acc[r][m] += a2[0] + a2[1];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            const float v = wave_sum(acc[r][m]);
            if (lane == 0) red[wave][r * MB + m] = v;
        }
    if constexpr (NORM) {
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            const float v = wave_sum(ss[m]);
            if (lane == 0) red_ss[wave][m] = v;
        }
    }
    __syncthreads();
    if (tid < R * MB) {
        const int n = n0 + tid / MB;
        float t = 0.f, rinv = 1.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += red[w][tid];
        if constexpr (NORM) {
            float q = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) q += red_ss[w][tid % MB];
            rinv = rsqrtf(q / (float)a.K + a.eps);
        }
        fin[tid] = t * rinv * a.wscale[n < a.N ? n : a.N - 1];
    }
    __syncthreads();
    if constexpr (EPI == EPI_SWIGLU) {
        if (tid < (R / 2) * MB) {
            const int j = tid / MB, m = tid % MB;
            const int n = n0 + 2 * j;
            if (m < a.M && n + 1 < a.N) {
                const float gt = bfround(fin[(2 * j) * MB + m] + (a.bias ? bf2f(a.bias[n]) : 0.f));
                const float up = bfround(fin[(2 * j + 1) * MB + m] + (a.bias ? bf2f(a.bias[n + 1]) : 0.f));
                a.out[(size_t)m * a.ldo + (n >> 1)] = f2bf(bfround(silu(gt)) * up);
            }
        }
    } else {
        if (tid < R * MB) {
            const int r = tid / MB, m = tid % MB;
            const int n = n0 + r;
            if (m < a.M && n < a.N) {
                float v = fin[tid];
                if (a.bias) v += bf2f(a.bias[n]);
                v = bfround(v);
                if constexpr (EPI == EPI_RESID) v = v + bf2f(a.res[(size_t)m * a.ldres + n]);
                a.out[(size_t)m * a.ldo + n] = f2bf(v);
            }
        }
    }
}

// ---- the launchers: plan values -> template arguments.  Grid and workgroup size come from the plan; nothing below tests a shape.

template <int R, int MB, bool NORM, int PRE>
int launch_block_epi(const GemvPlan& p, const GemvArgs& a, hipStream_t s) {
#define EMU_CASE(E) case E: hipLaunchKernelGGL((gemv_kernel<R, MB, NORM, E, PRE>), dim3(p.grid), dim3(p.block), 0, s, a); break;
    EMU_EPI5(EMU_CASE)
#undef EMU_CASE
}

// the block kernel's form as the template pair (NORM, PRE): preload = (false, 4), head = (true, -1), rolling = (norm, 0)
template <int R, int MB>
int launch_block(const GemvPlan& p, const GemvArgs& a, hipStream_t s) {
    if (p.form == GEMV_FORM_PRELOAD) {
        if constexpr (MB == 1 && R <= 4) return launch_block_epi<R, MB, false, 4>(p, a, s);       // register budget: PRE * R * 4 VGPRs
    } else if (p.form == GEMV_FORM_HEAD) {
        if constexpr (MB == 1) return launch_block_epi<R, MB, true, -1>(p, a, s);
    } else if (p.form == GEMV_FORM_ROLLING) {
        return a.norm_w ? launch_block_epi<R, MB, true, 0>(p, a, s) : launch_block_epi<R, MB, false, 0>(p, a, s);
    }
    return -22;
}

template <int R>
int launch_block_rows(const GemvPlan& p, const GemvArgs& a, hipStream_t s) {
    switch (p.mb) {
        case 1: return launch_block<R, 1>(p, a, s);
        case 2: return launch_block<R, 2>(p, a, s);
        case 3: return launch_block<R, 3>(p, a, s);
        case 4: return launch_block<R, 4>(p, a, s);
        case 5: return launch_block<R, 5>(p, a, s);           // 5 beams: the reference's default decoding mode
        case 8: return launch_block<R, 8>(p, a, s);
        default: return -22;
    }
}

template <int R, int KIT, bool FP8>
int launch_rt(const GemvPlan& p, const GemvArgs& a, hipStream_t s) {
#define EMU_CASE(E)                                                                                                              \
    case E:                                                                                                                      \
        if (a.norm_w) hipLaunchKernelGGL((gemv_rt_kernel<R, KIT, true, E, FP8>), dim3(p.grid), dim3(p.block), 0, s, a);          \
        else hipLaunchKernelGGL((gemv_rt_kernel<R, KIT, false, E, FP8>), dim3(p.grid), dim3(p.block), 0, s, a);                  \
        break;
    EMU_EPI5(EMU_CASE)
#undef EMU_CASE
}

template <int KITW>
int launch_wave(const GemvPlan& p, const GemvArgs& a, hipStream_t s) {
    if (a.epi == EPI_RESID) hipLaunchKernelGGL((gemv_wave_kernel<4, KITW, EPI_RESID>), dim3(p.grid), dim3(p.block), 0, s, a);
    else hipLaunchKernelGGL((gemv_wave_kernel<4, KITW, EPI_NONE>), dim3(p.grid), dim3(p.block), 0, s, a);
    EMU_CHECK_LAUNCH();
    return 0;
}

// Row groups per workgroup (each activation fragment, re-read from L2, then serves RG weight fragments): measured flat at M = 5
// (RG 1 / 2 / 4: 69.5 / 71.7 / 82.9 us on qkv), so the activation re-read is not what holds the kernel at 3.8 TB/s -- the
// 64-byte-per-row fragment loads are; RG = 1 keeps the most workgroups in flight.
int launch_mfma(const GemvPlan& p, const GemvArgs& a, hipStream_t s) {
#define EMU_CASE(E) case E: hipLaunchKernelGGL((gemv_mfma_kernel<E, 1>), dim3(p.grid), dim3(p.block), 0, s, a); break;
    EMU_EPI5(EMU_CASE)
#undef EMU_CASE
}

template <int R, int MB, int NW, int VB>
int launch_fp8(const GemvPlan& p, const GemvArgs& a, hipStream_t s) {
    static_assert(R * MB <= NW * 64, "epilogue needs one thread per (row, m)");
#define EMU_CASE(E)                                                                                                              \
    case E:                                                                                                                      \
        if (a.norm_w) hipLaunchKernelGGL((gemv_fp8_kernel<R, MB, true, E, NW, VB>), dim3(p.grid), dim3(p.block), 0, s, a);       \
        else hipLaunchKernelGGL((gemv_fp8_kernel<R, MB, false, E, NW, VB>), dim3(p.grid), dim3(p.block), 0, s, a);               \
        break;
    EMU_EPI3(EMU_CASE)
#undef EMU_CASE
}

int launch_planned(const GemvPlan& p, const GemvArgs& a, hipStream_t s) {
    if (p.status) return p.status;
    switch (p.family) {
        case GEMV_FAM_BLOCK:
            switch (p.rows) {
                case 2: return launch_block_rows<2>(p, a, s);
                case 4: return launch_block_rows<4>(p, a, s);
                case 8: return launch_block_rows<8>(p, a, s);
                case 16: return p.mb == 1 ? launch_block<16, 1>(p, a, s) : -22;    // 16 rows only pay at one row (accumulator registers)
                default: return -22;
            }
        case GEMV_FAM_RT: return p.trips == 4 ? launch_rt<4, 4, false>(p, a, s) : launch_rt<2, 9, false>(p, a, s);
        case GEMV_FAM_FP8_RT: return p.trips == 4 ? launch_rt<8, 4, true>(p, a, s) : launch_rt<4, 9, true>(p, a, s);
        case GEMV_FAM_WAVE:
            switch (p.trips) {
                case 1: return launch_wave<1>(p, a, s);
                case 2: return launch_wave<2>(p, a, s);
                case 3: return launch_wave<3>(p, a, s);
                case 4: return launch_wave<4>(p, a, s);
                case 5: return launch_wave<5>(p, a, s);
                default: return -22;
            }
        case GEMV_FAM_MFMA: return launch_mfma(p, a, s);
        case GEMV_FAM_THIN: return launch_gemv_thin(a, p, s);
        case GEMV_FAM_FP8_BLOCK:
            if (p.vb == 8) return p.mb == 1 ? launch_fp8<8, 1, 4, 8>(p, a, s) : launch_fp8<8, 2, 4, 8>(p, a, s);
            if (p.mb == 1) return p.waves == 2 ? launch_fp8<4, 1, 2, 16>(p, a, s) : launch_fp8<4, 1, 4, 16>(p, a, s);
            return p.rows == 4 ? launch_fp8<4, 2, 2, 16>(p, a, s) : launch_fp8<8, 2, 2, 16>(p, a, s);
        case GEMV_FAM_FP4_ROWS: return launch_gemv_fp4(a, p, s);
        case GEMV_FAM_FP8_THIN: return launch_gemv_fp8_thin(a, p, s);
        case GEMV_FAM_FP4_THIN: return launch_gemv_fp4_thin(a, p, s);
        default: return -22;
    }
}

// ---- the planner: every decision between a shape and a launch, in integers.  No HIP call, no global; the tune mask (emu_gemm_tune)
// is an argument.  tests/test_gemv_plan.py holds its answers against the launches recorded before it existed.

// the one-row wave form's 64-lane trips per row (1..5), or 0 when the shape is not covered
int gemv_wave_trips(int N, int K, bool norm, int epi) {
    if (norm || (epi != EPI_NONE && epi != EPI_RESID)) return 0;
    const int kitw = ((K >> 3) + 63) / 64;
    return kitw > 5 || N < 1024 ? 0 : kitw;                          // K <= 2560; tiny N stays on the block kernels
}
// the single-round-trip form's built trip count (4 or 9) that holds the row, or 0 when the shape is not covered
int gemv_rt_trips(int N, int K, bool norm, int epi, bool f8) {
    if (epi == EPI_SWIGLU && (N & 1)) return 0;
    const int kit = ((K >> 3) + 255) / 256;
    if (f8 && (epi == EPI_SILU || epi == EPI_GELU)) return 0;
    // measured (tools/kbench.py, profiles/r01_gemv_variants.log): one round trip wins for matrices small enough
    // that latency, not bandwidth, sets the time (TP shards, tiny models) and for long rows without the RMSNorm
    // prologue (down_proj: 6.3 vs 5.85 TB/s); big fused-norm matrices amortise the prologue better over 8 rows
    const size_t bytes = (size_t)N * K * (f8 ? 1 : 2);
    const bool small = bytes < ((size_t)(f8 ? 32 : 64) << 20);
    const bool long_rows = !f8 && kit >= 5 && !norm;
    if (!small && !long_rows) return 0;
    return kit <= 4 ? 4 : kit <= 9 ? 9 : 0;
}
// the form of the one-row block kernel for R rows per workgroup.  The preload form wins only for plain streams (o_proj); with the
// RMSNorm prologue it loses 20 % (clamped tail chunks + lower occupancy), so those take the head form or the rolling loop.
int gemv_block_form(int R, int K, bool norm) {
    if (!norm && R <= 4 && (K >> 3) <= 1024) return GEMV_FORM_PRELOAD;
    if (norm && (K >> 3) <= 1024) return GEMV_FORM_HEAD;
    return GEMV_FORM_ROLLING;
}
// rows per workgroup for 2..8 activation rows (beam search, CFG pairs): 8 amortises the activation unpack best
int gemv_rows_per_block_multi(int N) {
    int R = 8;
    while (R > 2 && (N + R - 1) / R < 512) R >>= 1;
    return R;
}

GemvPlan planned(const GemvShape& sh, int family, int form, int rows, int mb, int waves, int trips) {
    GemvPlan p{};
    p.family = family; p.form = form; p.rows = rows; p.mb = mb; p.waves = waves; p.trips = trips;
    p.grid = (sh.N + rows - 1) / rows; p.block = 64 * waves;
    p.partition = family == GEMV_FAM_WAVE ? 1 : family == GEMV_FAM_BLOCK || family == GEMV_FAM_RT || family == GEMV_FAM_FP8_RT ? 4 : 0;
    return p;
}

// one bf16 row, the arguments checked by the caller: wave form, single round trip, or the block kernel in one of its three forms
// (emu_gemm_tune bit 17, tests: no wave / single-round-trip form, so small matrices reach the block kernel's head and preload forms)
GemvPlan plan_one_row(const GemvShape& sh, int tune) {
    const bool norm = sh.norm != 0, block_only = (tune & (1 << 17)) != 0;
    if (const int kitw = block_only ? 0 : gemv_wave_trips(sh.N, sh.K, norm, sh.epi))
        return planned(sh, GEMV_FAM_WAVE, GEMV_FORM_WAVE, 16, 1, 4, kitw);         // 4 waves x 4 whole rows
    if (const int kit = block_only ? 0 : gemv_rt_trips(sh.N, sh.K, norm, sh.epi, false))
        return planned(sh, GEMV_FAM_RT, GEMV_FORM_RT, kit == 4 ? 4 : 2, 1, 4, kit);
    const int R = emu_gemv_rows_per_block(sh.N, sh.K, norm);
    const int form = gemv_block_form(R, sh.K, norm);
    return planned(sh, GEMV_FAM_BLOCK, form, R, 1, 4, form == GEMV_FORM_PRELOAD ? 4 : form == GEMV_FORM_HEAD ? -1 : 0);
}

// ---- the three matrix-core few-row streams (gemv_thin.hip, gemv_fp8_thin.hip, gemv_fp4_thin.hip): rows weight rows per workgroup of
// 4 waves, the activation rows in a bucket of mb = 8 (up to 8 rows) or 16, K walked in stages of kch 16-byte slots per weight row
// through a ring of `stages` stages in LDS
GemvPlan thin_planned(const GemvShape& sh, int family, int rows, int stages, int kch) {
    GemvPlan p = planned(sh, family, 0, rows, sh.M <= 8 ? 8 : 16, 4, 0);
    p.stages = stages; p.kch = kch;
    return p;
}
// bf16: 16 weight rows per workgroup (three co-resident workgroups per CU at <= 8 rows): measured at 5 rows against 32-row
// workgroups and 512-k stages (tools/thin_ab.py, profiles/r03_thin_stream_ab.log): qkv 42.1 vs 45.5 / 47.1 us.
// emu_gemm_tune bits 8-11 pick the other variants (A/B aid).
GemvPlan plan_thin(const GemvShape& sh, int tune) {
    const int variant = (tune >> 8) & 15;
    const bool rows8 = sh.M <= 8;
    int rn = 16, nstg = 4, kch = 32;
    if (variant == 1 && (sh.N + 31) / 32 >= 512) { rn = 32; nstg = 3; }
    else if (variant == 2) nstg = rows8 ? 6 : 3;
    else if (variant == 3 && rows8 && sh.K % 512 == 0) { nstg = 3; kch = 64; }
    return thin_planned(sh, GEMV_FAM_THIN, rn, nstg, kch);
}
// the epilogues the byte-fed kernels are built with (store_c4, fp4_tile.h)
bool epi3_ok(const GemvShape& sh) {
    return sh.epi == EPI_NONE || sh.epi == EPI_RESID || (sh.epi == EPI_SWIGLU && !(sh.N & 1));
}
// what both MXFP4 matrix-core kernels (gemv_fp4_thin.hip: 1..16 rows, gemm_fp4.hip: 17 and more) ask of a shape, the row count
// aside: K >= 256 in whole MX blocks (K % 256 != 0: the last stage partial, the TAIL instantiations), 16-byte element rows, scale
// rows of whole stages (fp4_scale_stride) fetched 4 bytes at a time, 16-byte aligned W and x, no fused norm
bool fp4_mfma_shape_ok(const GemvShape& sh) {
    return sh.fp4 && !sh.fp8 && !sh.norm && sh.w_aligned && sh.x_aligned && sh.N >= 1 && sh.K >= 256 && (sh.K & 31) == 0 &&
           (sh.ldw & 15) == 0 && (sh.ldx & 7) == 0 && (sh.lds & 3) == 0 && sh.ldw >= sh.K / 2 && sh.ldx >= sh.K &&
           sh.lds >= fp4_scale_stride(sh.K) && epi3_ok(sh);
}
// The matrix-core few-row plan of the shape's weight kind (sh.fp8 / sh.fp4; neither: bf16), or status -22.
//   bf16   2..16 rows, whole 256-wide k stages, no fused norm, 16-byte aligned operands, epilogues NONE .. GELU: plan_thin.
//   fp8    1..16 rows, whole 256-wide k stages (kch 16).  32 weight rows per workgroup halve what a workgroup re-stages of the
//          activations per weight byte (mb * 512 against rows * 256 bytes per stage); 16 where 32 would leave fewer than 128
//          workgroups, half the CUs of the device (short shards, the tests' small N).  The ring is as deep as 48 KiB hold: three
//          workgroups share a CU's LDS.
//   MXFP4  1..16 rows (kch 8).  32 weight rows per workgroup: measured against 16 at the five LLaMA-33B shapes (tools/fp4_wide_time.py
//          --ab), 32 rows win everywhere, also where they leave CUs without a workgroup -- qkv 28.1 vs 42.0 us, o_proj 13.1 vs
//          17.6, down 25.5 vs 38.6 at 5 rows: the activation rows a workgroup re-stages from L2 weigh twice the 4-bit bytes of 16
//          weight rows.  Ring depth by (rows, mb) as built: 32/8: 5, 16/8: 6, 32/16 and 16/16: 4 (32/16/4 is 53248 bytes, not the
//          48 KiB of the others).  The same tiles whether or not K ends in a partial stage.
// emu_gemm_tune bits 28-29 pin the weight rows of the two byte-fed streams to 16 / 32 (1 / 2).
GemvPlan gemv_thin_plan(const GemvShape& sh, int tune) {
    GemvPlan refused{};
    refused.status = -22;
    const int pin = (tune >> 28) & 3;
    if (sh.fp4) {
        if (sh.M < 1 || sh.M > 16 || !fp4_mfma_shape_ok(sh)) return refused;
        const int rows = pin == 1 ? 16 : 32;
        return thin_planned(sh, GEMV_FAM_FP4_THIN, rows, sh.M > 8 ? 4 : rows == 32 ? 5 : 6, 8);
    }
    if (sh.norm || !sh.w_aligned || !sh.x_aligned || sh.M > 16 || sh.N < 1 || sh.K < 256 || (sh.K % 256) || (sh.ldx & 7)) return refused;
    if (sh.fp8) {
        if (sh.M < 1 || (sh.ldw & 15) || sh.ldw < sh.K || sh.ldx < sh.K || !epi3_ok(sh)) return refused;
        const int rows = pin == 1 ? 16 : pin == 2 ? 32 : (sh.N + 31) / 32 >= 128 ? 32 : 16;
        return thin_planned(sh, GEMV_FAM_FP8_THIN, rows, 49152 / (rows * 256 + (sh.M <= 8 ? 8 : 16) * 512), 16);
    }
    if (sh.M < 2 || (sh.ldw & 7) || sh.epi < EPI_NONE || sh.epi > EPI_GELU || (sh.epi == EPI_SWIGLU && (sh.N & 1))) return refused;
    return plan_thin(sh, tune);
}

// the MXFP4 weight stream (gemv_fp4.hip): 16-byte loads of whole blocks, 32-bit row offsets; emu_gemm_tune bits 24-25 set the row
// sets per workgroup, bits 26-27 the weight rows per lane
GemvPlan plan_fp4_rows(const GemvShape& sh, int tune) {
    GemvPlan refused{};
    refused.status = -22;
    if (sh.M < 1 || sh.M > 2 || sh.N < 1 || sh.K < 32 || (sh.K & 31)) return refused;
    if ((sh.ldw & 15) || (sh.ldx & 7) || sh.ldw < sh.K / 2 || sh.lds < sh.K / 32) return refused;
    if (sh.epi != EPI_NONE && sh.epi != EPI_RESID && sh.epi != EPI_SWIGLU) return refused;
    if (sh.epi == EPI_SWIGLU && (sh.N & 1)) return refused;
    int tpr, rs;
    plan_fp4(sh.K >> 5, &tpr, &rs);
    if ((tune >> 24) & 3) rs = 1 << (((tune >> 24) & 3) - 1);
    if (rs > GEMV_FP4_MAX_SETS || rs * tpr > 1024) return refused;
    if ((size_t)sh.N * sh.ldw > 0xffffffffull || (size_t)sh.N * sh.lds > 0xffffffffull) return refused;
    // one row: 8 weight rows per lane share one unpack of the activations, where the grid still covers the device with them; two
    // rows keep 4 (the accumulators and activations of 8 x 2 do not fit the 128 registers of a 13-wave workgroup)
    const bool wide = (sh.N + rs * 8 - 1) / (rs * 8) >= 128;
    const int asked = 4 * ((tune >> 26) & 3);
    const int rpl = sh.M > 1 || asked == 4 || (!wide && asked != 8) ? 4 : 8;
    GemvPlan p = planned(sh, GEMV_FAM_FP4_ROWS, 0, rs * rpl, sh.M, (tpr * rs + 63) / 64, 0);   // lanes beyond the last row set idle
    p.tpr = tpr; p.row_sets = rs; p.rpl = rpl;
    return p;
}

}  // namespace

int emu_gemv_rows_per_block(int N, int K, bool norm) {
    // measured (tools/kbench.py, profiles/): plain streams are fastest with 2 rows per workgroup (more, smaller workgroups
    // balance the 256 CUs better).  Kernels with the fused RMSNorm prologue wanted 8-16 rows so the prologue was amortised;
    // in the head form (K <= 8192: the weight stream starts before the statistics are reduced) the prologue no longer
    // stalls the stream and 4 rows win: decode 93.1 (16 rows) / 93.6 (8) / 95.0 (4) tokens/s, 2 rows lose 12 %.
    int R = norm ? ((K >> 3) <= 1024 ? 4 : 16) : 2;
    while (R > 2 && (N + R - 1) / R < (R == 16 ? 1024 : 512)) R >>= 1;
    return R;
}

bool gemv_rows_9_16_ok(int M, int K, int ldx, int ldw, bool norm, bool fp8, int epi) {
    return M > 8 && M <= 16 && !norm && !fp8 && (K & 31) == 0 && (ldw & 7) == 0 && (ldx & 7) == 0 && epi >= EPI_NONE && epi <= EPI_GELU;
}

GemvPlan gemv_plan(const GemvShape& sh, int tune) {
    GemvPlan refused{};
    refused.status = -22;
    const bool norm = sh.norm != 0, f8 = sh.fp8 != 0;
    if (sh.fp4) return f8 ? refused : plan_fp4_rows(sh, tune);
    if (sh.M < 1 || sh.M > 16 || (sh.K & 7) || sh.N < 1) return refused;
    if (sh.epi < EPI_NONE || sh.epi > (f8 ? EPI_SWIGLU : EPI_GELU)) return refused;
    if (sh.epi == EPI_SWIGLU && (sh.N & 1)) return refused;
    // 4..16 rows with whole 256-wide k stages: LDS-DMA stages + MFMA (gemv_thin.hip).  Measured on the LLaMA-33B shapes
    // (tools/thin_ab.py, profiles/r03_thin_stream_ab.log): 5 rows 42.7 / 17.9 / 74.6 / 42.6 us (qkv / o / gate-up / down) against
    // 46.4 / 21.7 / 77.4 / 47.6 on the v_dot2c kernel, 8 rows 43.7 vs 60.7, 16 rows 49.2 vs 92.0 (register-fed MFMA); at 2-3
    // rows the v_dot2c kernel is level or ahead (qkv 40.6 vs 41.0).  emu_gemm_tune bit 2 switches it off (A/B).
    if (sh.M >= 4 && !(tune & 4) && !f8)
        if (const GemvPlan p = gemv_thin_plan(sh, tune); !p.status) return p;
    // 9..16 rows: the register-fed 16x16x32 MFMA stream.  Up to 8 rows the v_dot2c block kernel is faster (M = 2: 6.4 vs 4.1 TB/s,
    // M = 5: 4.5 vs 3.9, M = 8: 3.7 vs 3.5; tools/kbench.py --filter rows): its row-contiguous 1 KiB loads use HBM better
    // than the MFMA fragment's 64 bytes per row.
    if (sh.M > 8)
        return gemv_rows_9_16_ok(sh.M, sh.K, sh.ldx, sh.ldw, norm, f8, sh.epi) ? planned(sh, GEMV_FAM_MFMA, 0, 16, 16, 4, 0) : refused;
    if (f8) {                                        // fp8 weight stream (decode, batch <= 2 built)
        if ((sh.K & 15) || sh.M > 2) return refused;
        if (const int kit = sh.M == 1 ? gemv_rt_trips(sh.N, sh.K, norm, sh.epi, true) : 0)
            return planned(sh, GEMV_FAM_FP8_RT, GEMV_FORM_RT, kit == 4 ? 8 : 4, 1, 4, kit);
        // K = 6656 is only 416 16-byte groups, so rows of K <= 8192 take 8-byte loads on 4-wave blocks (3.25 trips per lane, like
        // the bf16 kernel); longer rows 16-byte loads: one row 4 rows x 4 waves (down_proj: 21.8 vs 23.1 us), few workgroups 2 waves
        GemvPlan p;
        if (sh.K <= 8192) p = planned(sh, GEMV_FAM_FP8_BLOCK, 0, 8, sh.M, 4, 0);
        else {
            const bool small = (sh.N + 7) / 8 < 512;
            p = planned(sh, GEMV_FAM_FP8_BLOCK, 0, small || sh.M == 1 ? 4 : 8, sh.M, sh.M == 1 && !small ? 4 : 2, 0);
        }
        p.vb = sh.K <= 8192 ? 8 : 16;
        return p;
    }
    if (sh.M == 1) return plan_one_row(sh, tune);
    return planned(sh, GEMV_FAM_BLOCK, GEMV_FORM_ROLLING, gemv_rows_per_block_multi(sh.N), sh.M <= 5 ? sh.M : 8, 4, 0);
}

// the one-row views of the plan (the successor's geometry for l2_warm.h and the persistent engine's column partition come from the
// same place as the launch)
GemvShape gemv_one_row_shape(int N, int K, bool norm, int epi) {
    GemvShape sh{};
    sh.M = 1; sh.N = N; sh.K = K; sh.ldx = sh.ldw = K; sh.epi = epi; sh.norm = norm; sh.w_aligned = sh.x_aligned = 1;
    return sh;
}
static GemvPlan one_row_view(int N, int K, bool norm, int epi) {
    return plan_one_row(gemv_one_row_shape(N, K, norm, epi), emu_gemm_tune_get());
}
GemvGeom emu_gemv_geometry(int N, int K, bool norm, int epi) {
    const GemvPlan p = one_row_view(N, K, norm, epi);
    return {p.form, p.rows};
}
int emu_gemv_partition(int N, int K, bool norm, int epi) { return one_row_view(N, K, norm, epi).partition; }

GemvShape gemv_shape_of(const GemvArgs& a) {
    GemvShape sh{};
    sh.M = a.M; sh.N = a.N; sh.K = a.K; sh.ldx = a.ldx; sh.ldw = a.ldw; sh.lds = a.lds; sh.epi = a.epi;
    sh.norm = a.norm_w != nullptr; sh.fp8 = a.wscale != nullptr; sh.fp4 = a.w4scale != nullptr;
    sh.w_aligned = (reinterpret_cast<size_t>(a.W) & 15) == 0; sh.x_aligned = (reinterpret_cast<size_t>(a.x) & 15) == 0;
    return sh;
}
int launch_gemv(const GemvArgs& a, hipStream_t s) {
    return launch_planned(gemv_plan(gemv_shape_of(a), emu_gemm_tune_get()), a, s);
}

// what only the pointers of an argument block can answer for the matrix-core kernels (the scale pointer of the weight kind is what
// names the kind in gemv_shape_of, so it is there)
static bool mfma_pointers_ok(const GemvArgs& a) {
    return a.x && a.W && a.out && (a.epi != EPI_RESID || a.res) && (reinterpret_cast<size_t>(a.w4scale) & 3) == 0;
}
int launch_gemv_thin_stream(const GemvArgs& a, hipStream_t s) {
    const GemvPlan p = gemv_thin_plan(gemv_shape_of(a), emu_gemm_tune_get());
    return p.status || !mfma_pointers_ok(a) ? -22 : launch_planned(p, a, s);
}
bool fp4_mfma_ok(const GemvArgs& a) { return a.M >= 17 && fp4_mfma_shape_ok(gemv_shape_of(a)) && mfma_pointers_ok(a); }

// The fp8 W8A16 GEMM of 17..64 rows (gemm_fp8.hip): 64 weight rows per workgroup, the activation rows in one tile of bm = 32 (narrow,
// up to 32 rows) or 64, K in whole stages of 256 through a ring of `stages` stages.  What it asks of a shape is what the fp8 few-row
// stream asks (gemv_thin_plan), the row count aside.  Ring depth: as deep as a CU's 160 KiB of LDS hold for one workgroup (narrow 4 x
// 32 KiB, one tile 3 x 48 KiB); emu_gemm_tune bit 20 gives the narrow form a ring of 2 (64 KiB: two workgroups per CU), the A/B twin
// (tools/fp8_mid_time.py --ab, profiles/fp8_mid.md).
// what the forms of the W8A16 GEMM ask of a shape, the row count aside
static bool fp8_gemm_shape_ok(const GemvShape& sh) {
    return sh.fp8 && !sh.fp4 && !sh.norm && sh.w_aligned && sh.x_aligned && sh.N >= 1 && sh.K >= 256 && !(sh.K % 256) && !(sh.ldx & 7) &&
           !(sh.ldw & 15) && sh.ldw >= sh.K && sh.ldx >= sh.K && epi3_ok(sh);
}
GemmFp8wPlan gemm_fp8w_plan(const GemvShape& sh, int tune) {
    GemmFp8wPlan refused{};
    refused.status = -22;
    if (sh.M < 17 || sh.M > 64 || !fp8_gemm_shape_ok(sh)) return refused;
    GemmFp8wPlan p{};
    p.form = sh.M <= 32 ? 1 : 2;
    p.bm = sh.M <= 32 ? 32 : 64;
    p.kc = 256;
    p.stages = p.form == 2 ? 3 : (tune & (1 << 20)) ? 2 : 4;
    p.lds_bytes = p.stages * (64 * p.kc + p.bm * p.kc * 2);
    p.grid = (sh.N + 63) / 64;
    p.block = 256;
    return p;
}
int launch_gemm_fp8w_stream(const GemvArgs& a, hipStream_t s) {
    const GemmFp8wPlan p = gemm_fp8w_plan(gemv_shape_of(a), emu_gemm_tune_get());
    return p.status || !mfma_pointers_ok(a) ? -22 : launch_gemm_fp8w(a, p, s);
}
// The same kernel for 65 rows and more: 64 weight rows x 128 activation rows per workgroup, grid.x over the row tiles so that the
// workgroups in flight share weight rows in L2, grid.y (at most 65535) over the column tiles; a ring of two 80 KiB stages is the CU's
// 160 KiB of LDS.  No tune bit is read.
GemmFp8tPlan gemm_fp8t_plan(const GemvShape& sh, int) {
    GemmFp8tPlan refused{};
    refused.status = -22;
    if (sh.M < 65 || !fp8_gemm_shape_ok(sh) || (sh.N + 63) / 64 > 65535) return refused;
    GemmFp8tPlan p{};
    p.form = 3;
    p.bm = 128;
    p.kc = 256;
    p.stages = 2;
    p.lds_bytes = p.stages * (64 * p.kc + p.bm * p.kc * 2);
    p.grid_x = (sh.M + 127) / 128;
    p.grid_y = (sh.N + 63) / 64;
    p.block = 256;
    return p;
}
int launch_gemm_fp8t_stream(const GemvArgs& a, hipStream_t s) {
    const GemmFp8tPlan p = gemm_fp8t_plan(gemv_shape_of(a), emu_gemm_tune_get());
    return p.status || !mfma_pointers_ok(a) ? -22 : launch_gemm_fp8t(a, p, s);
}

// The 13-bit packed twin of the bf16 thin stream (gemv_pack_thin.hip), from the bf16 plan of the same shape: it exists for kch 32.
// The built tiles, as (weight rows, ring depth: workgroups that share a CU's LDS): up to 8 activation rows (16, 4: 3), (32, 4: 2),
// (16, 6: 2), (32, 3: 3); up to 16 (16, 3: 3), (32, 3: 2), (16, 5: 2).  The plan is the tile whose grid fills the largest share of its
// whole rounds of 256 x (workgroups per CU) places, the first of equals in that order, which is the measured one.
// Measured at 5 rows (tools/pack_wide_time.py --ab, us, 16 / 32 weight rows): lm_head, 1009 workgroups of 32 on 2 x 512 places, 65.5 /
// 60.3 (a tie with 2018 of 16 at six stages); qkv, a tie of 1248 on 2 x 768 and 624 on 768, 37.1 / 44.6; down_proj, 416 on 512 at six stages, 41.4 / 40.0.  At 9..16 rows
// the rule leaves gate/up on 16 rows (85.2 us) where 32 measure 78.7: there the activation rows a workgroup re-stages outweigh the fill.
// emu_gemm_tune bits 28-29 pin 16 / 32 weight rows as for the byte-fed streams.
GemvPlan gemv_pack_thin_plan(const GemvShape& sh, int set_rows, int tune) {
    GemvPlan refused{};
    refused.status = -22;
    if (sh.fp8 || sh.fp4 || sh.norm || sh.M < 4 || sh.M > 16 || (set_rows != 2 && set_rows != 4)) return refused;
    if (sh.epi != EPI_NONE && sh.epi != EPI_RESID && sh.epi != EPI_SWIGLU) return refused;
    const GemvPlan b = gemv_plan(sh, tune);
    if (b.status || b.family != GEMV_FAM_THIN || b.kch != 32) return refused;
    struct Tile { int rows, stages, per_cu; };
    static const Tile tiles8[] = {{16, 4, 3}, {32, 4, 2}, {16, 6, 2}, {32, 3, 3}}, tiles16[] = {{16, 3, 3}, {32, 3, 2}, {16, 5, 2}};
    const Tile* tiles = sh.M <= 8 ? tiles8 : tiles16;
    const int ntiles = sh.M <= 8 ? 4 : 3, pin = (tune >> 28) & 3;
    const Tile* best = nullptr;
    long best_num = 0, best_den = 1;                                   // the filled share grid / (rounds * places), as a fraction
    for (int t = 0; t < ntiles; ++t) {
        if ((pin == 1 && tiles[t].rows != 16) || (pin == 2 && tiles[t].rows != 32)) continue;
        const long grid = (sh.N + tiles[t].rows - 1) / tiles[t].rows, places = 256L * tiles[t].per_cu;
        const long den = (grid + places - 1) / places * places;
        if (!best || grid * best_den > best_num * den) { best = &tiles[t]; best_num = grid; best_den = den; }
    }
    return thin_planned(sh, GEMV_FAM_PACK_THIN, best->rows, best->stages, 32);
}

// C-ABI test hooks (include/emu_hip.h)
int emu_gemv_pack_thin_plan(const emu_gemv_shape* shape, int set_rows, int tune, emu_gemv_plan_t* out) {
    return shape && out ? (*out = gemv_pack_thin_plan(*shape, set_rows, tune)).status : -22;
}
int emu_gemv_plan(const emu_gemv_shape* shape, int tune, emu_gemv_plan_t* out) {
    return shape && out ? (*out = gemv_plan(*shape, tune)).status : -22;
}
int emu_gemv_thin_plan(const emu_gemv_shape* shape, int tune, emu_gemv_plan_t* out) {
    return shape && out ? (*out = gemv_thin_plan(*shape, tune)).status : -22;
}
int emu_gemm_fp8w_plan(int M, int N, int K, int ldx, int ldw, int epi, int tune, emu_gemm_fp8w_plan_t* out) {
    if (!out) return -22;
    GemvShape sh{};
    sh.M = M; sh.N = N; sh.K = K; sh.ldx = ldx; sh.ldw = ldw; sh.epi = epi; sh.fp8 = sh.w_aligned = sh.x_aligned = 1;
    return (*out = gemm_fp8w_plan(sh, tune)).status;                 // refused: every field but the status is 0
}
int emu_gemm_fp8t_plan(int M, int N, int K, int ldx, int ldw, int epi, int tune, emu_gemm_fp8t_plan_t* out) {
    if (!out) return -22;
    GemvShape sh{};
    sh.M = M; sh.N = N; sh.K = K; sh.ldx = ldx; sh.ldw = ldw; sh.epi = epi; sh.fp8 = sh.w_aligned = sh.x_aligned = 1;
    return (*out = gemm_fp8t_plan(sh, tune)).status;                 // refused: every field but the status is 0
}
// the older view of the fp8 few-row plan: row-contiguous or strided operands on aligned buffers, no fused norm
int emu_gemv_fp8_thin_plan(int M, int N, int K, int ldx, int ldw, int epi, int tune, emu_gemv_fp8_thin_plan_t* out) {
    if (!out) return -22;
    GemvShape sh{};
    sh.M = M; sh.N = N; sh.K = K; sh.ldx = ldx; sh.ldw = ldw; sh.epi = epi; sh.fp8 = sh.w_aligned = sh.x_aligned = 1;
    const GemvPlan p = gemv_thin_plan(sh, tune);                     // refused: every field but the status is 0
    *out = {p.status, p.rows, p.mb, p.status ? 0 : 256, p.stages, p.stages * (p.rows * 256 + p.mb * 512), p.grid, p.block};
    return p.status;
}
