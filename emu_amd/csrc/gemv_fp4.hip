// MXFP4 weight stream for decode rows (M <= 2):  out[m, n] = epilogue( sum_k xeff[m, k] * fp4(W4[n, k]) * 2^(S[n, k / 32] - 127) )
//
// The format (emu_amd/mxfp4.py is its definition): elements uint8 [N, K/2], element 2j in the low nibble of byte j (sign bit +
// E2M1: 0, 0.5, 1, 1.5, 2, 3, 4, 6); scales uint8 [N, K/32], E8M0, one per 32 consecutive elements of a row.  0.53125 byte per
// weight: 0.27 of the bf16 stream, 0.53 of the fp8 stream (gemv.hip).  Not a reference feature (the reference is bf16 end to end).
//
// One 16-byte load is exactly one MX block and one scale byte.  Decoding is v_cvt_scalef32_pk_f32_fp4: one byte -> two fp32, the
// low nibble in result lane 0, multiplied by 2^(exponent field of the scale operand - 127) -- mantissa and sign of the operand are
// ignored, results below 2^-126 are kept as denormals (pinned by tests/test_gpu_fp4.py::test_decode_exhaustive).  So the scale
// operand is simply (byte << 23), the scale is applied per block inside the conversion, and the fp32 accumulation sees exact weights.
//
// Work split.  A lane owns one block column and walks R weight rows with it (the activation unpack is shared by the R rows); the
// lanes of a 16-lane DPP row sit on 16 consecutive blocks (256 contiguous element bytes, 16 contiguous scale bytes).  K = 6656 is
// 208 blocks = 13 x 16: not a whole number of waves, but a whole number of 16-lane rows.  So a workgroup is cut into `rs` row
// sets of `tpr` threads (a multiple of 16; plan_fp4 picks it so that trips x tpr covers the K/32 blocks with the least idle lanes:
// 208 -> 1 trip of 208, 560 -> 5 trips of 112, 70 -> 1 trip of 80, 28 -> 1 trip of 32), every set owns R rows, rs x tpr is a whole
// number of waves (208 x 4 = 13 waves, all lanes busy), and the K reduction is a DPP sum inside each 16-lane row followed by a
// sum of the row partials through LDS -- a wave may straddle two row sets, a 16-lane row never does.
//
// The fused RMSNorm has no prologue (as in gemv_fp8_kernel): y = rinv * sum_k w[k] * (g[k] * x[k]); the sum of squares rides along the
// pass over x, which every row set makes exactly once.  The only barriers are behind the last weight load.
#include "common.h"
#include "kernels.h"

namespace {

template <int R, int MB, bool NORM, int EPI>
__global__ __launch_bounds__(1024) void gemv_fp4_kernel(const GemvArgs a, const int tpr, const int rs) {
    __shared__ float red[64][R * MB];              // one slot per 16-lane row of the workgroup (<= 1024 / 16)
    __shared__ float red_ss[64][MB];
    __shared__ float fin[GEMV_FP4_MAX_SETS * R * MB];
    const int tid = threadIdx.x;
    const int grp = tid >> 4, gpt = tpr >> 4;      // 16-lane row of this thread; 16-lane rows per row set
    const int set = grp / gpt;
    const int KB = a.K >> 5;                       // MX blocks per weight row
    const int kb0 = set < rs ? tid - set * tpr : KB;
    const int n0 = (blockIdx.x * rs + (set < rs ? set : 0)) * R;
    // 32-bit row offsets against the two (uniform) base pointers: half the address registers of R pointer pairs (launch_gemv_fp4
    // checks that both arrays are within reach)
    const uint8_t* W4 = reinterpret_cast<const uint8_t*>(a.W);
    uint32_t wrow[R], srow[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int n = n0 + r;
        n = n < a.N ? n : a.N - 1;                 // tail rows: clamp loads, mask stores
        wrow[r] = (uint32_t)n * (uint32_t)a.ldw;
        srow[r] = (uint32_t)n * (uint32_t)a.lds;
    }
    float ss[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) ss[m] = 0.f;
    float acc[R][MB];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int m = 0; m < MB; ++m) acc[r][m] = 0.f;

    for (int kb = kb0; kb < KB; kb += tpr) {
        u32x4 wv[R];
        uint32_t sb[R];
#pragma unroll
        for (int r = 0; r < R; ++r) wv[r] = ld_stream(reinterpret_cast<const u32x4*>(W4 + (wrow[r] + (uint32_t)kb * 16u)));
#pragma unroll
        for (int r = 0; r < R; ++r) sb[r] = (uint32_t)__builtin_nontemporal_load(a.w4scale + (srow[r] + (uint32_t)kb)) << 23;
#pragma unroll
        for (int q = 0; q < 4; ++q) {              // dword q of the block = elements 8q .. 8q + 7 = one 16-byte chunk of x
            float xf[MB][8];
            float g[8];
            if constexpr (NORM) unpack8(ld16(a.norm_w + kb * 32 + q * 8), g);
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                if (m < a.M) {
                    unpack8(ld16(a.x + (size_t)m * a.ldx + kb * 32 + q * 8), xf[m]);
                    if constexpr (NORM) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) { ss[m] = fmaf(xf[m][j], xf[m][j], ss[m]); xf[m][j] *= g[j]; }
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) xf[m][j] = 0.f;
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float sc = __uint_as_float(sb[r]);
                f32x2_t wf[4];                                        // v_cvt_scalef32_pk_f32_fp4 pairs feed v_pk_fma_f32
                wf[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(wv[r][q], sc, 0);
                wf[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(wv[r][q], sc, 1);
                wf[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(wv[r][q], sc, 2);
                wf[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(wv[r][q], sc, 3);
#pragma unroll
                for (int m = 0; m < MB; ++m) {
                    f32x2_t a2 = {0.f, 0.f};
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        a2 = __builtin_elementwise_fma(wf[j], f32x2_t{xf[m][2 * j], xf[m][2 * j + 1]}, a2);
                    acc[r][m] += a2[0] + a2[1];
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            const float v = row16_sum(acc[r][m]);
            if ((tid & 15) == 0) red[grp][r * MB + m] = v;
        }
    if constexpr (NORM) {
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            const float v = row16_sum(ss[m]);
            if ((tid & 15) == 0) red_ss[grp][m] = v;
        }
    }
    __syncthreads();
    if (tid < rs * R * MB) {
        const int st = tid / (R * MB), j = tid % (R * MB);
        float t = 0.f, rinv = 1.f;
        for (int w = 0; w < gpt; ++w) t += red[st * gpt + w][j];
        if constexpr (NORM) {
            float q = 0.f;
            for (int w = 0; w < gpt; ++w) q += red_ss[st * gpt + w][j % MB];
            rinv = rsqrtf(q / (float)a.K + a.eps);
        }
        fin[tid] = t * rinv;
    }
    __syncthreads();
    if constexpr (EPI == EPI_SWIGLU) {
        if (tid < rs * (R / 2) * MB) {
            const int st = tid / ((R / 2) * MB), jj = tid % ((R / 2) * MB);
            const int j = jj / MB, m = jj % MB;
            const int n = (blockIdx.x * rs + st) * R + 2 * j;
            if (m < a.M && n + 1 < a.N) {
                const float* f = fin + st * R * MB;
                const float gt = bfround(f[(2 * j) * MB + m] + (a.bias ? bf2f(a.bias[n]) : 0.f));
                const float up = bfround(f[(2 * j + 1) * MB + m] + (a.bias ? bf2f(a.bias[n + 1]) : 0.f));
                a.out[(size_t)m * a.ldo + (n >> 1)] = f2bf(bfround(silu(gt)) * up);
            }
        }
    } else {
        if (tid < rs * R * MB) {
            const int st = tid / (R * MB), jj = tid % (R * MB);
            const int r = jj / MB, m = jj % MB;
            const int n = (blockIdx.x * rs + st) * R + r;
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

template <int R, int MB>
int launch_fp4(const GemvArgs& a, const GemvPlan& p, hipStream_t s) {
    const dim3 grid(p.grid), block(p.block);
    const bool norm = a.norm_w != nullptr;
    const int tpr = p.tpr, rs = p.row_sets;
#define EMU_FP4_CASE(E)                                                                                              \
    case E:                                                                                                          \
        if (norm) hipLaunchKernelGGL((gemv_fp4_kernel<R, MB, true, E>), grid, block, 0, s, a, tpr, rs);              \
        else hipLaunchKernelGGL((gemv_fp4_kernel<R, MB, false, E>), grid, block, 0, s, a, tpr, rs);                  \
        break;
    switch (a.epi) {
        EMU_FP4_CASE(EPI_NONE)
        EMU_FP4_CASE(EPI_RESID)
        EMU_FP4_CASE(EPI_SWIGLU)
        default: return -22;
    }
#undef EMU_FP4_CASE
    EMU_CHECK_LAUNCH();
    return 0;
}

// one thread per MX block: 64 bytes of bf16 in, 16 element bytes + 1 scale byte out (mxfp4.quantize_rows' arithmetic, bit for bit)
__global__ __launch_bounds__(256) void quant_mxfp4_kernel(const bf16_t* w, int ldw, uint8_t* q, int ldq, uint8_t* sc, int lds, int N,
                                                          int KB, int* bad) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)N * KB) return;
    const int n = (int)(idx / KB), kb = (int)(idx % KB);
    const bf16_t* src = w + (size_t)n * ldw + kb * 32;
    u32x4 v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = ld16(src + c * 8);
    uint32_t amax = 0;                             // |bf16| patterns order like the values
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const uint32_t lo = v[c][d] & 0x7fffu, hi = (v[c][d] >> 16) & 0x7fffu;
            amax = amax > lo ? amax : lo;
            amax = amax > hi ? amax : hi;
        }
    const int E = (int)(amax >> 7);                // biased exponent of amax
    if (E == 255) { atomicOr(bad, 1); return; }    // inf / nan: the call answers -22
    // e = floor(log2(amax)) - 2 clamped to [-126, 125]; a denormal amax lies below 2^-126, so it clamps like E = 0 would
    int e = E - 127 - 2;
    e = e < -126 ? -126 : e;
    if (amax == 0) e = 0;
    const float inv = __uint_as_float((uint32_t)(127 - e) << 23);     // 2^-e, exponent field 2 .. 253
    u32x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float f[8];
        unpack8(v[c], f);
        uint32_t pk = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float t = fabsf(f[j] * inv);     // exact: a power-of-two factor
            // nearest grid point, ties to the even code
            uint32_t code = (uint32_t)(t > 0.25f) + (uint32_t)(t >= 0.75f) + (uint32_t)(t > 1.25f) + (uint32_t)(t >= 1.75f) +
                            (uint32_t)(t > 2.5f) + (uint32_t)(t >= 3.5f) + (uint32_t)(t > 5.0f);
            code |= (__float_as_uint(f[j]) >> 31) << 3;
            pk |= code << (4 * j);
        }
        o[c] = pk;
    }
    st16(q + (size_t)n * ldq + kb * 16, o);
    sc[(size_t)n * lds + kb] = (uint8_t)(e + 127);
}

int gcd_int(int x, int y) { while (y) { const int t = x % y; x = y; y = t; } return x; }

}  // namespace

// threads per row set (a multiple of 16) and row sets per workgroup for rows of KB blocks: the trip count, among the four smallest
// that keep a row set within 256 threads, that leaves the fewest idle lanes; then as many row sets as make whole waves and at least
// four of them
void plan_fp4(int KB, int* tpr_out, int* rs_out) {
    const int g = (KB + 15) / 16;
    const int t0 = (g + 15) / 16;
    int best_gpt = 0, best_waste = 1 << 30;
    for (int trips = t0; trips < t0 + 4; ++trips) {
        const int gpt = (g + trips - 1) / trips;
        const int waste = trips * gpt * 16 - KB;
        if (waste < best_waste) { best_waste = waste; best_gpt = gpt; }
    }
    const int tpr = best_gpt * 16;
    int rs = 64 / gcd_int(tpr, 64);
    while (rs * tpr < 256) rs *= 2;
    *tpr_out = tpr; *rs_out = rs;
}

// (weight rows per lane, built activation rows) of a plan of this family (gemv.hip::plan_fp4_rows)
int launch_gemv_fp4(const GemvArgs& a, const GemvPlan& p, hipStream_t s) {
    if (p.mb == 2) return p.rpl == 4 ? launch_fp4<4, 2>(a, p, s) : -22;
    return p.rpl == 4 ? launch_fp4<4, 1>(a, p, s) : p.rpl == 8 ? launch_fp4<8, 1>(a, p, s) : -22;
}

int launch_quant_mxfp4_rows(const bf16_t* w, int ldw, uint8_t* q, int ldq, uint8_t* scales, int lds, int N, int K, hipStream_t s) {
    if (N < 1 || K < 32 || (K & 31) || (ldw & 7) || (ldq & 15) || ldw < K || ldq < K / 2 || lds < K / 32) return -22;
    int* bad = nullptr;
    if (hipMalloc(&bad, sizeof(int)) != hipSuccess) return -12;
    int st = 0, host = 0;
    if (hipMemsetAsync(bad, 0, sizeof(int), s) != hipSuccess) st = -5;
    if (!st) {
        const int KB = K >> 5;
        const long blocks = ((long)N * KB + 255) / 256;
        hipLaunchKernelGGL(quant_mxfp4_kernel, dim3((unsigned)blocks), dim3(256), 0, s, w, ldw, q, ldq, scales, lds, N, KB, bad);
        if (hipGetLastError() != hipSuccess) st = -5;
    }
    // non-finite weights are an error of the call, so it waits for its own result (an offline operation, never part of a decode step)
    if (!st && (hipMemcpyAsync(&host, bad, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)) st = -5;
    (void)hipFree(bad);
    return st ? st : (host ? -22 : 0);
}
