// Two-segment flash attention (gfx950, D = 128): many rows of few queries behind ONE shared prefix of keys.
//
//  flash_prefix : o = softmax over [prefix keys kstart .. P) ++ [own keys j <= i + (Sk - Sq)] for query i of row b.  The prefix
//                 K [H, P, D] / Vt [H, D, P_pad] is common to all B rows; every row has its own K [B, H, Sk, D] / Vt [B, H, D, Sk_pad]
//                 (the few slots a candidate continuation wrote itself).  One online softmax over both segments, fp32, bf16 out.
//
// The tile arithmetic is flash_kernel<128, 4>'s (attention.hip), statement for statement: 64-key tiles, v_mfma_f32_32x32x16_bf16 with
// swapped operands (S^T = K Q^T, O^T = Vt P^T), the exp2-domain softmax in the same operation order, -inf masking, dead rows.  The
// prefix tiles 0 .. ceil(P / 64) are walked first, then the own tiles, each masked by the key's index WITHIN its segment.  With P a
// multiple of 64 these are exactly the tiles flash_kernel walks over the concatenated keys, and the two agree bit for bit.
//
// Mapping.  The workload is B rows (candidates) x H heads x ceil(Sq / 32) blocks of 32 queries, Sq typically 1..32, P in the hundreds.
// A unit is one (row, 32-query block) of a head and belongs to ONE wave.  A workgroup of four waves takes four consecutive units of
// one head:
//   * the prefix tiles are staged through LDS once per workgroup and feed all four waves (four rows share every staged tile; the
//     staging and its two barriers per tile are flash_kernel's);
//   * the own tiles differ per wave, are one or two per unit, and are read by each wave straight from global memory into its MFMA
//     fragments (16-byte loads of the very bytes the LDS path would deliver): no barrier, waves with fewer own tiles just finish;
//   * workgroups are dealt so that an XCD owns a run of consecutive (head, unit group) pairs -- whole heads where the counts allow --
//     as flash_kernel's xcd_remap does: all candidates of a head find the prefix tiles in one XCD's L2, which fetches them once.
// A query's result depends on nothing but its own tile sequence (rescales by alpha = 1 and tiles wholly masked for a query leave its
// state untouched), so it does not depend on which wave, workgroup or neighbours it was given.  Waves past the last unit recompute the
// last unit (the barriers stay uniform) and store nothing.
//
// Replaces: the candidate loop of Emu1/models/prediction_mixin.py:36-131 (prompt + candidate through the model once per candidate).
#include "common.h"
#include "kernels.h"

namespace {

__device__ __forceinline__ int sw_off256(int row, int chunk) { return row * 256 + ((chunk ^ (row & 15)) << 4); }
__device__ __forceinline__ int sw_off128(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

__global__ __launch_bounds__(256, 2) void flash_prefix_kernel(const FlashPrefixArgs a) {
    constexpr int D = 128, THREADS = 256;
    constexpr int KCH = D / 8;                        // 16-byte chunks per K row
    constexpr int NKK = D / 16;                       // k-steps of QK^T
    constexpr int NDB = D / 32;                       // 32-wide d blocks of O
    constexpr int KT_BYTES = 64 * D * 2;              // K tile [64 keys][D]
    constexpr int VT_BYTES = D * 128;                 // Vt tile [D][64 keys]
    constexpr int NLD = (KT_BYTES / 16) / THREADS;    // 16-byte chunks per thread per tile
    __shared__ __attribute__((aligned(16))) char smem[KT_BYTES + VT_BYTES];
    char* sK = smem;
    char* sV = smem + KT_BYTES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    // workgroup -> (head, group of four units); blocks of equal blockIdx % 8 share an XCD (observed dispatch order, as in flash_kernel:
    // a matter of speed only): each such group owns a run of consecutive pairs
    const int nq = (a.Sq + 31) / 32, units = nq * a.B, groups = (units + 3) / 4, total = groups * a.H;
    int lin = blockIdx.x;
    {
        const int xcd = lin & 7, q8 = total >> 3, r8 = total & 7;
        lin = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (lin >> 3);
    }
    const int h = lin / groups, g = lin - h * groups;
    int unit = g * 4 + wave;
    const bool live = unit < units;
    unit = live ? unit : units - 1;
    const int b = unit / nq, q0 = (unit - b * nq) * 32;
    const int off = a.Sk - a.Sq;                      // own segment, causal: query i sees own keys <= i + off
    const int kstart = a.kstart_dev ? a.kstart_dev[0] : a.kstart;

    // Q fragments (B operand): column = query l31, k = 16*kk + 8*hi + j
    const int qi = q0 + l31;
    const int qrow = qi < a.Sq ? qi : a.Sq - 1;
    const bf16_t* qp = a.q + (size_t)b * a.q_sb + (size_t)h * a.q_sh + (size_t)qrow * a.q_ss + 8 * hi;
    bf16x8_t qf[NKK];
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) qf[kk] = *reinterpret_cast<const bf16x8_t*>(qp + 16 * kk);

    const bf16_t* kpbase = a.kp + (size_t)h * a.kp_sh;
    const bf16_t* vpbase = a.vtp + ((size_t)h * D) * a.P_pad;
    const bf16_t* kobase = a.ko + (size_t)b * a.ko_sb + (size_t)h * a.ko_sh;
    const bf16_t* vobase = a.vto + ((size_t)(b * a.H + h) * D) * a.Sk_pad;

    const int ntile_p = (a.P + 63) / 64;
    int qmax = q0 + 31; qmax = qmax < a.Sq ? qmax : a.Sq - 1;
    const int last_own = qmax + off < a.Sk - 1 ? qmax + off : a.Sk - 1;      // >= 0: Sk >= Sq >= 1
    const int ntile_o = last_own / 64 + 1;

    u32x4 rk[NLD], rv[NLD];
    auto gload = [&](int t) {
        const int kt0 = t * 64;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int q = tid + THREADS * i;
            { const int row = q / KCH, c = q % KCH;
              int key = kt0 + row; key = key < a.P ? key : a.P - 1;
              rk[i] = ld16(kpbase + (size_t)key * a.kp_ss + c * 8); }
            { const int row = q >> 3, c = q & 7;
              rv[i] = ld16(vpbase + (size_t)row * a.P_pad + kt0 + c * 8); }
        }
    };
    auto sstore = [&]() {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int q = tid + THREADS * i;
            st16(sK + sw_off256(q / KCH, q % KCH), rk[i]);
            st16(sV + sw_off128(q >> 3, q & 7), rv[i]);
        }
    };

    f32x16_t o[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const float sc = a.scale * 1.4426950408889634f;   // softmax in the exp2 domain

    // MFMA row i of the K operand holds key pi(i) = i with bits 2 and 3 swapped
    const int krow = (l31 & 0x13) | ((l31 & 4) << 1) | ((l31 & 8) >> 1);

    // One 64-key tile of a segment of `len` keys of which this lane's query sees [lo, hi_key]: flash_kernel's tile body.  kfrag(blk, kk)
    // and vfrag(db, ks) deliver the operand fragments (from LDS for the prefix, from global memory for the own keys).
    auto tile = [&](int kt0, int len, int lo, int hi_key, int hi_wave, auto kfrag, auto vfrag) {
        f32x16_t s[2];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[blk][r] = 0.f;
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) s[blk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfrag(blk, kk), qf[kk], s[blk], 0, 0, 0);
        }
        // lane (query qi) holds keys kt0 + 32*blk + 16*(r>>3) + 8*hi + (r&7); interior tiles skip the mask arithmetic (wave-uniform)
        const bool interior = kt0 + 63 < len && kt0 >= lo && kt0 + 63 <= hi_wave;
        float mloc = -INFINITY;
        if (interior) {
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, s[blk][r]);
        } else {
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kt0 + 32 * blk + 16 * (r >> 3) + 8 * hi + (r & 7);
                    const bool ok = key < len && key >= lo && key <= hi_key;
                    const float v = ok ? s[blk][r] : -INFINITY;
                    s[blk][r] = v;
                    mloc = fmaxf(mloc, v);
                }
        }
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64)) * sc;          // sc > 0: the maximum commutes with the scale
        const float mnew = fmaxf(m_run, mloc);
        float alpha = 1.f;
        const bool dead = (mnew == -INFINITY);         // every key so far masked for this query
        if (!dead) alpha = __builtin_amdgcn_exp2f(m_run - mnew);    // m_run = -inf -> 0
        const float nm = dead ? 0.f : -mnew;
        float psum = 0.f;
        u32x4 pfw[4];                                  // P as packed bf16 pairs = the B fragments of the PV MFMAs
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                // masked scores are -inf: fma(-inf, sc, nm) = -inf -> exp2 = 0 (dead rows: nm = 0, still 0)
                const float p0 = __builtin_amdgcn_exp2f(fmaf(s[blk][r], sc, nm));
                const float p1 = __builtin_amdgcn_exp2f(fmaf(s[blk][r + 1], sc, nm));
                psum += p0 + p1;
                pfw[blk * 2 + (r >> 3)][(r & 7) >> 1] = packbf(p0, p1);
            }
        l_run = l_run * alpha + psum;
        m_run = mnew;
        if (__any(alpha != 1.f)) {
#pragma unroll
            for (int db = 0; db < NDB; ++db)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int db = 0; db < NDB; ++db)
                o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfrag(db, ks), __builtin_bit_cast(bf16x8_t, pfw[ks]), o[db], 0, 0, 0);
    };

    // ---- the shared prefix: every key index is below every query's horizon, only the left pad (and the tile's tail) mask
    gload(0);
    for (int t = 0; t < ntile_p; ++t) {
        __syncthreads();                               // previous tile fully consumed
        sstore();
        __syncthreads();
        if (t + 1 < ntile_p) gload(t + 1);             // overlap next tile's latency with the MFMAs
        tile(t * 64, a.P, kstart, 0x7fffffff, 0x7fffffff,
             [&](int blk, int kk) { return *reinterpret_cast<const bf16x8_t*>(sK + sw_off256(blk * 32 + krow, kk * 2 + hi)); },
             [&](int db, int ks) { return *reinterpret_cast<const bf16x8_t*>(sV + sw_off128(db * 32 + l31, ks * 2 + hi)); });
    }
    // ---- the wave's own keys: fragments straight from global memory (rows clamped to the last key, Vt zero padded to Sk_pad)
    for (int t = 0; t < ntile_o; ++t) {
        const int kt0 = t * 64;
        tile(kt0, a.Sk, 0, qi + off, q0 + off,
             [&](int blk, int kk) {
                 int key = kt0 + blk * 32 + krow; key = key < a.Sk ? key : a.Sk - 1;
                 return *reinterpret_cast<const bf16x8_t*>(kobase + (size_t)key * a.ko_ss + (kk * 2 + hi) * 8);
             },
             [&](int db, int ks) {
                 return *reinterpret_cast<const bf16x8_t*>(vobase + (size_t)(db * 32 + l31) * a.Sk_pad + kt0 + (ks * 2 + hi) * 8);
             });
    }

    const float ltot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = ltot > 0.f ? 1.f / ltot : 0.f;
    if (live && qi < a.Sq) {
        bf16_t* op = a.o + (size_t)b * a.o_sb + (size_t)h * a.o_sh + (size_t)qi * a.o_ss;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                u32x2 ov;
                ov.x = packbf(o[db][4 * g4] * inv, o[db][4 * g4 + 1] * inv);
                ov.y = packbf(o[db][4 * g4 + 2] * inv, o[db][4 * g4 + 3] * inv);
                *reinterpret_cast<u32x2*>(op + db * 32 + 8 * g4 + 4 * hi) = ov;
            }
    }
}

}  // namespace

int launch_flash_attn_prefix(const FlashPrefixArgs& a, hipStream_t s) {
    if (a.D != 128 || a.B < 1 || a.H < 1 || a.Sq < 1 || a.P < 1 || a.Sk < a.Sq) return -22;
    if (!a.kstart_dev && (a.kstart < 0 || a.kstart >= a.P)) return -22;
    if ((a.P_pad & 63) || a.P_pad < a.P || (a.Sk_pad & 63) || a.Sk_pad < a.Sk) return -22;
    if (!a.q || !a.kp || !a.vtp || !a.ko || !a.vto || !a.o) return -22;
    if ((a.q_ss & 7) || (a.q_sh & 7) || (a.q_sb & 7) || (a.kp_ss & 7) || (a.kp_sh & 7) || (a.ko_ss & 7) || (a.ko_sh & 7) || (a.ko_sb & 7) ||
        (a.o_ss & 3) || (a.o_sh & 3) || (a.o_sb & 3)) return -22;
    const long units = (long)((a.Sq + 31) / 32) * a.B, total = (units + 3) / 4 * a.H;
    if (total > 0x7fffffffL) return -22;
    const bool prof = emu_prof_on();
    if (prof) emu_prof_begin(s);
    hipLaunchKernelGGL(flash_prefix_kernel, dim3((unsigned)total), dim3(256), 0, s, a);
    if (prof) emu_prof_end(s, "attn_prefix", a.Sq, a.P + a.Sk, a.D, a.B * a.H, 4.0 * a.B * a.H * (double)a.Sq * (a.P + a.Sk) * a.D);
    EMU_CHECK_LAUNCH();
    return 0;
}
