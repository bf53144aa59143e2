// One-row decode weight streams over the 13-bit and 12-bit lossless bf16 formats (bf16_pack.h; BITS picks the format, the 13-bit
// instantiations are what they were before the 12-bit ones came): the packed twins of the bf16 forms the headline decode step runs
// (gemv.hip):
//   head form, fused RMSNorm      gemv_kernel<4, 1, true, EPI, -1>       qkv, gate/up (SwiGLU), lm_head
//   preload form                  gemv_kernel<2, 1, false, EPI, 4>       o_proj
//   single round trip             gemv_rt_kernel<2, 9, false, EPI, false> down_proj
// Same rows per workgroup (the head form: two of the bf16 kernel's 4-row groups, so half as many workgroups normalise x), same
// column-to-thread partition, same order of the v_dot2c chain, same wave / LDS reductions, same epilogue rounding points: only the
// fetch and the in-register decode in front of bf16_dot2 differ, so the outputs are the bf16 kernels' bit for bit.  13/16 of the HBM bytes.  A workgroup whose row group is flagged (a weight outside the matrix's 32-binade window) streams the
// bf16 rows through the same registers instead; the branch is workgroup-uniform.  The packed loads of the first trip / the preload
// are requested before the flag word is back, so the flag costs an unflagged workgroup no latency.  No workgroup waits for another.
// 12 bits: no sign load; the row group's patch record (8 slots, requested at kernel start with the flag word) is applied to the decoded
// dwords in front of the unchanged bf16_dot2 chain, behind a workgroup-uniform test per trip and row pair; 12/16 of the HBM bytes.
#include "common.h"
#include "kernels.h"
#include "bf16_pack.h"

namespace {

// the registers of one fetch: R 16-byte bf16 vectors, or (packed) R/2 low units, R nibble dwords, the sign bytes
template <int R>
struct PackRaw { uint32_t d[4 * R]; };

template <int R>
struct PackPtrs {
    const u32x4* lo; const uint32_t* nib; const uint8_t* sign;      // at the row group
    const bf16_t* wrow[R];                                           // the bf16 rows (tail rows clamped)
    int KV;
    uint32_t hb4;
};

template <int R>
__device__ __forceinline__ PackPtrs<R> pack_ptrs(const GemvArgs& a, const PackSet& p, int g) {
    PackPtrs<R> q;
    q.KV = a.K >> 3;
    q.lo = reinterpret_cast<const u32x4*>(p.lo) + (size_t)g * (R / 2) * q.KV;
    q.nib = reinterpret_cast<const uint32_t*>(p.nib) + (size_t)g * q.KV * R;
    q.sign = reinterpret_cast<const uint8_t*>(p.sign) + (size_t)g * q.KV * R;
    q.hb4 = (uint32_t)p.hb * 0x01010101u;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int n = g * R + r;
        n = n < a.N ? n : a.N - 1;
        q.wrow[r] = a.W + (size_t)n * a.ldw;
    }
    return q;
}

// BITS: 13, or 12 (no sign load: the sign is in the nibble)
template <int R, int BITS = 13>
__device__ __forceinline__ void fetch_packed(const PackPtrs<R>& q, int vi, PackRaw<R>& w) {
#pragma unroll
    for (int h = 0; h < R / 2; ++h) {
        const u32x4 v = ld_stream(q.lo + (size_t)h * q.KV + vi);
        w.d[4 * h] = v.x; w.d[4 * h + 1] = v.y; w.d[4 * h + 2] = v.z; w.d[4 * h + 3] = v.w;
    }
    if constexpr (R == 4) {
        const u32x4 n = ld_stream(reinterpret_cast<const u32x4*>(q.nib) + vi);
        w.d[8] = n.x; w.d[9] = n.y; w.d[10] = n.z; w.d[11] = n.w;
        if constexpr (BITS == 13) w.d[12] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(q.sign) + vi);
    } else {
        const u32x2 n = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(q.nib) + vi);
        w.d[4] = n.x; w.d[5] = n.y;
        if constexpr (BITS == 13) w.d[6] = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(q.sign) + vi);
    }
}
// the 12-bit fetch of the single round trip (R = 2): buffer loads whose range is the row group's KV vectors, so a load past the row
// returns zeros by itself -- no branch around the load and no zero-initialised registers for it to merge with (with those the
// compiler waits for each trip's load before it requests the next)
__device__ __forceinline__ void fetch_packed12_ranged(const PackPtrs<2>& q, int vi, PackRaw<2>& w) {
    const __amdgpu_buffer_rsrc_t rl = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(q.lo), 0, (uint32_t)q.KV * 16u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rn = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(q.nib), 0, (uint32_t)q.KV * 8u, 0x00020000);
    const u32x4 v = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rl, (uint32_t)vi * 16u, 0, 2));      // (aux 2: nt)
    const u32x2 n = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rn, (uint32_t)vi * 8u, 0, 2));
    w.d[0] = v.x; w.d[1] = v.y; w.d[2] = v.z; w.d[3] = v.w;
    w.d[4] = n.x; w.d[5] = n.y;
}
template <int R>
__device__ __forceinline__ void fetch_bf16(const PackPtrs<R>& q, int vi, PackRaw<R>& w) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const u32x4 v = ld_stream(reinterpret_cast<const u32x4*>(q.wrow[r] + vi * 8));
        w.d[4 * r] = v.x; w.d[4 * r + 1] = v.y; w.d[4 * r + 2] = v.z; w.d[4 * r + 3] = v.w;
    }
}
// what a 12-bit stream carries beside its planes: the row group's patch record (nothing at 13 bits)
template <int BITS> struct PackPatch {};
template <> struct PackPatch<12> { Pack12Rec rec; };
template <int BITS>
__device__ __forceinline__ PackPatch<BITS> pack_patch(const PackSet& p, int g, int lane) {
    if constexpr (BITS == 12) return {pack12_record(p.patch, g, lane)};
    else return {};
}
// acc[r] += row r . xp, the bf16 kernels' chain: x, y, z, w of the row's vector in order (12 bits: the patches of trip `trip` first).
// 12 bits: called by EVERY lane of the wave, `active` = this lane holds a vector of the trip.  The record sits in lanes 0..7 and the
// patch test is a ballot, which sees active lanes only, so the decode and the patches run with the whole wave (the last wave of a
// ragged trip may hold 4 vectors: lanes 4..7 must still show their slots) and only the sums are the active lanes'; the packed
// registers of an inactive lane must be loaded (a clamped vector) all the same.  A wave with no active lane skips everything.
template <int R, int BITS = 13>
__device__ __forceinline__ void pack_dots(const PackPtrs<R>& q, bool flagged, const PackRaw<R>& w, const u32x4& xp, float (&acc)[R],
                                          const PackPatch<BITS>& pp = {}, int trip = 0, int tid = 0, bool active = true) {
    if constexpr (BITS == 12) {
        if (!__builtin_amdgcn_ballot_w64(active)) return;
        // two rows at a time: decoded, patched behind one uniform test, summed -- straight-line code but for that test.  The empty
        // asm pins each sum where it is made: without it the compiler sinks the chains of a whole trip below the next fetch and
        // keeps every decoded dword alive across it (the head form then needs 147 VGPRs: 3 waves per SIMD).
#pragma unroll
        for (int h = 0; h < R / 2; ++h) {
            uint32_t v[2][4];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int r = 2 * h + i;
                if (flagged) { v[i][0] = w.d[4 * r]; v[i][1] = w.d[4 * r + 1]; v[i][2] = w.d[4 * r + 2]; v[i][3] = w.d[4 * r + 3]; }
                else pack12_decode_row(w.d[2 * r], w.d[2 * r + 1], w.d[2 * R + r], q.hb4, v[i]);
            }
            if (!flagged) pack12_patch(pp.rec, trip, h, tid, v);
            if (!active) continue;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float t = acc[2 * h + i];
                t = bf16_dot2(v[i][0], xp.x, t);
                t = bf16_dot2(v[i][1], xp.y, t);
                t = bf16_dot2(v[i][2], xp.z, t);
                t = bf16_dot2(v[i][3], xp.w, t);
                asm volatile("" : "+v"(t));
                acc[2 * h + i] = t;
            }
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        uint32_t v[4];
        if (flagged) {
            v[0] = w.d[4 * r]; v[1] = w.d[4 * r + 1]; v[2] = w.d[4 * r + 2]; v[3] = w.d[4 * r + 3];
        } else {
            pack_decode_row<R>(w.d[2 * r], w.d[2 * r + 1], w.d[2 * R + r], w.d[3 * R], r, q.hb4, v);
        }
        float t = acc[r];
        t = bf16_dot2(v[0], xp.x, t);
        t = bf16_dot2(v[1], xp.y, t);
        t = bf16_dot2(v[2], xp.z, t);
        t = bf16_dot2(v[3], xp.w, t);
        acc[r] = t;
    }
}

// the one-row epilogue of gemv_kernel / gemv_rt_kernel (M == 1): fin[r] = the fp32 sums of the workgroup's rows
template <int R, int EPI>
__device__ __forceinline__ void pack_epilogue(const GemvArgs& a, const float* fin, int n0, int tid) {
    if constexpr (EPI == EPI_SWIGLU) {
        if (tid < R / 2) {
            const int n = n0 + 2 * tid;
            if (n + 1 < a.N) {
                const float gt = bfround(fin[2 * tid] + (a.bias ? bf2f(a.bias[n]) : 0.f));
                const float up = bfround(fin[2 * tid + 1] + (a.bias ? bf2f(a.bias[n + 1]) : 0.f));
                const float act = bfround(silu(gt));
                a.out[n >> 1] = f2bf(act * up);
            }
        }
    } else {
        if (tid < R) {
            const int n = n0 + tid;
            if (n < a.N) {
                float v = fin[tid];
                if (a.bias) v += bf2f(a.bias[n]);
                v = bfround(v);
                if constexpr (EPI == EPI_RESID) v = v + bf2f(a.res[n]);
                a.out[n] = f2bf(v);
            }
        }
    }
}

template <int R>
__device__ __forceinline__ void pack_reduce(float (&acc)[R], float (*red)[R], float* fin, int tid) {
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float v = wave_sum(acc[r]);
        if (lane == 0) red[wave][r] = v;
    }
    __syncthreads();
    if (tid < R) fin[tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    __syncthreads();
}

// ---- head form (gemv_kernel<4, 1, true, EPI, -1>): x, the gain and the first trip are requested before the RMSNorm statistics are
// reduced through a raw s_barrier; trips 1..3 stream behind it through two register sets.  A workgroup owns G adjacent 4-row groups
// of the R = 4 set (groups G b .. G b + G - 1): the column-to-thread partition, every row's v_dot2c chain over trips 0..3, the wave and
// 4-wave reductions and the epilogue rounding points are the 4-row kernel's, only the number of rows that share one normalisation of
// x differs, so the outputs stay the bf16 kernel's bits.  A group past the last one (an odd group count) is clamped to the last group
// for every load and its rows fail the epilogue's n < N.  G = 2: a workgroup with a flagged group streams the bf16 rows of all 8, one
// trip at a time through the registers of both sets (8 rows x 4 dwords do not fit one); rare, it only has to be exact.
template <int EPI, int G, int BITS>
__global__ __launch_bounds__(256) void gemv_pack_head_kernel(const GemvArgs a, const PackSet p, const int groups) {
    constexpr int R = 4;
    __shared__ float red[4][R * G];
    __shared__ float fin[R * G];
    __shared__ float ssp[4];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int KV = a.K >> 3;
    const int n0 = blockIdx.x * R * G;
    const int g0 = blockIdx.x * G;                                     // (G = 2: g0 is even, so both groups' flags share a word)
    const uint32_t fw = p.flags[g0 >> 5];
    PackPtrs<R> q[G];
#pragma unroll
    for (int j = 0; j < G; ++j) q[j] = pack_ptrs<R>(a, p, g0 + j < groups ? g0 + j : groups - 1);
    PackPatch<BITS> pp[G];
#pragma unroll
    for (int j = 0; j < G; ++j) pp[j] = pack_patch<BITS>(p, g0 + j < groups ? g0 + j : groups - 1, lane);

    u32x4 hx[4], hg[4];
    PackRaw<R> hw[G], w1[G];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int vi = tid + 256 * c;
        const int vc = vi < KV ? vi : KV - 1;
        hx[c] = vi < KV ? ld16(a.x + vi * 8) : u32x4{0u, 0u, 0u, 0u};
        hg[c] = ld16(a.norm_w + vc * 8);
    }
    const int v0 = tid < KV ? tid : KV - 1;                            // short rows (K < 2048): clamped, against a zero operand
#pragma unroll
    for (int j = 0; j < G; ++j) fetch_packed<R, BITS>(q[j], v0, hw[j]);
    bool flagged = false;
#pragma unroll
    for (int j = 0; j < G; ++j) flagged = flagged || (g0 + j < groups && ((fw >> ((g0 + j) & 31)) & 1u));
    if (flagged) {
#pragma unroll
        for (int j = 0; j < G; ++j) fetch_bf16<R>(q[j], v0, hw[j]);
    }
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
    const float rinv = rsqrtf((sp[0] + sp[1] + sp[2] + sp[3]) / (float)a.K + a.eps);
#pragma unroll
    for (int c = 0; c < 4; ++c) {                                      // hx <- bf16(g * bf16(x * rinv)), the dot2 operand
        float xf[8], g[8];
        unpack8(hx[c], xf);
        unpack8(hg[c], g);
#pragma unroll
        for (int j = 0; j < 8; ++j) xf[j] = g[j] * bfround(xf[j] * rinv);
        hx[c] = pack8(xf);
    }

    float acc[G][R];
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[j][r] = 0.f;
    auto dots = [&](bool fl, const PackRaw<R> (&w)[G], const u32x4& xp, int trip, bool active = true) {
#pragma unroll
        for (int j = 0; j < G; ++j) pack_dots<R, BITS>(q[j], fl, w[j], xp, acc[j], pp[j], trip, tid, active);
    };
    if (flagged) {
        dots(true, hw, hx[0], 0);
#pragma unroll
        for (int c = 1; c < 4; ++c) {
            const int vi = tid + 256 * c;
            if (vi < KV) {
#pragma unroll
                for (int j = 0; j < G; ++j) fetch_bf16<R>(q[j], vi, hw[j]);
                dots(true, hw, hx[c], c);
            }
        }
    } else {
        // (12 bits: a wave that holds any vector of the trip fetches with all its lanes, the lanes past the row a clamped vector,
        // and every lane calls dots -- pack_dots says why)
        auto fetch = [&](PackRaw<R> (&w)[G], int c) {
            const int vi = tid + 256 * c;
            if (BITS == 12 ? __builtin_amdgcn_ballot_w64(vi < KV) != 0 : vi < KV) {
#pragma unroll
                for (int j = 0; j < G; ++j) fetch_packed<R, BITS>(q[j], BITS == 12 && vi >= KV ? KV - 1 : vi, w[j]);
            }
        };
        fetch(w1, 1);
        dots(false, hw, hx[0], 0);
        __builtin_amdgcn_sched_barrier(0);
        fetch(hw, 2);
        if constexpr (BITS == 12) dots(false, w1, hx[1], 1, tid + 256 < KV);
        else if (tid + 256 < KV) dots(false, w1, hx[1], 1);
        __builtin_amdgcn_sched_barrier(0);
        fetch(w1, 3);
        if constexpr (BITS == 12) {
            dots(false, hw, hx[2], 2, tid + 512 < KV);
            dots(false, w1, hx[3], 3, tid + 768 < KV);
        } else {
            if (tid + 512 < KV) dots(false, hw, hx[2], 2);
            if (tid + 768 < KV) dots(false, w1, hx[3], 3);
        }
    }

    float accf[R * G];
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
        for (int r = 0; r < R; ++r) accf[j * R + r] = acc[j][r];
    pack_reduce<R * G>(accf, red, fin, tid);
    pack_epilogue<R * G, EPI>(a, fin, n0, tid);
}

// ---- the two plain forms of two rows per workgroup, every load requested up front.  CLAMP: the preload form (gemv_kernel<2, 1, false,
// EPI, 4>: loads past the row clamped, their trips skipped); else the single round trip (gemv_rt_kernel<2, 9, false, EPI, false>:
// loads past the row not issued, zero registers against a zero activation)
template <int KIT, bool CLAMP, int EPI, int BITS>
__global__ __launch_bounds__(256) void gemv_pack_rows2_kernel(const GemvArgs a, const PackSet p) {
    constexpr int R = 2;
    __shared__ float red[4][R];
    __shared__ float fin[R];
    const int tid = threadIdx.x;
    const int KV = a.K >> 3;
    const int n0 = blockIdx.x * R;
    const uint32_t fw = p.flags[blockIdx.x >> 5];
    const PackPtrs<R> q = pack_ptrs<R>(a, p, blockIdx.x);
    const PackPatch<BITS> pp = pack_patch<BITS>(p, blockIdx.x, tid & 63);

    u32x4 xv[KIT];
    PackRaw<R> wv[KIT];
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
        const int vi = tid + 256 * it;
        xv[it] = vi < KV ? ld16(a.x + vi * 8) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
        const int vi = tid + 256 * it;
        if constexpr (CLAMP) {
            fetch_packed<R, BITS>(q, vi < KV ? vi : KV - 1, wv[it]);
        } else if constexpr (BITS == 12) {
            fetch_packed12_ranged(q, vi, wv[it]);
            __builtin_amdgcn_sched_barrier(0);                       // trip by trip, so the first trip's planes are back first
        } else {
#pragma unroll
            for (int d = 0; d < 4 * R; ++d) wv[it].d[d] = 0u;
            if (vi < KV) fetch_packed<R, BITS>(q, vi, wv[it]);
        }
    }
    const bool flagged = (fw >> (blockIdx.x & 31)) & 1u;
    if (flagged) {
#pragma unroll
        for (int it = 0; it < KIT; ++it) {
            const int vi = tid + 256 * it;
            if constexpr (CLAMP) {
                fetch_bf16<R>(q, vi < KV ? vi : KV - 1, wv[it]);
            } else {
#pragma unroll
                for (int d = 0; d < 4 * R; ++d) wv[it].d[d] = 0u;
                if (vi < KV) fetch_bf16<R>(q, vi, wv[it]);
            }
        }
    }

    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    if constexpr (BITS == 12) {          // two copies of the chain, so no register of the packed fetch waits to merge with the bf16 one
        auto dots = [&](bool fl) {
#pragma unroll
            for (int it = 0; it < KIT; ++it) {
                pack_dots<R, BITS>(q, fl, wv[it], xv[it], acc, pp, it, tid, !CLAMP || tid + 256 * it < KV);       // (every lane calls)
            }
        };
        if (flagged) dots(true); else dots(false);
    } else {
#pragma unroll
        for (int it = 0; it < KIT; ++it) {
            if (!CLAMP || tid + 256 * it < KV) pack_dots<R>(q, flagged, wv[it], xv[it], acc);
        }
    }

    pack_reduce<R>(acc, red, fin, tid);
    pack_epilogue<R, EPI>(a, fin, n0, tid);
}

}  // namespace

// the forms the packed stream has a twin for, from the bf16 plan of the shape: rows per workgroup (the set's R), or 0
int gemv_pack_rows(const GemvPlan& p, const GemvShape& sh) {
    if (p.status || sh.M != 1 || sh.fp8 || sh.fp4 || (sh.K & 31) || sh.K < 32) return 0;
    if (sh.epi != EPI_NONE && sh.epi != EPI_RESID && sh.epi != EPI_SWIGLU) return 0;
    if (p.family == GEMV_FAM_BLOCK && p.form == GEMV_FORM_HEAD && p.rows == 4 && p.mb == 1 && sh.norm && sh.epi != EPI_RESID) return 4;
    if (p.family == GEMV_FAM_BLOCK && p.form == GEMV_FORM_PRELOAD && p.rows == 2 && p.mb == 1 && !sh.norm && sh.epi != EPI_SWIGLU) return 2;
    if (p.family == GEMV_FAM_RT && p.rows == 2 && p.trips == 9 && !sh.norm && sh.epi != EPI_SWIGLU) return 2;
    return 0;
}

// the twin of the set's format: p.patch set = the 12-bit set (no sign plane), else the 13-bit one.  Which kinds have a 12-bit twin is
// what profiles/bf16_pack12.md measured faster than the 13-bit one; a 12-bit set of another form is refused.
int launch_gemv_pack(const GemvArgs& a, const PackSet& p, int form, hipStream_t s) {
    const bool b12 = p.patch != nullptr;
    if (!a.x || !a.W || !a.out || !p.lo || !p.nib || (!b12 && !p.sign) || !p.flags || a.M != 1 || a.N < 1 || a.K < 32 || (a.K & 31)) return -22;
    if (a.ldw < a.K || (a.ldw & 7) || p.hb < 0 || p.hb > (b12 ? 120 : 112) || (a.epi == EPI_RESID && !a.res)) return -22;
    const int KV = a.K >> 3;
#define EMU_PACK_LAUNCH(KERNEL, R)                                                                                   \
    hipLaunchKernelGGL(KERNEL, dim3((a.N + R - 1) / R), dim3(256), 0, s, a, p);                                      \
    EMU_CHECK_LAUNCH();                                                                                              \
    return 0;
#define EMU_PACK_ROWS2(KIT, CLAMP, EPI)                                                                              \
    if (b12) { EMU_PACK_LAUNCH((gemv_pack_rows2_kernel<KIT, CLAMP, EPI, 12>), 2) }                                   \
    EMU_PACK_LAUNCH((gemv_pack_rows2_kernel<KIT, CLAMP, EPI, 13>), 2)
    if (form == GEMV_FORM_HEAD) {
        if (p.rows != 4 || !a.norm_w || KV > 1024) return -22;
        if (a.epi != EPI_NONE && (a.epi != EPI_SWIGLU || (a.N & 1))) return -22;
        const int groups = (int)pack_groups(a.N, 4);                 // two groups (8 rows) per workgroup
#define EMU_PACK_HEAD(EPI, BITS)                                                                                     \
    hipLaunchKernelGGL((gemv_pack_head_kernel<EPI, 2, BITS>), dim3((groups + 1) / 2), dim3(256), 0, s, a, p, groups); \
    EMU_CHECK_LAUNCH();                                                                                              \
    return 0;
        if (a.epi == EPI_NONE) { if (b12) { EMU_PACK_HEAD(EPI_NONE, 12) } EMU_PACK_HEAD(EPI_NONE, 13) }
        if (b12) { EMU_PACK_HEAD(EPI_SWIGLU, 12) }
        EMU_PACK_HEAD(EPI_SWIGLU, 13)
#undef EMU_PACK_HEAD
    }
    if (p.rows != 2 || a.norm_w) return -22;
    if (form == GEMV_FORM_PRELOAD) {
        if (KV > 1024) return -22;
        if (a.epi == EPI_NONE) { EMU_PACK_ROWS2(4, true, EPI_NONE) }
        if (a.epi == EPI_RESID) { EMU_PACK_ROWS2(4, true, EPI_RESID) }
        return -22;
    }
    if (form == GEMV_FORM_RT) {
        if (KV > 9 * 256) return -22;
        if (a.epi == EPI_NONE) { EMU_PACK_ROWS2(9, false, EPI_NONE) }
        if (a.epi == EPI_RESID) { EMU_PACK_ROWS2(9, false, EPI_RESID) }
        return -22;
    }
#undef EMU_PACK_ROWS2
#undef EMU_PACK_LAUNCH
    return -22;
}
