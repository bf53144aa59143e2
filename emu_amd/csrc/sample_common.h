// The machinery of the one-workgroup-per-row logits kernels (sample.hip: the one-beam sampler; beam_sample.hip: the per-beam rows of
// beam-search sampling), written once.  A workgroup of 1024 threads holds one row in LDS as the order-preserving integer image
// ("key") of its fp32 scores: 4 bytes per token of dynamic LDS behind SAMPLE_SCRATCH bytes of reduction scratch, so the vocabulary
// bound is EMU_SAMPLE_MAX_VOCAB = 40 000 (160 000 B + 1 KiB of the CU's 160 KiB).  Thread t owns the contiguous ids [t * C, t * C + C)
// with C = ceil(V / 1024) made odd, so that the 64 lanes of a wave read 64 different banks.
//
// Thresholds without a sort: the top-k value is the largest key t with count{key >= t} >= k', the top-p value the largest key t
// with mass{key < t} <= (1 - top_p) * Z; both are found by a 4-ary search over the 32 key bits (16 levels, three thresholds per
// level, one pass over the row each).  Every sum over the row is blocked: at most SAMPLE_CMAX sequential fp32 adds per thread in
// ascending id order, then a fixed tree (6 levels inside the wave, 4 across the 16 waves) -- no floating-point atomics, so the
// same inputs give the same results on every launch.
#pragma once
#include "common.h"
#include "kernels.h"

namespace {

constexpr int SAMPLE_THREADS = 1024;
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / 64;
constexpr int SAMPLE_CMAX = 41;                                  // ceil(40000 / 1024) = 40, made odd
constexpr int SAMPLE_SCRATCH = 1024;                             // bytes of reduction scratch ahead of the keys

static_assert(SAMPLE_CMAX * SAMPLE_THREADS >= EMU_SAMPLE_MAX_VOCAB && (SAMPLE_CMAX & 1), "chunk bound");
static_assert(SAMPLE_SCRATCH + EMU_SAMPLE_MAX_VOCAB * 4 <= 160 * 1024, "LDS bound");

// fp32 -> uint32, monotone: a < b <=> key(a) < key(b) for all non-NaN a, b (with -0 canonicalised to +0 by the caller)
__device__ __forceinline__ uint32_t f2key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// ---- block reductions over 16 waves: fixed order, every thread gets the result.  scratch: >= 3 * 16 words.
template <int N>
__device__ __forceinline__ void block_sum_f(float* v, float* scratch) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
    for (int m = 0; m < N; ++m) v[m] = wave_sum(v[m]);
    __syncthreads();
    if (l == 0) {
#pragma unroll
        for (int m = 0; m < N; ++m) scratch[m * SAMPLE_WAVES + w] = v[m];
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < N; ++m) {
        float t[SAMPLE_WAVES];
#pragma unroll
        for (int i = 0; i < SAMPLE_WAVES; ++i) t[i] = scratch[m * SAMPLE_WAVES + i];
#pragma unroll
        for (int o = SAMPLE_WAVES / 2; o > 0; o >>= 1)
#pragma unroll
            for (int i = 0; i < o; ++i) t[i] = t[i] + t[i + o];
        v[m] = t[0];
    }
}

template <int N>
__device__ __forceinline__ void block_sum_i(int* v, int* scratch) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
    for (int m = 0; m < N; ++m)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[m] += __shfl_xor(v[m], o);
    __syncthreads();
    if (l == 0) {
#pragma unroll
        for (int m = 0; m < N; ++m) scratch[m * SAMPLE_WAVES + w] = v[m];
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < N; ++m) {
        int t = 0;
#pragma unroll
        for (int i = 0; i < SAMPLE_WAVES; ++i) t += scratch[m * SAMPLE_WAVES + i];
        v[m] = t;
    }
}

// block-wide maximum over 16 waves; every thread gets the result.  scratch: >= 16 words.
__device__ __forceinline__ float block_max_f(float v, float* scratch) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < SAMPLE_WAVES; ++i) v = fmaxf(v, scratch[i]);
    return v;
}

// (value, index) arg-max with the first index winning ties; every thread gets the result
__device__ __forceinline__ void block_argmax_first(float& v, int& i, float* sv, int* si) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    __syncthreads();
    if (l == 0) { sv[w] = v; si[w] = i; }
    __syncthreads();
    v = sv[0]; i = si[0];
#pragma unroll
    for (int k = 1; k < SAMPLE_WAVES; ++k) {
        const float ov = sv[k];
        const int oi = si[k];
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}

// block-wide exclusive scan of one value per thread, in thread order: Hillis-Steele inside the wave, then over the 16 wave totals.
// Returns the sum over the threads before this one; `total` receives the sum over all of them.  scratch: >= 32 words.
__device__ __forceinline__ float block_scan_f(float local, float& total, float* scratch) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    float inc = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(inc, o);
        if (l >= o) inc += t;
    }
    float exc = __shfl_up(inc, 1);
    if (l == 0) exc = 0.f;
    __syncthreads();
    if (l == 63) scratch[w] = inc;
    __syncthreads();
    if (w == 0) {
        float t = l < SAMPLE_WAVES ? scratch[l] : 0.f;
#pragma unroll
        for (int o = 1; o < SAMPLE_WAVES; o <<= 1) {
            const float u = __shfl_up(t, o);
            if (l >= o) t += u;
        }
        if (l < SAMPLE_WAVES) scratch[SAMPLE_WAVES + l] = t;     // inclusive totals of waves 0..l
    }
    __syncthreads();
    total = scratch[2 * SAMPLE_WAVES - 1];
    return (w ? scratch[SAMPLE_WAVES + w - 1] : 0.f) + exc;
}

// s = float32(logit) of one row into LDS: 16-byte loads over the aligned body, scalar head and tail (the base may be only 2-byte
// aligned).  The caller places the barrier.
__device__ __forceinline__ void load_row_scores(const bf16_t* lrow, int V, float* score) {
    const int tid = threadIdx.x;
    const int head = (int)((16 - (reinterpret_cast<size_t>(lrow) & 15)) & 15) >> 1;
    const int h = head < V ? head : V;
    const int nv = (V - h) >> 3;
    if (tid < h) score[tid] = bf2f(lrow[tid]);
    for (int vi = tid; vi < nv; vi += SAMPLE_THREADS) {
        float f[8];
        unpack8(ld16(lrow + h + vi * 8), f);
#pragma unroll
        for (int j = 0; j < 8; ++j) score[h + vi * 8 + j] = f[j];
    }
    for (int i = h + nv * 8 + tid; i < V; i += SAMPLE_THREADS) score[i] = bf2f(lrow[i]);
}

// largest key t with count{key >= t} >= k (1 <= k <= number of keys): the k-th largest key.  4-ary search, 16 levels.
__device__ __forceinline__ uint32_t select_kth(const uint32_t* keys, int i0, int n, int k, int* scratch) {
    uint32_t lo = 0;
    for (int shift = 30; shift >= 0; shift -= 2) {
        const uint32_t step = 1u << shift;
        int c[3] = {0, 0, 0};
#pragma unroll
        for (int j = 0; j < SAMPLE_CMAX; ++j) {
            if (j < n) {
                const uint32_t d = keys[i0 + j] - lo;            // keys below lo wrap to huge values: mask them
                const bool in = keys[i0 + j] >= lo;
                c[0] += (in && d >= step) ? 1 : 0;
                c[1] += (in && d >= 2 * step) ? 1 : 0;
                c[2] += (in && (d >> shift) >= 3u) ? 1 : 0;
            }
        }
        block_sum_i<3>(c, scratch);
        lo += c[2] >= k ? 3 * step : c[1] >= k ? 2 * step : c[0] >= k ? step : 0;
    }
    return lo;
}

// largest key t with mass{key < t} <= limit, p the thread's un-normalised probabilities of its ids.  4-ary search, 16 levels.
__device__ __forceinline__ uint32_t select_mass(const uint32_t* keys, const float (&p)[SAMPLE_CMAX], int i0, int n, float limit,
                                                float* scratch) {
    uint32_t lo = 0;
    for (int shift = 30; shift >= 0; shift -= 2) {
        const uint32_t stp = 1u << shift;
        float m[3] = {0.f, 0.f, 0.f};                            // mass{key < lo + (m + 1) * stp}
#pragma unroll
        for (int j = 0; j < SAMPLE_CMAX; ++j) {
            if (j < n) {
                const uint32_t k = keys[i0 + j];
                const uint32_t d = k - lo;
                const bool below = k < lo;
                m[0] += (below || d < stp) ? p[j] : 0.f;
                m[1] += (below || d < 2 * stp) ? p[j] : 0.f;
                m[2] += (below || (d >> shift) < 3u) ? p[j] : 0.f;
            }
        }
        block_sum_f<3>(m, scratch);
        lo += m[2] <= limit ? 3 * stp : m[1] <= limit ? 2 * stp : m[0] <= limit ? stp : 0;
    }
    return lo;
}

// The warpers' kept set of a row of keys (steps 6 and 7 of emu_amd/sampling.py): returns the lowest kept key, and the thread's
// un-normalised probabilities exp(s - mx) of what top-k keeps in p (what top-p removes is still in there: compare with the result).
__device__ __forceinline__ uint32_t warp_threshold(const uint32_t* keys, float (&p)[SAMPLE_CMAX], int i0, int n, int V, float mx,
                                                   int top_k, float top_p, int min_keep, float* sf, int* si) {
    // 6. top-k: drop s < k'-th largest value, ties stay
    uint32_t t_k = 0;
    {
        int kk = top_k > min_keep ? top_k : min_keep;
        if (top_k > 0 && kk < V) t_k = select_kth(keys, i0, n, kk, si);
    }
    // un-normalised probabilities of the owned ids (0 for what top-k removed) and their sum
    float z[1] = {0.f};
#pragma unroll
    for (int j = 0; j < SAMPLE_CMAX; ++j) {
        p[j] = 0.f;
        if (j < n) {
            const uint32_t k = keys[i0 + j];
            if (k >= t_k) p[j] = expf(key2f(k) - mx);
            z[0] += p[j];
        }
    }
    // 7. top-p: keep i iff mass{s_j <= s_i} > 1 - top_p, and everything >= the min_keep-th largest value
    uint32_t t_keep = t_k;
    if (top_p < 1.0f) {
        block_sum_f<1>(z, sf);
        const float limit = (1.0f - top_p) * z[0];
        const uint32_t lo = select_mass(keys, p, i0, n, limit, sf);
        const uint32_t t_min = min_keep <= 1 ? f2key(mx) : select_kth(keys, i0, n, min_keep < V ? min_keep : V, si);
        const uint32_t t_p = lo < t_min ? lo : t_min;
        t_keep = t_p > t_k ? t_p : t_k;
    }
    return t_keep;
}

}  // namespace
