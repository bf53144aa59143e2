// Next-token selection with transformers' logits pipeline in ONE launch (the specification is emu_amd/sampling.py):
// repetition penalty over the ids generated so far, min-length suppress, then either the first-index arg-max or
// temperature -> top-k -> top-p -> one draw from a caller-supplied uniform; EOS / PAD bookkeeping of the row in the same launch.
// Replaces, per token, the torch launches of LlamaEngine.sample_generate (Emu2/emu/emu.py:213-229 -> lm.generate(do_sample=True,
// temperature, top_p, ...), the mode the chat demo runs).
//
// One workgroup of 1024 threads per row.  The row lives in LDS as the order-preserving integer image ("key") of its fp32 scores:
// 4 bytes per token of dynamic LDS, so the vocabulary bound is EMU_SAMPLE_MAX_VOCAB = 40 000 (160 000 B + 1 KiB of reduction
// scratch of the CU's 160 KiB).  Thread t owns the contiguous ids [t * C, t * C + C) with C = ceil(V / 1024) made odd, so that the
// 64 lanes of a wave read 64 different banks; the un-normalised probabilities exp(s - max) of the owned ids stay in registers.
//
// Thresholds without a sort: the top-k value is the largest key t with count{key >= t} >= k', the top-p value the largest key t
// with mass{key < t} <= (1 - top_p) * Z; both are found by a 4-ary search over the 32 key bits (16 levels, three thresholds per
// level, one pass over the row each).  Every sum over the row is blocked: at most SAMPLE_CMAX sequential fp32 adds per thread in
// ascending id order, then a fixed tree (6 levels inside the wave, 4 across the 16 waves) -- no floating-point atomics, so the
// same inputs give the same token and the same probabilities on every launch.
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

struct SampleArgs {
    const bf16_t* logits; int ld; int vocab;
    const int32_t* hist; int hist_ld; int hist_rows;             // ids generated so far: hist[t * hist_ld + row], t < min(step, hist_rows)
    const int32_t* step;                                         // device int32[1]
    const float* uniforms; int uni_ld; int uni_rows;             // u = uniforms[min(step, uni_rows - 1) * uni_ld + row]
    float penalty; int suppress_id; int min_len;
    int do_sample; float temperature; int top_k; float top_p; int min_keep;
    int eos_id; int pad_id;
    int32_t* unfinished; int32_t* out; float* probs; int ld_probs;
};

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

__global__ __launch_bounds__(SAMPLE_THREADS) void sample_kernel(SampleArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    float* sf = reinterpret_cast<float*>(lds_raw);               // 192 words of reduction scratch
    int* si = reinterpret_cast<int*>(lds_raw) + 64;
    int* found = reinterpret_cast<int*>(lds_raw) + 200;          // [0] lowest id past the draw, [1] highest kept id
    uint32_t* keys = reinterpret_cast<uint32_t*>(lds_raw + SAMPLE_SCRATCH);
    float* score = reinterpret_cast<float*>(keys);               // the same words hold fp32 scores until the keys are made

    const int row = blockIdx.x, tid = threadIdx.x, V = a.vocab;
    if (a.unfinished && a.unfinished[row] == 0) {                // a finished row emits PAD whatever its logits
        if (tid == 0) a.out[row] = a.pad_id;
        return;
    }
    const bf16_t* lrow = a.logits + (size_t)row * a.ld;
    const int step = *a.step;

    // 1. s = float32(logit): 16-byte loads over the aligned body, scalar head and tail (the base may be only 2-byte aligned)
    {
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
    __syncthreads();
    // 2. repetition penalty, once per distinct id: every occurrence writes the same value computed from the ORIGINAL logit
    if (a.hist && a.penalty != 1.0f) {
        const int nh = step < a.hist_rows ? step : a.hist_rows;
        for (int t = tid; t < nh; t += SAMPLE_THREADS) {
            const int id = a.hist[(size_t)t * a.hist_ld + row];
            if (id >= 0 && id < V) {
                const float s = bf2f(lrow[id]);
                score[id] = s < 0.f ? s * a.penalty : s / a.penalty;
            }
        }
        __syncthreads();
    }
    // 3. min-length suppress
    if (a.suppress_id >= 0 && a.suppress_id < V && step < a.min_len) {
        if (tid == 0) score[a.suppress_id] = -INFINITY;
        __syncthreads();
    }

    int C = (V + SAMPLE_THREADS - 1) / SAMPLE_THREADS;
    C |= 1;
    const int i0 = tid * C;
    const int n = i0 >= V ? 0 : (V - i0 < C ? V - i0 : C);       // ids this thread owns: [i0, i0 + n)

    // 4. greedy: first index of the maximum
    if (!a.do_sample) {
        float best = -INFINITY;
        int bi = 0x7fffffff;
        for (int j = 0; j < n; ++j) {
            const float s = score[i0 + j];
            if (s > best || (s == best && i0 + j < bi)) { best = s; bi = i0 + j; }
        }
        block_argmax_first(best, bi, sf, si);
        if (tid == 0) {
            const int tok = bi < V ? bi : 0;
            a.out[row] = tok;
            if (a.unfinished && tok == a.eos_id) a.unfinished[row] = 0;
        }
        return;
    }

    // 5. temperature (IEEE division), -0 -> +0, scores -> keys in place; the row maximum
    float mx = -INFINITY;
    const bool scale = a.temperature != 1.0f;
#pragma unroll
    for (int j = 0; j < SAMPLE_CMAX; ++j) {
        if (j < n) {
            float s = score[i0 + j];
            if (scale) s = s / a.temperature;
            if (s == 0.f) s = 0.f;
            mx = fmaxf(mx, s);
            keys[i0 + j] = f2key(s);
        }
    }
    mx = wave_max(mx);
    __syncthreads();
    if ((tid & 63) == 0) sf[tid >> 6] = mx;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < SAMPLE_WAVES; ++i) mx = fmaxf(mx, sf[i]);
    // (each thread reads only the keys it wrote itself from here on: no further barrier is needed for the keys)

    // 6. top-k: drop s < k'-th largest value, ties stay
    uint32_t t_k = 0;
    {
        int kk = a.top_k > a.min_keep ? a.top_k : a.min_keep;
        if (a.top_k > 0 && kk < V) t_k = select_kth(keys, i0, n, kk, si);
    }
    // un-normalised probabilities of the owned ids (0 for what top-k removed) and their sum
    float p[SAMPLE_CMAX];
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
    if (a.top_p < 1.0f) {
        block_sum_f<1>(z, sf);
        const float limit = (1.0f - a.top_p) * z[0];
        uint32_t lo = 0;
        for (int shift = 30; shift >= 0; shift -= 2) {
            const uint32_t stp = 1u << shift;
            float m[3] = {0.f, 0.f, 0.f};                        // mass{key < lo + (m + 1) * stp}
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
            block_sum_f<3>(m, sf);
            lo += m[2] <= limit ? 3 * stp : m[1] <= limit ? 2 * stp : m[0] <= limit ? stp : 0;
        }
        const uint32_t t_min = a.min_keep <= 1 ? f2key(mx) : select_kth(keys, i0, n, a.min_keep < V ? a.min_keep : V, si);
        const uint32_t t_p = lo < t_min ? lo : t_min;
        t_keep = t_p > t_k ? t_p : t_k;
    }

    // 8. q = softmax over the kept tokens; the draw: lowest id whose inclusive cumulative q in ascending id order exceeds u
    float local = 0.f;
    int hi_kept = -1;
#pragma unroll
    for (int j = 0; j < SAMPLE_CMAX; ++j) {
        if (j < n) {
            if (keys[i0 + j] < t_keep) p[j] = 0.f;
            local += p[j];
            if (p[j] > 0.f) hi_kept = i0 + j;
        }
    }
    // block-wide exclusive scan of `local` in thread order: Hillis-Steele inside the wave, then over the 16 wave totals
    const int w = tid >> 6, l = tid & 63;
    float inc = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(inc, o);
        if (l >= o) inc += t;
    }
    float exc = __shfl_up(inc, 1);
    if (l == 0) exc = 0.f;
    __syncthreads();
    if (l == 63) sf[w] = inc;
    if (tid == 0) { found[0] = 0x7fffffff; found[1] = -1; }
    __syncthreads();
    if (w == 0) {
        float t = l < SAMPLE_WAVES ? sf[l] : 0.f;
#pragma unroll
        for (int o = 1; o < SAMPLE_WAVES; o <<= 1) {
            const float u = __shfl_up(t, o);
            if (l >= o) t += u;
        }
        if (l < SAMPLE_WAVES) sf[SAMPLE_WAVES + l] = t;          // inclusive totals of waves 0..l
    }
    __syncthreads();
    const float total = sf[2 * SAMPLE_WAVES - 1];
    const float base = (w ? sf[SAMPLE_WAVES + w - 1] : 0.f) + exc;
    int lo_step = step < a.uni_rows ? step : a.uni_rows - 1;
    if (lo_step < 0) lo_step = 0;
    const float target = a.uniforms[(size_t)lo_step * a.uni_ld + row] * total;
    // cumulative of id i0 + j = base + (the chunk's own sequential prefix): a term passes at most 40 sequential adds, 6 + 4 scan
    // levels and two more adds on its way into any cumulative value
    int hit = 0x7fffffff;
    float lp = 0.f;
#pragma unroll
    for (int j = 0; j < SAMPLE_CMAX; ++j) {
        if (j < n && p[j] > 0.f) {
            lp += p[j];
            if (base + lp > target && hit == 0x7fffffff) hit = i0 + j;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        hit = min(hit, __shfl_xor(hit, o));
        hi_kept = max(hi_kept, __shfl_xor(hi_kept, o));
    }
    if (l == 0) {
        if (hit != 0x7fffffff) atomicMin(&found[0], hit);
        if (hi_kept >= 0) atomicMax(&found[1], hi_kept);
    }
    if (a.probs) {
        float* pr = a.probs + (size_t)row * a.ld_probs;
#pragma unroll
        for (int j = 0; j < SAMPLE_CMAX; ++j)
            if (j < n) pr[i0 + j] = p[j] / total;
    }
    __syncthreads();
    if (tid == 0) {
        int tok = found[0] != 0x7fffffff ? found[0] : found[1];  // rounding left u at or beyond the total: highest kept id
        if (tok < 0 || tok >= V) tok = 0;
        a.out[row] = tok;
        if (a.unfinished && tok == a.eos_id) a.unfinished[row] = 0;
    }
}

}  // namespace

int launch_sample(const bf16_t* logits, int ld, int rows, int vocab, const int32_t* hist, int hist_ld, int hist_rows,
                  const int32_t* step_dev, const float* uniforms, int uni_ld, int uni_rows, const emu_sample_params* p,
                  int32_t* unfinished, int32_t* out, float* probs_out, int ld_probs, hipStream_t s) {
    if (!logits || !step_dev || !out || !p || rows < 1 || vocab < 1 || vocab > EMU_SAMPLE_MAX_VOCAB || ld < vocab) return -22;
    if (p->min_keep < 1 || !(p->repetition_penalty > 0.f)) return -22;
    if (p->do_sample && (!uniforms || uni_rows < 1 || uni_ld < rows || !(p->temperature > 0.f) || !(p->top_p > 0.f))) return -22;
    if (hist && (hist_ld < rows || hist_rows < 0)) return -22;
    if (probs_out && ld_probs < vocab) return -22;
    SampleArgs a;
    a.logits = logits; a.ld = ld; a.vocab = vocab;
    a.hist = hist; a.hist_ld = hist_ld; a.hist_rows = hist_rows;
    a.step = step_dev;
    a.uniforms = uniforms; a.uni_ld = uni_ld; a.uni_rows = uni_rows;
    a.penalty = p->repetition_penalty; a.suppress_id = p->suppress_id; a.min_len = p->min_len;
    a.do_sample = p->do_sample; a.temperature = p->temperature; a.top_k = p->top_k; a.top_p = p->top_p; a.min_keep = p->min_keep;
    a.eos_id = p->eos_id; a.pad_id = p->pad_id;
    a.unfinished = unfinished; a.out = out; a.probs = probs_out; a.ld_probs = ld_probs;
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(sample_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                SAMPLE_SCRATCH + EMU_SAMPLE_MAX_VOCAB * 4) != hipSuccess)
            return -5;
        attr_set = true;
    }
    const size_t lds = SAMPLE_SCRATCH + (((size_t)vocab * 4 + 15) & ~(size_t)15);
    hipLaunchKernelGGL(sample_kernel, dim3(rows), dim3(SAMPLE_THREADS), lds, s, a);
    EMU_CHECK_LAUNCH();
    return 0;
}
