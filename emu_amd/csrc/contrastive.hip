// Contrastive search on the device (lm.generate(penalty_alpha, top_k), Emu2/emu/emu.py:167,223): the per-token host work of
// LlamaEngine.contrastive_generate as launches that read their step from a device counter, so that one captured step replays for
// every token.  The specification is emu_amd/sampling.py (contrastive_reference_candidates / contrastive_reference_select).
//
//   pick     one workgroup per prompt: the logit row the previous step kept -> repetition penalty, min-length suppress, softmax,
//            the k most probable ids in descending order (ties to the lower id).  The row in LDS, the blocked sums and the key
//            search are sample_common.h's.
//   score 1  grid (context chunk, prompt): the dot products of CS_ROWS already-normalised fp32 context rows with the k candidates'
//            final-normed bf16 rows (held in LDS, un-normalised: their inverse norms are applied in phase 2) -> the chunk's maximum
//            per candidate.  Chunks beyond the current length exit at once.
//   score 2  one workgroup per prompt: maxima over the chunks, the candidates' norms (fp64 sums), score = (1 - a) p - a pen, first
//            maximum wins; token / EOS / PAD bookkeeping; the kept candidate's normalised row joins the context.
//   keep     the kept candidate's KV slot goes to its k - 1 siblings (one slot per row and layer).
//   advance  slot / position of the step's rows from the counter; counter + 1 (launch_step_advance, attention.hip).
//
// Every sum has a fixed order (no floating-point atomics): the same inputs give the same outputs bit for bit.  One dot product is, per
// lane, 4 * ceil(H / 256) sequential fp32 multiply-adds (elements it * 256 + lane * 4 + 0..3 in ascending order) and then the
// 6-level tree of wave_sum.
#include "sample_common.h"

namespace {

constexpr int CS_MAXK = EMU_CONTRASTIVE_MAX_K;
constexpr int CS_ROWS = EMU_CONTRASTIVE_CHUNK_ROWS;              // context rows per workgroup of phase 1
constexpr int CS_THREADS = 256;
constexpr int CS_WAVES = CS_THREADS / 64;
constexpr int CS_RPW = CS_ROWS / CS_WAVES;                       // rows a wave holds in registers at a time
static_assert(CS_ROWS % CS_WAVES == 0, "rows per wave");

// ------------------------------------------------------------------------------------------------------------------ pick
__global__ __launch_bounds__(SAMPLE_THREADS) void contrastive_pick_kernel(ContrastivePickArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    float* sf = reinterpret_cast<float*>(lds_raw);
    int* si = reinterpret_cast<int*>(lds_raw) + 64;
    uint32_t* keys = reinterpret_cast<uint32_t*>(lds_raw + SAMPLE_SCRATCH);
    float* score = reinterpret_cast<float*>(keys);               // the same words hold fp32 scores until the keys are made

    const int b = blockIdx.x, tid = threadIdx.x, V = a.vocab, k = a.k;
    const int step = *a.step;
    if (step >= a.L) return;
    int sj = a.sel ? a.sel[b] : 0;
    if (sj < 0 || sj >= k) sj = 0;
    const int srow = b * k + sj;
    const bf16_t* lrow = a.logits + (size_t)srow * a.ld;

    // s = float32(logit); repetition penalty once per distinct id (every occurrence writes the value computed from the ORIGINAL
    // logit); min-length suppress
    load_row_scores(lrow, V, score);
    __syncthreads();
    if (a.hist && a.penalty != 1.0f) {
        for (int t = tid; t < step; t += SAMPLE_THREADS) {
            const int id = a.hist[(size_t)t * a.hist_ld + b];
            if (id >= 0 && id < V) {
                const float s = bf2f(lrow[id]);
                score[id] = s < 0.f ? s * a.penalty : s / a.penalty;
            }
        }
        __syncthreads();
    }
    if (a.eos_id >= 0 && a.eos_id < V && step < a.min_len) {
        if (tid == 0) score[a.eos_id] = -INFINITY;
        __syncthreads();
    }

    int C = (V + SAMPLE_THREADS - 1) / SAMPLE_THREADS;
    C |= 1;
    const int i0 = tid * C;
    const int n = i0 >= V ? 0 : (V - i0 < C ? V - i0 : C);       // ids this thread owns: [i0, i0 + n)

    // -0 -> +0, scores -> keys in place; the row maximum
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < SAMPLE_CMAX; ++j) {
        if (j < n) {
            float s = score[i0 + j];
            if (s == 0.f) s = 0.f;
            mx = fmaxf(mx, s);
            keys[i0 + j] = f2key(s);
        }
    }
    mx = block_max_f(mx, sf);
    // (each thread reads only the keys it wrote itself from here on)

    // softmax denominator: at most SAMPLE_CMAX sequential adds in ascending id order, then the fixed tree
    float z[1] = {0.f};
#pragma unroll
    for (int j = 0; j < SAMPLE_CMAX; ++j)
        if (j < n) z[0] += expf(key2f(keys[i0 + j]) - mx);
    block_sum_f<1>(z, sf);

    // the k-th largest value; the candidates are everything above it and the lowest ids at it
    const uint32_t t_k = select_kth(keys, i0, n, k, si);

    // k rounds of (value, first index) arg-max over what has not been emitted yet: descending value, ties to the lower id
    float pv = INFINITY;
    int pi = -1;
    for (int r = 0; r < k; ++r) {
        float best = -INFINITY;
        int bi = 0x7fffffff;
        for (int j = 0; j < n; ++j) {
            const uint32_t key = keys[i0 + j];
            if (key < t_k) continue;
            const float s = key2f(key);
            const int id = i0 + j;
            const bool open = r == 0 || s < pv || (s == pv && id > pi);
            if (open && (s > best || (s == best && id < bi))) { best = s; bi = id; }
        }
        block_argmax_first(best, bi, sf, si);
        pv = best; pi = bi;
        if (tid == 0) {
            a.cand_ids[b * k + r] = bi < V ? bi : 0;
            a.cand_p[b * k + r] = expf(best - mx) / z[0];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ score, phase 1
// KP: k rounded up to a power of two (the LDS rows beyond k are zero and their maxima are not written)
template <int KP>
__global__ __launch_bounds__(CS_THREADS) void contrastive_score1_kernel(ContrastiveScoreArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    bf16_t* cand = reinterpret_cast<bf16_t*>(lds_raw);           // [KP, H]
    __shared__ float wmax[CS_WAVES][CS_MAXK];

    const int step = *a.step;
    if (step >= a.L) return;
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x, H = a.H, k = a.k;
    const int len = a.S + step;                                  // valid context rows: [kstart, len)
    const int r0 = chunk * CS_ROWS;
    if (r0 >= len) return;
    const int ks = a.kstart ? a.kstart[b] : 0;
    float* part = a.ws + ((size_t)b * a.nchunks + chunk) * CS_MAXK;
    if (r0 + CS_ROWS <= ks) {                                    // left padding only
        if (tid < k) part[tid] = -INFINITY;
        return;
    }

    // the candidates' rows -> LDS, 8 bytes (4 bf16) per lane and load
    const int H4 = H >> 2;
    for (int j = 0; j < KP; ++j) {
        const bf16_t* src = a.cand + ((size_t)b * k + j) * H;
        for (int e = tid; e < H4; e += CS_THREADS) {
            u32x2 v = {0u, 0u};
            if (j < k) v = *reinterpret_cast<const u32x2*>(src + e * 4);
            *reinterpret_cast<u32x2*>(cand + (size_t)j * H + e * 4) = v;
        }
    }
    __syncthreads();

    const int w = tid >> 6, l = tid & 63;
    float acc[CS_RPW][KP];
    const float* rowp[CS_RPW];
    bool ok[CS_RPW];
#pragma unroll
    for (int i = 0; i < CS_RPW; ++i) {
        const int r = r0 + w * CS_RPW + i;
        ok[i] = r >= ks && r < len;
        rowp[i] = a.ctx_n + ((size_t)b * a.Lc + (ok[i] ? r : r0 < ks ? ks : r0)) * H;       // a row inside the buffer either way
#pragma unroll
        for (int j = 0; j < KP; ++j) acc[i][j] = 0.f;
    }
    for (int e = l * 4; e < H; e += 256) {
        f32x4_t x[CS_RPW];
#pragma unroll
        for (int i = 0; i < CS_RPW; ++i) x[i] = *reinterpret_cast<const f32x4_t*>(rowp[i] + e);
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            const u32x2 c = *reinterpret_cast<const u32x2*>(cand + (size_t)j * H + e);
            const float c0 = bflo(c[0]), c1 = bfhi(c[0]), c2 = bflo(c[1]), c3 = bfhi(c[1]);
#pragma unroll
            for (int i = 0; i < CS_RPW; ++i) {
                float s = acc[i][j];
                s = fmaf(x[i][0], c0, s);
                s = fmaf(x[i][1], c1, s);
                s = fmaf(x[i][2], c2, s);
                s = fmaf(x[i][3], c3, s);
                acc[i][j] = s;
            }
        }
    }
    // the wave's maximum per candidate over its valid rows
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < CS_RPW; ++i) {
            const float d = wave_sum(acc[i][j]);
            if (ok[i]) m = fmaxf(m, d);
        }
        if (l == 0 && j < k) wmax[w][j] = m;
    }
    __syncthreads();
    if (tid < k) {
        float m = wmax[0][tid];
#pragma unroll
        for (int i = 1; i < CS_WAVES; ++i) m = fmaxf(m, wmax[i][tid]);
        part[tid] = m;
    }
}

// ------------------------------------------------------------------------------------------------------------------ score, phase 2
__global__ __launch_bounds__(CS_THREADS) void contrastive_score2_kernel(ContrastiveScoreArgs a) {
    __shared__ double red[CS_THREADS];
    __shared__ float fmx[CS_WAVES][CS_MAXK];
    __shared__ float inv_s[CS_MAXK];
    __shared__ int sel_s;

    const int step = *a.step;
    if (step >= a.L) return;
    const int b = blockIdx.x, tid = threadIdx.x, H = a.H, k = a.k;
    if (a.unfinished[b] == 0) {                                  // a finished prompt emits PAD and nothing else of it is written
        if (tid == 0) a.out_ids[(size_t)step * a.B + b] = a.pad_id;
        return;
    }
    const int len = a.S + step;
    const int nlive = (len + CS_ROWS - 1) / CS_ROWS;
    const int w = tid >> 6, l = tid & 63;

    // maxima over the live chunks
    float m[CS_MAXK];
#pragma unroll
    for (int j = 0; j < CS_MAXK; ++j) m[j] = -INFINITY;
    for (int c = tid; c < nlive; c += CS_THREADS) {
        const float* part = a.ws + ((size_t)b * a.nchunks + c) * CS_MAXK;
#pragma unroll
        for (int j = 0; j < CS_MAXK; ++j)
            if (j < k) m[j] = fmaxf(m[j], part[j]);
    }
#pragma unroll
    for (int j = 0; j < CS_MAXK; ++j) {
        m[j] = wave_max(m[j]);
        if (l == 0) fmx[w][j] = m[j];
    }
    // the candidates' norms: fp64 sums in a fixed order (strided per thread, then a tree over the threads)
    for (int j = 0; j < k; ++j) {
        const bf16_t* src = a.cand + ((size_t)b * k + j) * H;
        double ss = 0.0;
        for (int e = tid; e < H; e += CS_THREADS) {
            const double x = (double)bf2f(src[e]);
            ss += x * x;
        }
        __syncthreads();
        red[tid] = ss;
        __syncthreads();
        for (int o = CS_THREADS / 2; o > 0; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        if (tid == 0) inv_s[j] = (float)(1.0 / sqrt(red[0]));
    }
    __syncthreads();
    if (tid == 0) {
        float best = -INFINITY;
        int bj = 0;
        for (int j = 0; j < k; ++j) {
            float d = fmx[0][j];
            for (int i = 1; i < CS_WAVES; ++i) d = fmaxf(d, fmx[i][j]);
            const float pen = __fmul_rn(d, inv_s[j]);
            const float sc = __fsub_rn(__fmul_rn(a.one_minus_alpha, a.cand_p[b * k + j]), __fmul_rn(a.alpha, pen));
            if (a.pen_out) a.pen_out[b * k + j] = pen;
            if (j == 0 || sc > best) { best = sc; bj = j; }      // the first maximum wins
        }
        const int tok = a.cand_ids[b * k + bj];
        a.out_ids[(size_t)step * a.B + b] = tok;
        if (tok == a.eos_id) a.unfinished[b] = 0;
        a.sel[b] = bj;
        sel_s = bj;
    }
    __syncthreads();
    // the kept candidate's normalised row joins the context
    const int sj = sel_s;
    const float inv = inv_s[sj];
    const bf16_t* src = a.cand + ((size_t)b * k + sj) * H;
    float* dst = a.ctx_n + ((size_t)b * a.Lc + len) * H;
    for (int e = tid; e < H; e += CS_THREADS) dst[e] = __fmul_rn(bf2f(src[e]), inv);
}

// ------------------------------------------------------------------------------------------------------------------ keep
// cache [layers, rows, Hl, s_max, D]: slot slot0 + step of row g * k + sel[g] -> its k - 1 siblings.  grid (layers * Hl, groups).
__global__ __launch_bounds__(128) void contrastive_keep_kernel(bf16_t* kc, bf16_t* vc, const int32_t* sel, const int32_t* step_dev,
                                                               int rows, int Hl, int s_max, int D, int k, int slot0, int L) {
    const int step = *step_dev;
    if (step >= L) return;
    const int lh = blockIdx.x, layer = lh / Hl, h = lh - layer * Hl, g = blockIdx.y;
    int sj = sel[g];
    if (sj < 0 || sj >= k) sj = 0;
    const int pieces = D >> 3, slot = slot0 + step;
    const size_t so = ((((size_t)layer * rows + g * k + sj) * Hl + h) * s_max + slot) * D;
    for (int i = threadIdx.x; i < k * pieces; i += blockDim.x) {
        const int j = i / pieces, piece = i - j * pieces;
        if (j == sj) continue;
        const size_t dofs = ((((size_t)layer * rows + g * k + j) * Hl + h) * s_max + slot) * D;
        st16(kc + dofs + piece * 8, ld16(kc + so + piece * 8));
        st16(vc + dofs + piece * 8, ld16(vc + so + piece * 8));
    }
}

}  // namespace

int launch_contrastive_pick(const ContrastivePickArgs& a, hipStream_t s) {
    if (!a.logits || !a.step || !a.cand_ids || !a.cand_p || a.B < 1 || a.k < 1 || a.k > CS_MAXK || a.vocab < a.k ||
        a.vocab > EMU_SAMPLE_MAX_VOCAB || a.ld < a.vocab || a.L < 1 || !(a.penalty > 0.f) || (a.hist && a.hist_ld < a.B))
        return -22;
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(contrastive_pick_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                SAMPLE_SCRATCH + EMU_SAMPLE_MAX_VOCAB * 4) != hipSuccess)
            return -5;
        attr_set = true;
    }
    const size_t lds = SAMPLE_SCRATCH + (((size_t)a.vocab * 4 + 15) & ~(size_t)15);
    hipLaunchKernelGGL(contrastive_pick_kernel, dim3(a.B), dim3(SAMPLE_THREADS), lds, s, a);
    EMU_CHECK_LAUNCH();
    return 0;
}

size_t contrastive_ws_floats(int B, int k, int Lc) {
    (void)k;
    return (size_t)B * ((Lc + CS_ROWS - 1) / CS_ROWS) * CS_MAXK;
}

template <int KP>
static int launch_score1(const ContrastiveScoreArgs& a, hipStream_t s) {
    const size_t lds = (size_t)KP * a.H * sizeof(bf16_t);
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(contrastive_score1_kernel<KP>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                KP * EMU_CONTRASTIVE_MAX_HIDDEN * (int)sizeof(bf16_t)) != hipSuccess)
            return -5;
        attr_set = true;
    }
    hipLaunchKernelGGL(contrastive_score1_kernel<KP>, dim3(a.nchunks, a.B), dim3(CS_THREADS), lds, s, a);
    EMU_CHECK_LAUNCH();
    return 0;
}

int launch_contrastive_score(ContrastiveScoreArgs a, size_t ws_floats, hipStream_t s) {
    if (!a.ctx_n || !a.cand || !a.cand_ids || !a.cand_p || !a.step || !a.out_ids || !a.unfinished || !a.sel || !a.ws || a.B < 1 ||
        a.k < 1 || a.k > CS_MAXK || a.H < 4 || (a.H & 3) || a.H > EMU_CONTRASTIVE_MAX_HIDDEN || a.S < 1 || a.L < 1 ||
        a.Lc < a.S + a.L || ws_floats < contrastive_ws_floats(a.B, a.k, a.Lc))
        return -22;
    a.nchunks = (a.Lc + CS_ROWS - 1) / CS_ROWS;
    int rc;
    if (a.k == 1) rc = launch_score1<1>(a, s);
    else if (a.k == 2) rc = launch_score1<2>(a, s);
    else if (a.k <= 4) rc = launch_score1<4>(a, s);
    else rc = launch_score1<8>(a, s);
    if (rc) return rc;
    hipLaunchKernelGGL(contrastive_score2_kernel, dim3(a.B), dim3(CS_THREADS), 0, s, a);
    EMU_CHECK_LAUNCH();
    return 0;
}

int launch_contrastive_keep(bf16_t* kc, bf16_t* vc, const int32_t* sel, const int32_t* step_dev, int layers, int rows, int Hl, int s_max,
                            int D, int k, int slot0, int L, hipStream_t s) {
    if (!kc || !vc || !sel || !step_dev || k < 1 || k > CS_MAXK || rows < k || rows % k || D < 8 || (D & 7) || slot0 < 0 || L < 1 ||
        slot0 + L > s_max)
        return -22;
    if (k == 1) return 0;                              // no sibling
    hipLaunchKernelGGL(contrastive_keep_kernel, dim3(layers * Hl, rows / k), dim3(128), 0, s, kc, vc, sel, step_dev, rows, Hl, s_max, D,
                       k, slot0, L);
    EMU_CHECK_LAUNCH();
    return 0;
}
