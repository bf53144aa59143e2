// Next-token selection with transformers' logits pipeline in ONE launch (the specification is emu_amd/sampling.py):
// repetition penalty over the ids generated so far, min-length suppress, then either the first-index arg-max or
// temperature -> top-k -> top-p -> one draw from a caller-supplied uniform; EOS / PAD bookkeeping of the row in the same launch.
// Replaces, per token, the torch launches of LlamaEngine.sample_generate (Emu2/emu/emu.py:213-229 -> lm.generate(do_sample=True,
// temperature, top_p, ...), the mode the chat demo runs).
//
// One workgroup of 1024 threads per row; the row in LDS as keys, the odd per-thread chunks, the threshold searches and the blocked sums
// are sample_common.h's (shared with the beam rows of beam_sample.hip).  The un-normalised probabilities exp(s - max) of the owned
// ids stay in registers.
//
// Under a constraint (emu_sample_trie_bf16) every thread walks the sorted edge slice of the row's trie node alongside the ids it owns
// and writes -inf over those that are no edge, right after the suppress: the row fills the LDS at V = 40 000, so there is no room for
// a bitmap, and from there on a thread reads only the ids it owns, so the mask needs no barrier of its own.  Thread 0 advances the
// node by the id it files.
//
// With a no-repeat n-gram ban (emu_sample_ngram_bf16; ngram.h) the threads share the start positions of the row's history and write
// -inf over the id behind every repetition of its last n - 1 ids, between the penalty and the suppress (the library's processor
// order); one barrier follows, since the banned id is rarely one the writing thread owns.
//
// The body is one __device__ function of (row, history, step, uniform); sample_kernel gives it a column of the table of generated
// ids, lookup_sample_kernel (emu_lookup_sample_bf16: prompt-lookup speculation for sampling and penalised greedy decoding) the
// generated ids followed by the draft ids fed ahead of the chunk row, so that row i is picked as output index step + i would be.
#include "sample_common.h"
#include "trie.h"
#include "ngram.h"

namespace {

struct SampleArgs {
    const bf16_t* logits; int ld; int vocab;
    const int32_t* hist; int hist_ld; int hist_rows;             // ids generated so far: hist[t * hist_ld + row], t < min(step, hist_rows)
    const int32_t* step;                                         // device int32[1]
    const float* uniforms; int uni_ld; int uni_rows;             // u = uniforms[min(step, uni_rows - 1) * uni_ld + row]
    float penalty; int suppress_id; int min_len;
    int do_sample; float temperature; int top_k; float top_p; int min_keep;
    int eos_id; int pad_id;
    int32_t* unfinished; int32_t* out; float* probs; int ld_probs;
    emu_token_trie trie; int32_t* node;                          // node null = no constraint
    int ngram;                                                   // no-repeat n-gram size over hist; 0 = off
};

// A row's history, as the body below reads it: n ids, id t = at(t).  ColumnHist is a column of an int32 table in memory (the one-row
// loops: hist[t * ld + row]); ChunkHist is row i of a prompt-lookup chunk step: the `step` generated ids of out_ids, then the i draft
// ids cur[1 .. 1 + i) that were fed ahead of the row.
struct ColumnHist {
    const int32_t* p; size_t ld; int n;
    static constexpr bool kColumn = true;
    __device__ __forceinline__ bool present() const { return p != nullptr; }
    __device__ __forceinline__ int at(int t) const { return p[(size_t)t * ld]; }
};
struct ChunkHist {
    const int32_t* out_ids; const int32_t* cur; int step; int n;
    static constexpr bool kColumn = false;
    __device__ __forceinline__ bool present() const { return true; }
    __device__ __forceinline__ int at(int t) const { return t < step ? out_ids[t] : cur[1 + t - step]; }
};

// The selection of one row by one workgroup: logits row `row` of a, the history `hist`, the step index `step` (min-length suppress,
// row of the uniforms) and column `ucol` of the uniforms; the id goes to a.out[row].  a.step is not read.
template <class Hist>
__device__ __forceinline__ void sample_row(const SampleArgs& a, const int row, const int ucol, const Hist hist, const int step,
                                           unsigned char* lds_raw) {
    float* sf = reinterpret_cast<float*>(lds_raw);               // 192 words of reduction scratch
    int* si = reinterpret_cast<int*>(lds_raw) + 64;
    int* found = reinterpret_cast<int*>(lds_raw) + 200;          // [0] lowest id past the draw, [1] highest kept id
    uint32_t* keys = reinterpret_cast<uint32_t*>(lds_raw + SAMPLE_SCRATCH);
    float* score = reinterpret_cast<float*>(keys);               // the same words hold fp32 scores until the keys are made

    const int tid = threadIdx.x, V = a.vocab;
    const bf16_t* lrow = a.logits + (size_t)row * a.ld;

    // 1. s = float32(logit)
    load_row_scores(lrow, V, score);
    __syncthreads();
    // 2. repetition penalty, once per distinct id: every occurrence writes the same value computed from the ORIGINAL logit
    if (hist.present() && a.penalty != 1.0f) {
        for (int t = tid; t < hist.n; t += SAMPLE_THREADS) {
            const int id = hist.at(t);
            if (id >= 0 && id < V) {
                const float s = bf2f(lrow[id]);
                score[id] = s < 0.f ? s * a.penalty : s / a.penalty;
            }
        }
        __syncthreads();
    }
    // 2a. no-repeat n-gram ban: the id behind every earlier occurrence of the row's last n - 1 ids -> -inf
    if constexpr (Hist::kColumn) {
        if (hist.present() && a.ngram > 0) {
            ngram_matches(hist.p, hist.ld, hist.n, a.ngram, tid, SAMPLE_THREADS, [&](int id) {
                if (id >= 0 && id < V) score[id] = -INFINITY;
            });
            __syncthreads();
        }
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

    // 3a. constraint: the ids that are no edge of the row's node -> -inf (the exhausted node allows EOS alone)
    const int node = a.node ? a.node[row] : 0;
    if (a.node) {
        int lo, hi;
        const bool live = trie_edges(a.trie, node, lo, hi);
        int e = live && n > 0 ? trie_lower_bound(a.trie.tok, lo, hi, i0) : hi;
        for (int j = 0; j < n; ++j) {
            const int id = i0 + j;
            bool ok;
            if (live) {
                while (e < hi && a.trie.tok[e] < id) ++e;
                ok = e < hi && a.trie.tok[e] == id;
            } else {
                ok = id == a.eos_id;
            }
            if (!ok) score[id] = -INFINITY;
        }
    }

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
            if (a.node) a.node[row] = trie_child(a.trie, node, tok);
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
    mx = block_max_f(mx, sf);
    // (each thread reads only the keys it wrote itself from here on: no further barrier is needed for the keys)

    // 6. top-k (drop s < k'-th largest value, ties stay), 7. top-p (keep i iff mass{s_j <= s_i} > 1 - top_p, and everything >= the
    // min_keep-th largest value); p: un-normalised probabilities of the owned ids
    float p[SAMPLE_CMAX];
    const uint32_t t_keep = warp_threshold(keys, p, i0, n, V, mx, a.top_k, a.top_p, a.min_keep, sf, si);

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
    // block-wide exclusive scan of `local` in thread order
    const int l = tid & 63;
    if (tid == 0) { found[0] = 0x7fffffff; found[1] = -1; }
    float total;
    const float base = block_scan_f(local, total, sf);
    int lo_step = step < a.uni_rows ? step : a.uni_rows - 1;
    if (lo_step < 0) lo_step = 0;
    const float target = a.uniforms[(size_t)lo_step * a.uni_ld + ucol] * total;
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
        if (a.node) a.node[row] = trie_child(a.trie, node, tok);
    }
}

__global__ __launch_bounds__(SAMPLE_THREADS) void sample_kernel(SampleArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int row = blockIdx.x;
    if (a.unfinished && a.unfinished[row] == 0) {                // a finished row emits PAD whatever its logits
        if (threadIdx.x == 0) a.out[row] = a.pad_id;
        return;
    }
    const int step = *a.step;
    const ColumnHist hist{a.hist ? a.hist + row : nullptr, (size_t)a.hist_ld, step < a.hist_rows ? step : a.hist_rows};
    sample_row(a, row, row, hist, step, lds_raw);
}

// The selection behind a prompt-lookup chunk step when it samples or penalises (emu_amd/speculate.py: row_select): workgroup i picks
// the id of chunk row i exactly as sample_kernel would pick output index step + i -- history = the step generated ids, then the i
// draft ids fed ahead of the row.  The ids go to amax[i], where lookup_select_kernel reads them.  The step, the finished flag and the
// number of draft ids come from the device, so one captured launch serves every iteration; a workgroup past the end, or of a row
// behind the draft (lookup_select_kernel reads amax[0 .. n_draft] only), returns without writing.
struct LookupSampleArgs { const int32_t* st; const int32_t* cur; const int32_t* out_ids; int max_new; };

__global__ __launch_bounds__(SAMPLE_THREADS) void lookup_sample_kernel(SampleArgs a, LookupSampleArgs l) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int i = blockIdx.x, step = l.st[LOOKUP_STEP];
    if (step >= l.max_new || l.st[LOOKUP_FINISHED] || i > l.st[LOOKUP_NDRAFT]) return;       // (uniform)
    const ChunkHist hist{l.out_ids, l.cur, step, step + i};
    sample_row(a, i, 0, hist, step + i, lds_raw);
}

template <class Kernel>
int sample_lds_attr(Kernel kernel, bool& set) {
    if (!set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                SAMPLE_SCRATCH + EMU_SAMPLE_MAX_VOCAB * 4) != hipSuccess)
            return -5;
        set = true;
    }
    return 0;
}

}  // namespace

int launch_sample(const bf16_t* logits, int ld, int rows, int vocab, const int32_t* hist, int hist_ld, int hist_rows,
                  const int32_t* step_dev, const float* uniforms, int uni_ld, int uni_rows, const emu_sample_params* p,
                  int32_t* unfinished, int32_t* out, float* probs_out, int ld_probs, const emu_token_trie* trie, int32_t* node,
                  int ngram, hipStream_t s) {
    if ((trie || node) && !trie_args_ok(trie, node)) return -22;
    if (ngram < 0) return -22;
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
    a.trie = trie ? *trie : emu_token_trie{}; a.node = node;
    a.ngram = ngram;
    static bool attr_set = false;
    if (int e = sample_lds_attr(sample_kernel, attr_set)) return e;
    const size_t lds = SAMPLE_SCRATCH + (((size_t)vocab * 4 + 15) & ~(size_t)15);
    hipLaunchKernelGGL(sample_kernel, dim3(rows), dim3(SAMPLE_THREADS), lds, s, a);
    EMU_CHECK_LAUNCH();
    return 0;
}

bool lookup_sample_ok(int vocab, const emu_sample_params* p, const float* uniforms, int uni_rows) {
    if (!p || vocab < 1 || vocab > EMU_SAMPLE_MAX_VOCAB || p->min_keep < 1 || !(p->repetition_penalty > 0.f)) return false;
    return !p->do_sample || (uniforms && uni_rows >= 1 && p->temperature > 0.f && p->top_p > 0.f);
}

int launch_lookup_sample(const LookupArgs& l, const emu_sample_params* p, const float* uniforms, int uni_rows, hipStream_t s) {
    if (!l.logits || !l.amax || !l.cur || !l.st || !l.out_ids || l.T < 2 || l.T > DECODE_CHUNK_MAX || l.ld < l.V || l.max_new < 1 ||
        !lookup_sample_ok(l.V, p, uniforms, uni_rows))
        return -22;
    SampleArgs a{};
    a.logits = l.logits; a.ld = l.ld; a.vocab = l.V;
    a.uniforms = uniforms; a.uni_ld = 1; a.uni_rows = uni_rows;
    a.penalty = p->repetition_penalty; a.suppress_id = p->suppress_id; a.min_len = p->min_len;
    a.do_sample = p->do_sample; a.temperature = p->temperature; a.top_k = p->top_k; a.top_p = p->top_p; a.min_keep = p->min_keep;
    a.eos_id = p->eos_id; a.pad_id = p->pad_id;
    a.out = l.amax;
    static bool attr_set = false;
    if (int e = sample_lds_attr(lookup_sample_kernel, attr_set)) return e;
    const size_t lds = SAMPLE_SCRATCH + (((size_t)l.V * 4 + 15) & ~(size_t)15);
    hipLaunchKernelGGL(lookup_sample_kernel, dim3(l.T), dim3(SAMPLE_THREADS), lds, s, a, LookupSampleArgs{l.st, l.cur, l.out_ids, l.max_new});
    EMU_CHECK_LAUNCH();
    return 0;
}
