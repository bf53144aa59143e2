// One step of transformers' beam search, on the device, in one launch.
//
// The reference's default decoding mode is lm.generate(num_beams=5, length_penalty=-1, early_stopping=False)
// (Emu2/emu/emu.py:163-172,213-229).  emu_amd/llama.py::beam_search_generate restates the library's vectorised search in ~70
// small torch kernels per step; on a slow host their dispatch alone is 2-3 ms of a 13 ms step (bench leg beam_search_5: 13.2 ms
// per step on one box, 15.8 on another with the same GPU time).  This kernel is that step for the deterministic mode (no sampling
// or repetition penalty -- those keep the torch pipeline or go to beam_sample.hip), in two launches (the first one-workgroup version walked
// global memory in every arg-max round and took 485 us; a register-resident one spilled):
//   1. per (1024-entry vocabulary chunk, beam, prompt): the chunk's softmax statistics and its 2N best logits;
//   2. per prompt: the beams' log-sum-exp from the chunk statistics, the 2N best continuations over beams x vocabulary of
//      log p + running score  (EOS masked while min_length is not reached; ties go to the lower flat index), and
//      the scorer's bookkeeping, statement for statement the host's: the N best non-finished candidates keep running, the
//      finished ones among the first N candidates (EOS or the length limit) compete with the kept results at
//      score / (len ** length_penalty), and the early-stopping heuristic compares the best running beam with the worst kept one.
// Two scorer conventions (BeamStepArgs::hf431): 0 = the vectorised search of transformers 5.x (what is installed here and what the
// golden fixtures pin): a hypothesis that ends -- by EOS or at the length limit -- is scored over cur + 1 tokens, only the first N
// candidates may end, the heuristic looks at the best RUNNING beam.  1 = BeamSearchScorer / BeamHypotheses of transformers 4.31 (the
// release the reference pins, Emu2/requirements.txt:2; restated, not runnable here): an EOS hypothesis is scored over the cur tokens
// before the EOS (`hyp.shape[-1] ** length_penalty`), the heuristic looks at the best of all 2N candidates, and at the length limit
// `finalize` adds every running beam at L ** length_penalty unless the prompt is already done.
// The step index and everything derived from it (EOS suppression below min_len, the length divisors) are read from a device counter
// when one is given, so a captured hipGraph replays the step for every token.
// Out: the N tokens to feed next, the beam each of them extends (flat cache row, for the KV re-order), the updated state.
// Under a constraint (emu_beam_step_trie_bf16; BeamStepArgs::node set) every beam carries a trie node.  Kernel 1 takes the chunk's
// statistics from the unmasked values (the library masks the LOG-PROBABILITIES, after the softmax), then sets a 1024-bit map in LDS
// from the node's edges that fall in the chunk and puts -inf over the rest before the 2N rounds, so a chunk may hand up -inf
// candidates: they rank by index among themselves like every tie.  Kernel 2, after the bookkeeping, moves the nodes with the beams.
// With a no-repeat n-gram ban (emu_beam_step_ngram_bf16; BeamStepArgs::ngram > 0; ngram.h) kernel 1 masks in the same place and the
// same way: the threads share the start positions of the beam's ids running_seq[b, j, :cur], a match whose banned id falls in the
// chunk sets its bit in the LDS map, and the owning lanes put -inf over the marked ids.  The ids follow the beams already.
#include "beam_common.h"
#include "trie.h"
#include "ngram.h"

namespace {

constexpr int BEAM_T = 2 * BEAM_MAXN;                  // candidates a chunk hands up (>= 2N)
constexpr int CHUNK = 1024;                            // vocabulary entries per workgroup of the first kernel
constexpr int PART = 2 + 2 * BEAM_T;                   // floats per chunk partial: max, sum exp, T values, T indices
constexpr int NT = 256, NW = NT / 64;

// block-wide arg-max of (v, i) under before(); every thread gets the winner
__device__ __forceinline__ void block_argmax(float& v, int& i, float* red_v, int* red_i) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        const float ov = __shfl_xor(v, sh, 64);
        const int oi = __shfl_xor(i, sh, 64);
        if (before(ov, oi, v, i)) { v = ov; i = oi; }
    }
    __syncthreads();
    if (lane == 0) { red_v[wave] = v; red_i[wave] = i; }
    __syncthreads();
    v = red_v[0]; i = red_i[0];
#pragma unroll
    for (int w = 1; w < NW; ++w)
        if (before(red_v[w], red_i[w], v, i)) { v = red_v[w]; i = red_i[w]; }
}

// Kernel 1, one workgroup per (vocabulary chunk, beam, prompt): the chunk's softmax statistics and its 2N best logits (within a beam
// the order of the logits is the order of the log-probabilities), EOS masked while min_length is not reached.  4 values per thread,
// held in registers through the 2N arg-max rounds.
__global__ __launch_bounds__(NT) void beam_chunk_kernel(const BeamStepArgs a, float* part, int nchunk) {
    __shared__ float red_v[NW];
    __shared__ int red_i[NW];
    __shared__ unsigned int allow[CHUNK / 32];         // constraint: the chunk's allowed ids; n-gram ban: its banned ids
    const int c = blockIdx.x, j = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cur = a.cur_dev ? *a.cur_dev : a.cur;
    if (cur >= a.L) return;                            // graph replays beyond the length limit are no-ops
    const bool suppress_eos = cur < a.min_len;
    const bf16_t* r = a.logits + (size_t)b * a.ld_prompt + (size_t)j * a.ld_beam;
    float x[4]; int vi[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        vi[e] = c * CHUNK + tid + NT * e;
        x[e] = vi[e] < a.V ? bf2f(r[vi[e]]) : -INFINITY;
    }
    float m = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
    m = wave_max(m);
    __syncthreads();
    if (lane == 0) red_v[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red_v[0], red_v[1]), fmaxf(red_v[2], red_v[3]));
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) sum += (x[e] == -INFINITY) ? 0.f : __expf(x[e] - m);
    sum = wave_sum(sum);
    __syncthreads();
    if (lane == 0) red_v[wave] = sum;
    __syncthreads();
    sum = (red_v[0] + red_v[1]) + (red_v[2] + red_v[3]);
    float* out = part + (((size_t)b * a.nb + j) * nchunk + c) * PART;
    if (tid == 0) { out[0] = m; out[1] = sum; }
    // (the statistics include the EOS logit: the library masks its LOG-PROBABILITY, after the softmax)
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (suppress_eos && vi[e] == a.eos_id) x[e] = -INFINITY;
    if (a.node) {                                      // the constraint, where the library's processor stands: after the suppress
        if (tid < CHUNK / 32) allow[tid] = 0u;
        __syncthreads();
        const int base = c * CHUNK;
        int lo, hi;
        if (trie_edges(a.trie, a.node[(size_t)b * a.nb + j], lo, hi)) {
            for (int e = trie_lower_bound(a.trie.tok, lo, hi, base) + tid; e < hi; e += NT) {
                const int id = a.trie.tok[e] - base;
                if (id >= CHUNK) break;                // ascending ids: the rest lies in later chunks
                if (id >= 0) atomicOr(&allow[id >> 5], 1u << (id & 31));
            }
        } else if (tid == 0 && a.eos_id >= base && a.eos_id < base + CHUNK) {
            allow[(a.eos_id - base) >> 5] = 1u << ((a.eos_id - base) & 31);       // exhausted: EOS alone
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int id = tid + NT * e;
            if (!((allow[id >> 5] >> (id & 31)) & 1u)) x[e] = -INFINITY;
        }
    }
    if (a.ngram > 0 && cur + 1 >= a.ngram) {           // the n-gram ban (a mask on the log-probabilities like the two above)
        __syncthreads();                               // (a constraint's map, were both ever set, is read by now)
        if (tid < CHUNK / 32) allow[tid] = 0u;
        __syncthreads();
        const int base = c * CHUNK;
        ngram_matches(a.running_seq + ((size_t)b * a.nb + j) * a.L, 1, cur, a.ngram, tid, NT, [&](int id) {
            id -= base;
            if (id >= 0 && id < CHUNK) atomicOr(&allow[id >> 5], 1u << (id & 31));
        });
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int id = tid + NT * e;
            if ((allow[id >> 5] >> (id & 31)) & 1u) x[e] = -INFINITY;
        }
    }
    const int T = 2 * a.nb;
    for (int k = 0; k < T; ++k) {
        float bv = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (vi[e] < a.V && before(x[e], vi[e], bv, bi)) { bv = x[e]; bi = vi[e]; }
        block_argmax(bv, bi, red_v, red_i);
        if (tid == 0) { out[2 + k] = bv; out[2 + BEAM_T + k] = __int_as_float(bi); }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (vi[e] == bi) vi[e] = 0x7fffffff;       // taken (its owner retires it)
    }
}

// Kernel 2, one workgroup per prompt: log-sum-exp of every beam from the chunk statistics, the 2N best of the N x chunks x 2N handed-up
// candidates of (log p + running score) -- ties to the lower flat index --, then the scorer's bookkeeping.
__global__ __launch_bounds__(NT) void beam_step_kernel(const BeamStepArgs a, const float* part, int nchunk) {
    __shared__ float red_v[NW];
    __shared__ int red_i[NW];
    __shared__ float s_lse[BEAM_MAXN], s_rs[BEAM_MAXN];
    __shared__ float top_lp[2 * BEAM_MAXN];
    __shared__ int top_idx[2 * BEAM_MAXN];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nb = a.nb, V = a.V, L = a.L, cur = a.cur_dev ? *a.cur_dev : a.cur;
    if (cur >= L) return;
    const float* run_sc = a.running_scores + (size_t)b * nb;
    const float* pb = part + (size_t)b * nb * nchunk * PART;

    if (tid < nb) {                                    // log-sum-exp of beam tid over its chunks (fixed order)
        float m = -INFINITY;
        for (int c = 0; c < nchunk; ++c) m = fmaxf(m, pb[((size_t)tid * nchunk + c) * PART]);
        float sum = 0.f;
        for (int c = 0; c < nchunk; ++c) {
            const float* q = pb + ((size_t)tid * nchunk + c) * PART;
            sum += q[0] == -INFINITY ? 0.f : q[1] * __expf(q[0] - m);
        }
        s_lse[tid] = m + __logf(sum);
        s_rs[tid] = run_sc[tid];
    }
    __syncthreads();
    const int T = 2 * nb, ncand = nb * nchunk * T;
    float pv = INFINITY; int pi = -1;                  // last pick (everything taken ranks before or at it)
    for (int k = 0; k < T; ++k) {
        float bv = -INFINITY; int bi = 0x7fffffff;
        for (int q = tid; q < ncand; q += NT) {
            const int t = q % T, jc = q / T, j = jc / nchunk;
            const float* pq = pb + (size_t)jc * PART;
            const int v = __float_as_int(pq[2 + BEAM_T + t]);
            if (v == 0x7fffffff) continue;             // the chunk had fewer than T live entries
            const float x = (pq[2 + t] - s_lse[j]) + s_rs[j];
            const int idx = j * V + v;
            const bool taken = pi >= 0 && !before(pv, pi, x, idx);
            if (!taken && before(x, idx, bv, bi)) { bv = x; bi = idx; }
        }
        block_argmax(bv, bi, red_v, red_i);
        if (tid == 0) { top_lp[k] = bv; top_idx[k] = bi; }
        pv = bv; pi = bi;
    }
    __syncthreads();
    beam_bookkeeping<NT>(a, b, cur, top_lp, top_idx);
    if (a.node) {                                      // the new beam tid continues an old one: its node follows, by the token it took
        int nn = -1;
        if (tid < nb) {                                // (next_tok / beam_flat of this entry were written by this very thread)
            const int src = (int)(a.beam_flat[b * nb + tid] - (long)b * nb);
            if (src >= 0 && src < nb) nn = trie_child(a.trie, a.node[(size_t)b * nb + src], a.next_tok[b * nb + tid]);
        }
        __syncthreads();                               // every old node is read before the first new one is written
        if (tid < nb) a.node[(size_t)b * nb + tid] = nn;
    }
}

// ---- the rest of a beam step that used to be host work: with this and launch_step_advance (attention.hip) the whole step {advance,
// re-order, embed, 60 layers, logits, beam_step_kernel} reads its step index from a device counter and is replayed from one hipGraph.
// transformers' _reorder_cache for the GENERATED slots [slot0, slot0 + cur - 1) (the prompt's slots are shared by the beams of a
// group and never move): cache row r takes the slots of row beam_flat[r].  In place: one workgroup owns a (layer, head, slot) of
// all the rows of a group -- it loads the nb source vectors, then stores them (a barrier in between).  grid = (layers * heads,
// slot chunks, groups); D / 8 lanes per row.
template <int D>
__global__ __launch_bounds__(256) void beam_reorder_kernel(bf16_t* kc, bf16_t* vc, const long* beam_flat, const int32_t* cur_dev,
                                                           int rows, int Hl, int s_max, int nb, int slot0, int L, int chunk) {
    constexpr int LPR = D / 8;                         // lanes per row (16-byte pieces)
    const int c = *cur_dev;
    if (c >= L) return;
    const int ngen = c - 1;
    const int lh = blockIdx.x, layer = lh / Hl, h = lh - layer * Hl, grp = blockIdx.z;
    const int j = threadIdx.x / LPR, piece = threadIdx.x - j * LPR;
    const bool live = j < nb;
    const int dst_row = grp * nb + j;
    const int src_row = live ? (int)beam_flat[dst_row] : 0;
    const size_t plane = (size_t)rows * Hl * s_max * D;
    for (int sl = blockIdx.y * chunk; sl < ngen && sl < (blockIdx.y + 1) * chunk; ++sl) {
        const size_t so = (((size_t)layer * rows + src_row) * Hl + h) * s_max + slot0 + sl;
        const size_t dofs = (((size_t)layer * rows + dst_row) * Hl + h) * s_max + slot0 + sl;
        u32x4 kv, vv;
        if (live) { kv = ld16(kc + so * D + piece * 8); vv = ld16(vc + so * D + piece * 8); }
        __syncthreads();                               // every source of this slot is in registers
        if (live) { st16(kc + dofs * D + piece * 8, kv); st16(vc + dofs * D + piece * 8, vv); }
        __syncthreads();
    }
    (void)plane;
}

}  // namespace

int launch_beam_reorder(bf16_t* kc, bf16_t* vc, const long* beam_flat, const int32_t* cur_dev, int layers, int rows, int Hl, int s_max,
                        int D, int nb, int slot0, int L, hipStream_t s) {
    if (!kc || !vc || !beam_flat || !cur_dev || nb < 1 || nb > BEAM_MAXN || rows % nb || (D != 64 && D != 128) ||
        slot0 < 0 || slot0 + L > s_max + 1)
        return -22;
    if (L < 2) return 0;                               // never a generated slot to move
    constexpr int CHUNK_SLOTS = 8;
    const dim3 grid(layers * Hl, (L - 1 + CHUNK_SLOTS - 1) / CHUNK_SLOTS, rows / nb);
    if (D == 128) hipLaunchKernelGGL(beam_reorder_kernel<128>, grid, dim3(nb * 16 <= 128 ? 128 : 256), 0, s, kc, vc, beam_flat, cur_dev, rows, Hl, s_max, nb, slot0, L, CHUNK_SLOTS);
    else hipLaunchKernelGGL(beam_reorder_kernel<64>, grid, dim3(64), 0, s, kc, vc, beam_flat, cur_dev, rows, Hl, s_max, nb, slot0, L, CHUNK_SLOTS);
    EMU_CHECK_LAUNCH();
    return 0;
}

size_t beam_step_ws_floats(int B, int nb, int V) { return (size_t)B * nb * ((V + CHUNK - 1) / CHUNK) * PART; }

int launch_beam_step(const BeamStepArgs& a, float* ws, size_t ws_floats, hipStream_t s) {
    if (a.B < 1 || a.nb < 1 || a.nb > BEAM_MAXN || a.L < 1 || a.L > BEAM_MAXL || (!a.cur_dev && (a.cur < 0 || a.cur >= a.L)) || a.V < 2 * a.nb ||
        a.min_len < 0 || !ws || ws_floats < beam_step_ws_floats(a.B, a.nb, a.V))
        return -22;
    if (a.node && !trie_args_ok(&a.trie, a.node)) return -22;
    if (a.ngram < 0) return -22;
    const int nchunk = (a.V + CHUNK - 1) / CHUNK;
    hipLaunchKernelGGL(beam_chunk_kernel, dim3(nchunk, a.nb, a.B), dim3(NT), 0, s, a, ws, nchunk);
    hipLaunchKernelGGL(beam_step_kernel, dim3(a.B), dim3(NT), 0, s, a, ws, nchunk);
    EMU_CHECK_LAUNCH();
    return 0;
}
